"""The branch of SG3/genlib/metric/metric_utils.py `get_outdir_model_path` (:37-93) that the projector takes: a snapshot
named by file name inside the one training run whose directory name contains the experiment id.  The other branch
(pick the snapshot with the best FID from the metric jsonl files, asking on stdin for the modality) is not ported."""
import os


def get_outdir_model_path(outdir, outdir_model, experiment, metric_name='fid50k_full', modalities=None, snap=10,
                          projector_kwargs=None, logplot=False):
    """<outdir_model>/<the run containing `experiment`>/<metric_name>; also stored in projector_kwargs (network_pkl,
    outdir_model) when given.  An absolute path to an existing file in `metric_name` is taken as is."""
    if metric_name == 'fid50k_full':
        raise NotImplementedError('selecting the snapshot by its FID is not ported: name the snapshot file '
                                  '(--network_pkl network-snapshot-XXXXXX.pkl)')
    if os.path.isabs(metric_name) and os.path.isfile(metric_name):
        path = metric_name
    else:
        runs = [x for x in os.listdir(outdir_model) if experiment in x]
        if len(runs) != 1:
            raise RuntimeError(f'expected exactly one training run matching {experiment!r} under {outdir_model}, '
                               f'found {sorted(runs)}')
        path = os.path.join(outdir_model, runs[0], metric_name)
    if projector_kwargs is not None:
        projector_kwargs.network_pkl = metric_name
        projector_kwargs.outdir_model = path
    print(f'Snapshot selected:           {metric_name}')
    print(f'Outdir model:                {path}')
    return path
