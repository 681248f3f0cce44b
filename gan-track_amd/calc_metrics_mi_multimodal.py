"""Offline evaluation of a snapshot: SG3/calc_metrics_mi_multimodal.py -- every requested metric, per modality,
on the G_ema of a network pickle, one JSON line per evaluation printed and (inside a training run's directory)
appended to metric-<modality>-<metric>.jsonl.

    python calc_metrics_mi_multimodal.py --network <run_dir>/network-snapshot-000200.pkl \\
        --metrics fid50k_full,kid50k,pr50k3_full,ppl2_wend

The dataset options come from --data, or else from the snapshot's own training_set_kwargs.  The snapshot is read by
this build's legacy.load_network_pkl (nothing embedded in the pickle is executed) and must be a local file; the
detectors are supplied offline (SG2_FID_DETECTOR, SG2_PR_DETECTOR; metrics/metric_utils.py).  With --gpus > 1 one
fresh process per GPU is spawned and the ranks meet over a file store with the 'nccl' backend (RCCL).
"""
import copy
import json
import os
import tempfile

import click
import torch

import dnnlib
import legacy
from metrics import metric_main_mi_multimodal as metric_main
from metrics import metric_utils


def _device(rank):
    return torch.device('cuda', rank)


def parse_comma_separated_list(s):
    if isinstance(s, (list, tuple)):
        return list(s)
    if s is None or s == '' or s.lower() == 'none':
        return []
    return [part for part in s.replace(' ', '').split(',') if part]


def subprocess_fn(rank, args, temp_dir):
    device = _device(rank)
    try:
        if args.num_gpus > 1:       # (a fresh child process per rank)
            from torch_utils import training_stats
            init_file = os.path.abspath(os.path.join(temp_dir, '.torch_distributed_init'))
            torch.cuda.set_device(rank)
            torch.distributed.init_process_group(backend='nccl', init_method=f'file://{init_file}', rank=rank,
                                                 world_size=args.num_gpus)
            training_stats.init_multiprocessing(rank=rank, sync_device=device)
        G = copy.deepcopy(args.G).eval().requires_grad_(False).to(device)
        for metric in args.metrics:
            if rank == 0 and args.verbose:
                print(f'Calculating {metric}...')
            progress = metric_utils.ProgressMonitor(verbose=args.verbose)
            for mode_idx, mode in enumerate(args.dataset_kwargs.modalities):
                result = metric_main.calc_metric(metric=metric, G=G, dataset_kwargs=args.dataset_kwargs,
                                                 num_gpus=args.num_gpus, rank=rank, device=device,
                                                 cache=args.metrics_cache, progress=progress,
                                                 mode_dict={'mode_name': mode, 'mode_idx': mode_idx})
                if rank == 0:
                    metric_main.report_metric(result, mode=mode, run_dir=args.run_dir, snapshot_pkl=args.network_pkl)
            if rank == 0 and args.verbose:
                print()
        if rank == 0 and args.verbose:
            print('Exiting...')
    finally:
        if args.num_gpus > 1 and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def build_args(network_pkl, metrics, data, mirror, dtype, modalities, dataset, split, metrics_cache, gpus, verbose):
    """The evaluation's options (metrics, G, dataset_kwargs, run_dir, ...) from the command line's; raises
    click.ClickException on a bad one.  (--dataset is accepted for the reference's job scripts and unused, as there.)"""
    args = dnnlib.EasyDict(metrics=parse_comma_separated_list(metrics), num_gpus=gpus, network_pkl=network_pkl,
                           verbose=verbose, metrics_cache=bool(metrics_cache))
    unknown = [m for m in args.metrics if not metric_main.is_valid_metric(m)]
    if unknown:
        raise click.ClickException('\n'.join([f'--metrics: unknown {", ".join(unknown)}; it can only contain the '
                                              f'following values:'] + metric_main.list_valid_metrics()))
    if not args.num_gpus >= 1:
        raise click.ClickException('--gpus must be at least 1')
    if not os.path.isfile(network_pkl):
        raise click.ClickException('--network must point to a snapshot file')
    if args.verbose:
        print(f'Loading network from "{network_pkl}"...')
    with open(network_pkl, 'rb') as f:
        network_dict = legacy.load_network_pkl(f)
    args.G = network_dict['G_ema']

    if data is not None:
        args.dataset_kwargs = dnnlib.EasyDict(class_name='training.dataset_mi_multimodal.CustomImageFolderDataset',
                                              path=data, dtype=dtype, use_labels=True, max_size=None, xflip=False,
                                              split=split, modalities=parse_comma_separated_list(modalities))
    elif network_dict['training_set_kwargs'] is not None:
        args.dataset_kwargs = dnnlib.EasyDict(network_dict['training_set_kwargs'])
        args.dataset_kwargs.modalities = parse_comma_separated_list(args.dataset_kwargs.modalities)
    else:
        raise click.ClickException('Could not look up dataset options; please specify --data')
    args.dataset_kwargs.resolution = args.G.img_resolution
    args.dataset_kwargs.use_labels = (args.G.c_dim != 0)
    if mirror is not None:
        args.dataset_kwargs.xflip = mirror
    if args.verbose:
        print('Dataset options:')
        print(json.dumps(args.dataset_kwargs, indent=2))

    args.run_dir = None
    pkl_dir = os.path.dirname(network_pkl)
    if os.path.isfile(os.path.join(pkl_dir, 'training_options.json')):
        args.run_dir = pkl_dir
    return args


@click.command()
@click.option('network_pkl', '--network', help='Network pickle filename', metavar='PATH', required=True)
@click.option('--metrics', help='Quality metrics', metavar='[NAME|A,B,C|none]', type=parse_comma_separated_list,
              default='fid50k_full', show_default=True)
@click.option('--data', help='Dataset to evaluate against  [default: look up]', metavar='[ZIP|DIR]')
@click.option('--mirror', help='Enable dataset x-flips  [default: look up]', type=bool, metavar='BOOL')
@click.option('--dtype', help='Dynamic range of images', type=str, default='float32')
@click.option('--modalities', help='Modalities for StyleGAN', metavar='STRING', type=str,
              default='MR_nonrigid_CT,MR_MR_T2')
@click.option('--dataset', help='Dataset name', metavar='STRING', type=str, default='Pelvis_2.1')
@click.option('--split', help='Validation split', metavar='STRING', type=str, default='train')
@click.option('--metrics_cache', help='Use cache to upload precomputed features for real images', type=bool,
              default=False)
@click.option('--gpus', help='Number of GPUs to use', type=int, default=1, metavar='INT', show_default=True)
@click.option('--verbose', help='Print optional information', type=bool, default=True, metavar='BOOL', show_default=True)
def calc_metrics(**kwargs):
    """Calculate quality metrics of a training run's snapshot, per modality.

    \b
    Metrics:
      fid50k_full    Frechet inception distance against the full dataset.
      pr50k3_full    Precision and recall against the full dataset.
      ppl2_wend      Perceptual path length in W, endpoints, full image.
      fid50k         Frechet inception distance against 50k real images.
      pr50k3         Precision and recall against 50k real images.
      kid50k         Kernel inception distance against 50k real images.
      prdc50k5_full  Precision, recall, density and coverage (k = 5) against the full dataset.
      prdc50k5       Precision, recall, density and coverage (k = 5) against 50k real images.
    """
    args = build_args(**kwargs)
    if args.verbose:
        print('Launching processes...')
    with tempfile.TemporaryDirectory() as temp_dir:
        if args.num_gpus == 1:
            subprocess_fn(rank=0, args=args, temp_dir=temp_dir)
        else:
            torch.multiprocessing.spawn(fn=subprocess_fn, args=(args, temp_dir), nprocs=args.num_gpus)


if __name__ == '__main__':
    calc_metrics()   # pylint: disable=no-value-for-parameter
