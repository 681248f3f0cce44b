"""Score the projections of a run against their targets: MSE, PSNR and SSIM per patient, slice and modality
(genlib/projector/score.py; SSIM and MSE on the fused float64 kernel of torch_utils/ops/ssim.py).

    python gan-track_amd/genlib/score_projections.py --run PROJECTION_RUN_DIR [--data ZIP] [--network PKL] \\
        [--batch 16] [--data-range 255] [--lpips] [--maps]

Reads <run>/training_options.json and <run>/projected_w, writes <run>/reconstruction.csv and reconstruction.json and
prints the per-modality table.  --data and --network name the dataset and the snapshot when they have moved since the
run.  --lpips adds the squared LPIPS-feature distance (needs the detector the projector needs: SG2_LPIPS_DETECTOR /
SG2_PR_DETECTOR); --maps writes the SSIM maps as 8-bit PNGs under <run>/<patient>/<modality>/ssim_map/.  One process.
"""
import os
import pickle
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import click  # noqa: E402


@click.command()
@click.option('--run', 'run_dir', help='Projection run directory', metavar='DIR', required=True,
              type=click.Path(exists=True, file_okay=False))
@click.option('--data', help='Dataset, when it has moved since the run', metavar='[ZIP|DIR]', type=str, default=None)
@click.option('--network', help='Snapshot, when it has moved since the run', metavar='PKL', type=str, default=None)
@click.option('--batch', help='Slices rendered and scored per call', metavar='INT', type=click.IntRange(min=1),
              default=16, show_default=True)
@click.option('--data-range', 'data_range', help='Dynamic range L of the images', type=click.FloatRange(min=0,
              min_open=True), default=255.0, show_default=True)
@click.option('--lpips', help='Add the squared LPIPS-feature distance per modality', is_flag=True)
@click.option('--maps', help='Write the SSIM maps as PNGs', is_flag=True)
def main(run_dir, data, network, batch, data_range, lpips, maps):
    from genlib.projector import score
    try:
        score.score_run(run_dir, data=data, network=network, batch=batch, data_range=data_range, lpips=lpips,
                        maps=maps)
    except (RuntimeError, IOError, pickle.UnpicklingError) as err:
        raise click.ClickException(str(err))


if __name__ == '__main__':
    main()   # pylint: disable=no-value-for-parameter
