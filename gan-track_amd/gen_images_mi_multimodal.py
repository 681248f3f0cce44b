"""Generate images from a network snapshot, one 8-bit greyscale PNG per modality and seed -- the reference's
src/models/gen_images*.py and SG3/gen_images.py without their prompts and run-directory scaffolding.

    python gan-track_amd/gen_images_mi_multimodal.py --network=network-snapshot-005000.pkl --seeds=0-31 --trunc=0.7 \\
        --outdir=out [--grid=8x8] [--raw]

Writes OUTDIR/<modality>/seed%04d.png; with --grid also OUTDIR/grid.png, every channel of every seed as grey tiles
(seed-major, the order of the training loop's snapshot grids); with --raw also OUTDIR/seed%04d.npy, the generator's
float32 [C, H, W] output.  The float image becomes uint8 tiles on the device in one kernel per batch
(genlib/generate.py); SG2_GEN_FUSED=0 selects the reference's torch composition instead.
"""
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import click  # noqa: E402
import numpy as np  # noqa: E402


def _range(ctx, param, value):
    from genlib import generate
    try:
        return None if value is None else generate.parse_range(value)
    except ValueError as err:
        raise click.BadParameter(str(err))


def _tuple(ctx, param, value):
    from genlib import generate
    try:
        return None if value is None else generate.parse_tuple(value)
    except ValueError as err:
        raise click.BadParameter(str(err))


def generate_images(G, modalities, seeds, outdir, truncation_psi=1.0, truncation_cutoff=None, noise_mode='const',
                    class_idx=None, batch=1, grid=None, raw=False):
    """The CLI's body on a loaded generator.  Returns the list of files written."""
    from genlib import generate
    res, ch = G.img_resolution, G.img_channels
    if grid is not None and grid[0] * grid[1] < len(seeds) * ch:
        raise click.ClickException(f'--grid {grid[0]}x{grid[1]} has fewer cells than {len(seeds)} seeds x {ch} '
                                   f'channels')
    label = generate.class_label(G, class_idx)
    for m in modalities:
        os.makedirs(os.path.join(outdir, m), exist_ok=True)
    batch = max(int(batch), 1)
    written = []
    # with --grid one canvas holds every seed; without, a canvas per batch (one row of C tiles per seed)
    canvas = generate.new_canvas(G, grid) if grid is not None else None
    for i in range(0, len(seeds), batch):
        chunk = seeds[i:i + batch]
        ws = generate.map_seeds(G, chunk, label, truncation_psi, truncation_cutoff)
        keep = [] if raw else None
        if grid is not None:
            generate.synthesize_tiles(G, ws, canvas, first_tile=i * ch, noise_mode=noise_mode, batch=batch,
                                      tiles='grey', grid=grid, keep=keep)
        else:
            part = generate.new_canvas(G, (ch, len(chunk)))
            generate.synthesize_tiles(G, ws, part, noise_mode=noise_mode, batch=batch, tiles='grey',
                                      grid=(ch, len(chunk)), keep=keep)
            host = part.cpu().numpy()
            for j, seed in enumerate(chunk):
                for k, m in enumerate(modalities):
                    written.append(os.path.join(outdir, m, f'seed{seed:04d}.png'))
                    generate.save_grey(written[-1], generate.cell(host, j * ch + k, (ch, len(chunk)), res))
        if raw:
            for seed, img in zip(chunk, keep[0].float().cpu().numpy()):
                written.append(os.path.join(outdir, f'seed{seed:04d}.npy'))
                np.save(written[-1], img)
    if grid is not None:
        host = canvas.cpu().numpy()
        for j, seed in enumerate(seeds):
            for k, m in enumerate(modalities):
                written.append(os.path.join(outdir, m, f'seed{seed:04d}.png'))
                generate.save_grey(written[-1], generate.cell(host, j * ch + k, grid, res))
        written.append(os.path.join(outdir, 'grid.png'))
        generate.save_grey(written[-1], host)
    return written


@click.command()
@click.option('--network', 'network_pkl', help='Network snapshot (network-snapshot-*.pkl)', required=True)
@click.option('--seeds', callback=_range, help="Random seeds, e.g. '0,1,4-6'", required=True)
@click.option('--trunc', 'truncation_psi', type=float, help='Truncation psi', default=1.0, show_default=True)
@click.option('--trunc-cutoff', 'truncation_cutoff', type=int, help='Truncate only the first N style layers',
              default=None)
@click.option('--noise-mode', type=click.Choice(['const', 'random', 'none']), help='Noise mode', default='const',
              show_default=True)
@click.option('--class', 'class_idx', type=int, help='Class label (conditional generators)', default=None)
@click.option('--modalities', type=str, default=None,
              help="Channel names, comma separated [default: the snapshot's training-set modalities, else ch0,ch1,...]")
@click.option('--outdir', help='Where to save the images', type=str, required=True, metavar='DIR')
@click.option('--batch', type=click.IntRange(min=1), default=1, show_default=True,
              help="Seeds per generator call (1: the reference's per-seed calls)")
@click.option('--grid', callback=_tuple, default=None,
              help="Also write grid.png with WxH grey tiles, e.g. '8x4' (needs W*H >= seeds x channels)")
@click.option('--raw', is_flag=True, help='Also write seed%04d.npy, the float32 [C, H, W] generator output')
def main(network_pkl, seeds, truncation_psi, truncation_cutoff, noise_mode, class_idx, modalities, outdir, batch, grid,
         raw):
    """Generate per-modality images from the seeds of a trained generator."""
    import torch
    from genlib import generate
    print(f'Loading networks from "{network_pkl}"...')
    G, ts_kwargs = generate.load_snapshot(network_pkl, torch.device('cuda'))
    try:
        names = generate.snapshot_modalities(G, ts_kwargs, modalities)
        if G.c_dim == 0 and class_idx is not None:
            print('warning: --class is ignored by an unconditional generator')
        files = generate_images(G, names, seeds, outdir, truncation_psi, truncation_cutoff, noise_mode, class_idx, batch,
                                grid, raw)
    except ValueError as err:
        raise click.ClickException(str(err))
    print(f'Wrote {len(files)} files to {outdir}')


if __name__ == '__main__':
    main()   # pylint: disable=no-value-for-parameter
