"""Style mixing: the images of the row seeds with the styles `--styles` replaced by those of the column seeds -- the
reference's src/models/gen_images_style_mixing.py without its prompt, YAML and run-directory scaffolding.

    python gan-track_amd/gen_images_style_mixing.py --network=network-snapshot-005000.pkl --rows=85,100,75 \\
        --cols=55,821,1789 --styles=10-13 --outdir=out

Writes OUTDIR/<modality>/<row>-<col>.png for every mix, <seed>-<seed>.png for every source, and
OUTDIR/<modality>/grid.png: a black top-left cell, the column sources along the top, the row sources down the left
and the mixes inside.  As in the reference the sources are rendered with force_fp32=True and the mixes without it,
and w is truncated as w_avg + (w - w_avg) * psi.  Every image is converted to uint8 straight into its grid cell on
the device (genlib/generate.py); the files are cut from the finished grids.
"""
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import click  # noqa: E402

from gen_images_mi_multimodal import _range  # noqa: E402


def style_mixing(G, modalities, rows, cols, styles, outdir, truncation_psi=1.0, noise_mode='const'):
    """The CLI's body on a loaded generator.  Returns {modality: the [(R + 1) * H, (C + 1) * W] uint8 grid}."""
    import torch
    from genlib import generate
    if not rows or not cols:
        raise ValueError('--rows and --cols need at least one seed each')
    if min(styles) < 0 or max(styles) >= G.num_ws:
        raise ValueError(f'--styles must lie in 0..{G.num_ws - 1} for this generator; got {styles}')
    res = G.img_resolution
    seeds = sorted(set(rows + cols))
    with torch.no_grad():
        z = generate.seeds_to_z(seeds, G.z_dim).to(next(G.parameters()).device)
        w_all = generate.truncate(G.mapping(z, generate.class_label(G, None, len(seeds))), G.mapping.w_avg,
                                  truncation_psi)
    w = dict(zip(seeds, w_all))
    grid = (len(cols) + 1, len(rows) + 1)
    canvases = [generate.new_canvas(G, grid) for _ in modalities]
    kw = dict(noise_mode=noise_mode, batch=1, tiles='channels', grid=grid)
    generate.synthesize_tiles(G, torch.stack([w[s] for s in cols]), canvases, first_tile=1, force_fp32=True, **kw)
    for r, row in enumerate(rows):
        first = (r + 1) * grid[0]
        generate.synthesize_tiles(G, w[row].unsqueeze(0), canvases, first_tile=first, force_fp32=True, **kw)
        mixes = torch.stack([generate.mix_styles(w[row], w[col], styles) for col in cols])
        generate.synthesize_tiles(G, mixes, canvases, first_tile=first + 1, **kw)
    out = {}
    for m, canvas in zip(modalities, canvases):
        host = canvas.cpu().numpy()[:, :, 0]
        os.makedirs(os.path.join(outdir, m), exist_ok=True)
        for c, col in enumerate(cols):
            generate.save_grey(os.path.join(outdir, m, f'{col}-{col}.png'), generate.cell(host, c + 1, grid, res))
        for r, row in enumerate(rows):
            first = (r + 1) * grid[0]
            generate.save_grey(os.path.join(outdir, m, f'{row}-{row}.png'), generate.cell(host, first, grid, res))
            for c, col in enumerate(cols):
                generate.save_grey(os.path.join(outdir, m, f'{row}-{col}.png'),
                                   generate.cell(host, first + 1 + c, grid, res))
        generate.save_grey(os.path.join(outdir, m, 'grid.png'), host)
        out[m] = host
    return out


@click.command()
@click.option('--network', 'network_pkl', help='Network snapshot (network-snapshot-*.pkl)', required=True)
@click.option('--rows', callback=_range, help="Seeds of the row images, e.g. '85,100,75'", required=True)
@click.option('--cols', callback=_range, help="Seeds of the column images, e.g. '55,821'", required=True)
@click.option('--styles', callback=_range, help='Style layers taken from the column image', default='10-13',
              show_default=True)
@click.option('--trunc', 'truncation_psi', type=float, help='Truncation psi', default=1.0, show_default=True)
@click.option('--noise-mode', type=click.Choice(['const', 'random', 'none']), help='Noise mode', default='const',
              show_default=True)
@click.option('--modalities', type=str, default=None,
              help="Channel names, comma separated [default: the snapshot's training-set modalities, else ch0,ch1,...]")
@click.option('--outdir', help='Where to save the images', type=str, required=True, metavar='DIR')
def main(network_pkl, rows, cols, styles, truncation_psi, noise_mode, modalities, outdir):
    """Generate a style-mixing grid per modality."""
    import torch
    from genlib import generate
    print(f'Loading networks from "{network_pkl}"...')
    G, ts_kwargs = generate.load_snapshot(network_pkl, torch.device('cuda'))
    try:
        names = generate.snapshot_modalities(G, ts_kwargs, modalities)
        style_mixing(G, names, rows, cols, styles, outdir, truncation_psi, noise_mode)
    except ValueError as err:
        raise click.ClickException(str(err))
    print(f'Wrote {len(names)} grids of {len(rows) + 1} x {len(cols) + 1} cells to {outdir}')


if __name__ == '__main__':
    main()   # pylint: disable=no-value-for-parameter
