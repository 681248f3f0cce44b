"""Render a latent interpolation through the seeds of a trained generator, one modality as grey tiles -- the reference's
SG3/gen_video.py.

    python gan-track_amd/gen_video.py --network=network-snapshot-005000.pkl --seeds=0-31 --grid=4x2 --trunc=1 \\
        --output=frames/            # frame_%05d.png
        --output=lerp.mp4           # needs the imageio package

The W x H cells of --grid each run through their own keyframes (len(seeds) / (W * H) of them unless --num-keyframes
says otherwise) on a periodic cubic curve, --w-frames frames from one keyframe to the next.  Every frame is
synthesised with noise_mode='const' and converted to a uint8 [H * res, W * res] canvas on the device
(genlib/generate.py); only that canvas goes to the host.  Each seed is mapped on its own, so a keyframe is the image
gen_images_mi_multimodal.py makes of that seed.
"""
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import click  # noqa: E402
import numpy as np  # noqa: E402

from gen_images_mi_multimodal import _range, _tuple  # noqa: E402


def keyframe_seeds(seeds, grid, num_keyframes=None, shuffle_seed=None):
    """The seed of every (cell, keyframe), cell-major: seeds repeated to gh * gw * num_keyframes entries, optionally
    shuffled by RandomState(shuffle_seed).  Returns (int64 array, num_keyframes)."""
    cells = grid[0] * grid[1]
    if num_keyframes is None:
        if len(seeds) % cells != 0:
            raise ValueError('Number of input seeds must be divisible by grid W*H')
        num_keyframes = len(seeds) // cells
    if num_keyframes < 1:
        raise ValueError('--num-keyframes must be at least 1')
    out = np.array([seeds[i % len(seeds)] for i in range(num_keyframes * cells)], dtype=np.int64)
    if shuffle_seed is not None:
        np.random.RandomState(seed=shuffle_seed).shuffle(out)
    return out, num_keyframes


def frames(G, seeds, grid=(1, 1), num_keyframes=None, w_frames=120, shuffle_seed=None, truncation_psi=1.0, channel=0,
           kind='cubic', wraps=2):
    """Yields num_keyframes * w_frames uint8 arrays [gh * res, gw * res]."""
    import torch
    from genlib import generate
    all_seeds, num_keyframes = keyframe_seeds(seeds, grid, num_keyframes, shuffle_seed)
    ws = generate.map_seeds(G, all_seeds, None, truncation_psi, None, batch=1)
    ws = ws.reshape(grid[1] * grid[0], num_keyframes, *ws.shape[1:])
    curves = [generate.interp_ws(w, w_frames, wraps=wraps, kind=kind) for w in ws]
    for per_cell in zip(*curves):
        canvas = generate.new_canvas(G, grid)
        generate.synthesize_tiles(G, torch.stack(per_cell).to(ws.device), canvas, noise_mode='const', batch=1,
                                  tiles=int(channel), grid=grid)
        yield canvas.cpu().numpy()[:, :, 0]


@click.command()
@click.option('--network', 'network_pkl', help='Network snapshot (network-snapshot-*.pkl)', required=True)
@click.option('--seeds', callback=_range, help='List of random seeds', required=True)
@click.option('--shuffle-seed', type=int, help='Random seed to use for shuffling seed order', default=None)
@click.option('--grid', callback=_tuple, help="Grid width/height, e.g. '4x3'", default='1x1', show_default=True)
@click.option('--num-keyframes', type=int, default=None,
              help='Number of seeds to interpolate through [default: len(seeds) / (W*H)]')
@click.option('--w-frames', type=click.IntRange(min=1), help='Number of frames to interpolate between latents',
              default=120, show_default=True)
@click.option('--trunc', 'truncation_psi', type=float, help='Truncation psi', default=1.0, show_default=True)
@click.option('--modality', type=str, default=None, help='Channel to render: a name or an index [default: the first]')
@click.option('--output', help="Output: a directory for frame_%05d.png, or an .mp4 file (needs imageio)", type=str,
              required=True, metavar='DIR|FILE')
def main(network_pkl, seeds, shuffle_seed, grid, num_keyframes, w_frames, truncation_psi, modality, output):
    """Render a latent vector interpolation as frames or a video."""
    import torch
    from genlib import generate
    video = None
    if output.lower().endswith('.mp4') and not os.path.isdir(output):
        try:
            import imageio
        except ImportError as err:
            raise click.ClickException('an .mp4 --output needs the imageio package, which is not installed; give a '
                                       'directory to get frame_%05d.png files instead') from err
        video = imageio.get_writer(output, mode='I', fps=60, codec='libx264', bitrate='12M')
    print(f'Loading networks from "{network_pkl}"...')
    G, ts_kwargs = generate.load_snapshot(network_pkl, torch.device('cuda'))
    try:
        names = generate.snapshot_modalities(G, ts_kwargs)
        if modality is None:
            channel = 0
        elif modality in names:
            channel = names.index(modality)
        elif modality.isdigit() and int(modality) < G.img_channels:
            channel = int(modality)
        else:
            raise ValueError(f'--modality {modality}: not one of {names} nor a channel index below {G.img_channels}')
        if video is None:
            os.makedirs(output, exist_ok=True)
        count = 0
        for count, frame in enumerate(frames(G, seeds, grid, num_keyframes, w_frames, shuffle_seed, truncation_psi,
                                             channel), 1):
            if video is None:
                generate.save_grey(os.path.join(output, f'frame_{count - 1:05d}.png'), frame)
            else:
                video.append_data(frame)
    except ValueError as err:
        raise click.ClickException(str(err))
    finally:
        if video is not None:
            video.close()
    print(f'Wrote {count} frames to {output}')


if __name__ == '__main__':
    main()   # pylint: disable=no-value-for-parameter
