"""Compare average power spectra between real and generated images, or between generators, per modality -- the
reference's SG3/avg_spectra.py on the fused power-spectrum kernel (genlib/spectra.py, torch_utils/ops/power_spectrum.py).

    # per-modality mean and std of the training slices, needed by calc
    python gan-track_amd/avg_spectra.py stats --source=claro.zip --modalities=CT,MR
    # average spectrum of the data and of a snapshot (one .npz per modality: tmp/data-CT.npz, tmp/data-MR.npz, ...)
    python gan-track_amd/avg_spectra.py calc --source=claro.zip --modalities=CT,MR --dest=tmp/data.npz \\
        --mean=112.7,98.2 --std=69.5,61.0
    python gan-track_amd/avg_spectra.py calc --source=network-snapshot-005000.pkl --dest=tmp/gen.npz \\
        --mean=112.7,98.2 --std=69.5,61.0 --num=50000
    # display, or save with --save
    python gan-track_amd/avg_spectra.py heatmap tmp/data-CT.npz --save=tmp/data-CT.png --dpi=300
    python gan-track_amd/avg_spectra.py slices tmp/data-CT.npz tmp/gen-CT.npz --save=tmp/slices-CT.png

Sources are local files: a network snapshot .pkl (--num required) or the dataset zip of per-slice pickles.  Images are
8-bit on both sides by default (generated: the reference's quantisation; real: clamped and truncated); --float skips
that.  SG2_SPECTRA_FUSED=0 selects the reference's torch composition instead of the fused kernel, =1 the kernel at every
size it takes; by default the kernel runs below 512 x 512 (torch_utils/ops/power_spectrum.py).
"""
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import click  # noqa: E402
import numpy as np  # noqa: E402


def _device():
    import torch
    return torch.device('cuda')


def _source_options(f):
    for opt in reversed([
        click.option('--source', help='Where the images come from: a snapshot .pkl or a dataset .zip', metavar='[PKL|ZIP]', required=True),
        click.option('--num', help='How many images to use  [default: the whole dataset; required for a .pkl]', metavar='INT',
                     type=click.IntRange(min=1)),
        click.option('--seed', help='Seed of the image draws (a .pkl) or of the subset (a .zip)', metavar='INT', type=click.IntRange(min=0),
                     default=0, show_default=True),
        click.option('--split', help='Dataset split (zip sources)', default='train', show_default=True),
        click.option('--modalities', help='Modalities, comma separated  [default: MR_nonrigid_CT,MR_MR_T2 for a zip, '
                     "the snapshot's for a pkl]", default=None),
        click.option('--noise-mode', type=click.Choice(['const', 'random', 'none']), default='random',
                     show_default=True, help='Noise mode (pkl sources)'),
        click.option('--batch', help='Images per batch', metavar='INT', type=click.IntRange(min=1), default=32,
                     show_default=True),
        click.option('--float', 'as_float', is_flag=True, help='Skip the 8-bit quantisation of the images'),
    ]):
        f = opt(f)
    return f


def _stream(source, num, seed, split, modalities, noise_mode, batch, as_float):
    from genlib import spectra
    try:
        return spectra.stream_source_images(source, num, seed, _device(), batch=batch, split=split,
                                            modalities=modalities, noise_mode=noise_mode, as_float=as_float)
    except ValueError as err:       # (SourceError included)
        raise click.ClickException(str(err))


@click.group()
def main():
    """Average power spectra of datasets and generators, per modality: stats, calc, heatmap, slices."""


@main.command()
@_source_options
def stats(source, num, seed, split, modalities, noise_mode, batch, as_float):
    """Print every modality's pixel mean and standard deviation in the form calc takes them."""
    from genlib import spectra
    _n, _size, names, batches = _stream(source, num, seed, split, modalities, noise_mode, batch, as_float)
    mean, std = spectra.channel_moments(batches)
    for name, m, s in zip(names, mean, std):
        print(f'{name}: --mean={m:g} --std={s:g}')
    if len(names) > 1:
        print('--mean=' + ','.join(f'{m:g}' for m in mean) + ' --std=' + ','.join(f'{s:g}' for s in std))


@main.command()
@_source_options
@click.option('--dest', help='Output .npz; several modalities write <stem>-<modality>.npz each',
              metavar='NPZ', required=True)
@click.option('--mean', help='Mean subtracted from the pixels: one value, or one per modality separated by commas',
              metavar='FLOAT[,FLOAT...]', required=True)
@click.option('--std', help='Standard deviation the pixels are divided by: one value, or one per modality', metavar='FLOAT[,FLOAT...]',
              required=True)
@click.option('--beta', help='Beta of the Kaiser window', metavar='FLOAT', type=click.FloatRange(min=0),
              default=8, show_default=True)
@click.option('--interp', help='Zero-padding factor: the spectrum has interp x the image size per side', metavar='INT', type=click.IntRange(min=1),
              default=4, show_default=True)
def calc(source, num, seed, split, modalities, noise_mode, batch, as_float, dest, mean, std, beta, interp):
    """Average the power spectrum of every modality over the source's images and write the .npz files."""
    from genlib import spectra
    count, size, names, batches = _stream(source, num, seed, split, modalities, noise_mode, batch, as_float)
    try:
        mean = spectra.parse_floats(mean, len(names), '--mean')
        std = spectra.parse_floats(std, len(names), '--std')
    except ValueError as err:
        raise click.ClickException(str(err))
    if min(std) <= 0:
        raise click.ClickException(f'--std must be > 0; got {std}')
    spectrum = spectra.average_spectrum(batches, count, size, mean, std, beta=beta, interp=interp)
    for path, plane in zip(spectra.dest_paths(dest, names), spectrum):
        spectra.save_spectrum(path, plane, size)
        print(f'Wrote {path}')


def _pyplot(save):
    import matplotlib
    if save is not None:
        matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    return plt


def _finish(plt, save):
    if save is None:
        plt.show()
        return
    if os.path.dirname(save):
        os.makedirs(os.path.dirname(save), exist_ok=True)
    plt.savefig(save)
    plt.close('all')


_plot_options = [
    click.option('--save', help='Write the figure to this file; without it the figure is shown', metavar='[PNG|PDF|...]'),
    click.option('--dpi', help='Dots per inch of the figure', metavar='FLOAT', type=click.FloatRange(min=1), default=100,
                 show_default=True),
]


@main.command()
@click.argument('npz-file', nargs=1)
@_plot_options[0]
@_plot_options[1]
@click.option('--smooth', help='Gaussian smoothing of the dB map, in image-frequency bins', metavar='FLOAT', type=click.FloatRange(min=0), default=1.25,
              show_default=True)
def heatmap(npz_file, save, smooth, dpi):
    """Plot one spectrum as a filled contour map in dB over the frequency plane."""
    from genlib import spectra
    db, size = spectra.construct_heatmap(npz_file, smooth)
    plt = _pyplot(save)
    half = 0.5 * float(size)                            # the axes run over [-N / 2, N / 2] cycles per image
    axis = np.linspace(-half, half, db.shape[0])
    levels = np.arange(-40.0, 20.0 + 2.5, 5.0)          # -40 .. 20 dB in 5 dB steps
    fig, ax = plt.subplots(figsize=(6, 4.8), dpi=dpi, tight_layout=True)
    filled = ax.contourf(axis, axis, db, levels=levels, cmap='Blues', extend='both')
    ax.contour(axis, axis, db, levels=levels, colors='midnightblue', linewidths=1, linestyles='solid', alpha=0.2,
               extend='both')
    ax.set_aspect('equal')
    quarters = np.linspace(-half, half, 5)
    ax.set(xlim=(-half, half), ylim=(-half, half), xticks=quarters, yticks=quarters)
    fig.colorbar(filled, ax=ax, ticks=levels)
    _finish(plt, save)


@main.command()
@click.argument('npz-files', nargs=-1, required=True)
@_plot_options[0]
@_plot_options[1]
@click.option('--smooth', help='Gaussian smoothing of the dB map, in image-frequency bins', metavar='FLOAT', type=click.FloatRange(min=0), default=0,
              show_default=True)
def slices(npz_files, save, dpi, smooth):
    """Plot the 0 and 45 degree slices of several spectra over one another."""
    from genlib import spectra
    curves = []
    for path in npz_files:
        db, size = spectra.construct_heatmap(path, smooth)
        curves.append((os.path.splitext(os.path.basename(path))[0], db, size))
    size, side = curves[0][2], curves[0][1].shape[0]
    if any(c[2] != size or c[1].shape[0] != side for c in curves):
        raise click.ClickException('All .npz must have the same resolution')
    plt = _pyplot(save)
    plt.figure(figsize=[12, 4.6], dpi=dpi, tight_layout=True)
    centre = side // 2
    upper = np.arange(centre, side)
    yticks = np.linspace(-50, 30, num=9, endpoint=True)
    panels = [('0° slice', size / 2, False, lambda db: db[centre, upper]),
              ('45° slice', size / np.sqrt(2), True, lambda db: db[upper, upper])]
    for k, (title, top, rounded, pick) in enumerate(panels):
        freqs = np.linspace(0, top, num=side // 2 + 1, endpoint=True)
        xticks = np.linspace(freqs[0], freqs[-1], num=9, endpoint=True)
        xticks = np.round(xticks) if rounded else xticks
        plt.subplot(1, 2, k + 1)
        plt.title(title)
        plt.xlim(xticks[0], xticks[-1])
        plt.ylim(yticks[0], yticks[-1])
        plt.xticks(xticks)
        plt.yticks(yticks)
        for label, db, _ in curves:
            plt.plot(freqs, pick(db), label=label)
        plt.grid()
        plt.legend(loc='upper right')
    _finish(plt, save)


if __name__ == '__main__':
    main()   # pylint: disable=no-value-for-parameter
