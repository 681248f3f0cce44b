"""Average power spectra of datasets and generators: what avg_spectra.py's commands share (the reference's
SG3/avg_spectra.py, per modality).

The hot path -- whitening, Kaiser window, zero padding to interp times the size, float64 2-D DFT, |.|^2, the sum over
the images -- is torch_utils/ops/power_spectrum.batch_power: one fused call per batch on the GPU (SG2_SPECTRA_FUSED=0
selects the reference's torch composition, which is also the default from 512 x 512 on).  A channel is a modality here
and keeps its own spectrum, where the reference averages an RGB image's channels.

Sources.  A network snapshot (.pkl) is sampled with the reference's per-image draws (RandomState(seed + idx):
randn(1, z_dim), then randint(c_dim) for the label), in batches, noise_mode 'random' as the reference's G(z, c), and
quantised as the reference does: (img * 127.5 + 128).clamp(0, 255) to uint8.  A dataset zip (the project's zip of
per-slice pickles, float32 in [0, 255]) is read through CustomImageFolderDataset and by default clamped and truncated
to uint8 the same way, so that both sides carry the same 8-bit quantisation floor (it lies inside the plotted -50 dB
range); as_float skips the quantisation on both kinds of source.  No network access: sources are local files.
"""
import os

import numpy as np
import torch

from torch_utils.ops import power_spectrum, staged_sum

DEFAULT_MODALITIES = ('MR_nonrigid_CT', 'MR_MR_T2')


class SourceError(ValueError):
    """A source that cannot be streamed as asked (the CLI turns it into a click error)."""


# ---- command-line grammar ----

def parse_floats(text, count, what):
    """'112.7' -> [112.7] * count; '1,2.5' -> [1.0, 2.5], which must be `count` values.  ValueError otherwise."""
    if isinstance(text, (int, float)):
        vals = [float(text)]
    else:
        try:
            vals = [float(p) for p in str(text).split(',')]
        except ValueError:
            raise ValueError(f'{what}: cannot parse {text!r} as a number or a comma-separated list of numbers')
    if len(vals) == 1:
        vals = vals * count
    if len(vals) != count:
        raise ValueError(f'{what}: {len(vals)} values for {count} modalities')
    return vals


def dest_paths(dest, modalities):
    """Where each modality's spectrum goes: `dest` itself for a single channel, <stem>-<modality><ext> otherwise."""
    if len(modalities) == 1:
        return [dest]
    stem, ext = os.path.splitext(dest)
    return [f'{stem}-{m}{ext or ".npz"}' for m in modalities]


def parse_modalities(text):
    if text is None:
        return None
    names = [m for m in (text if isinstance(text, (list, tuple)) else text.replace(' ', '').split(',')) if m]
    return names or None


# ---- sources ----

def latent_draw(seed, z_dim, c_dim):
    """(z float64 [1, z_dim], class index or None): the reference's draws for image `seed`."""
    rnd = np.random.RandomState(int(seed))
    z = rnd.randn(1, z_dim)
    return z, (int(rnd.randint(c_dim)) if c_dim > 0 else None)


def quantise_generated(img):
    """The reference's uint8 image of a generator output in [-1, 1]."""
    return (img * 127.5 + 128).clamp(0, 255).to(torch.uint8)


def quantise_real(img):
    """A dataset slice (float in [0, 255]) clamped and truncated to uint8, as quantise_generated ends."""
    return img.clamp(0, 255).to(torch.uint8)


def _generator_batches(G, num, seed, device, batch, noise_mode, as_float):
    for i in range(0, num, batch):
        idx = range(i, min(i + batch, num))
        draws = [latent_draw(seed + j, G.z_dim, G.c_dim) for j in idx]
        z = torch.from_numpy(np.concatenate([d[0] for d in draws])).to(device=device, dtype=torch.float32)
        c = torch.zeros([len(draws), G.c_dim], device=device)
        for row, (_, k) in enumerate(draws):
            if k is not None:
                c[row, k] = 1
        with torch.no_grad():
            img = G(z, c, noise_mode=noise_mode).float()
        yield (img * 127.5 + 128) if as_float else quantise_generated(img)


def _dataset_batches(ds, device, batch, as_float):
    for i in range(0, len(ds), batch):
        img = torch.from_numpy(np.stack([ds[j][0] for j in range(i, min(i + batch, len(ds)))])).to(device)
        yield img.float() if as_float else quantise_real(img)


def stream_source_images(source, num, seed, device, batch=32, split='train', modalities=None, noise_mode='random',
                         as_float=False):
    """(number of images, image size, modality names, iterator of [b, C, N, N] uint8 (float32 with as_float) batches
    on `device`) of a snapshot .pkl or a dataset zip.  SourceError when the source does not fit the request."""
    ext = source.split('.')[-1].lower()
    batch = max(int(batch), 1)
    names = parse_modalities(modalities)
    if ext == 'pkl':
        if num is None:
            raise SourceError('--num is required when --source points to network pickle')
        from genlib import generate
        G, ts_kwargs = generate.load_snapshot(source, device)
        names = generate.snapshot_modalities(G, ts_kwargs, names)
        return num, G.img_resolution, names, _generator_batches(G, num, seed, device, batch, noise_mode, as_float)
    if ext == 'zip':
        from training.dataset_mi_multimodal import CustomImageFolderDataset
        names = names or list(DEFAULT_MODALITIES)
        try:
            ds = CustomImageFolderDataset(path=source, split=split, modalities=names, dtype='float32', max_size=num,
                                          random_seed=seed, use_labels=False, xflip=False)
        except (IOError, KeyError) as err:
            raise SourceError(f'cannot read {source}: {err!r}')
        if num is not None and num != len(ds):
            raise SourceError(f'--source contains fewer than {num} images')
        return len(ds), ds.resolution, names, _dataset_batches(ds, device, batch, as_float)
    raise SourceError('--source must point to network pickle or dataset zip')


# ---- the two passes ----

def channel_moments(batches):
    """(mean [C], std [C]) float64 numpy over all pixels of each channel: float64 sums of x and x^2 per batch."""
    acc = None
    for img in batches:
        x = img.to(torch.float64)
        m = torch.stack([torch.full([x.shape[1]], float(x.shape[0] * x.shape[2] * x.shape[3]), dtype=torch.float64,
                                    device=x.device),
                         staged_sum.staged_sum(x, [0, 2, 3]), staged_sum.staged_sum(x.square(), [0, 2, 3])])
        acc = m if acc is None else acc + m
    if acc is None:
        raise SourceError('the source holds no images')
    count, total, total_sq = acc.cpu().numpy()
    mean = total / count
    return mean, np.sqrt(total_sq / count - mean * mean)


def average_spectrum(batches, num_images, image_size, mean, std, beta=8, interp=4):
    """float64 numpy [C, S, S]: the summed batch_power of every batch divided by the number of images."""
    window = power_spectrum.kaiser_window(image_size, beta)
    total = None
    for img in batches:
        p = power_spectrum.batch_power(img, mean, std, window, interp)
        total = p if total is None else total + p
    if total is None:
        raise SourceError('the source holds no images')
    return (total / num_images).cpu().numpy()


def save_spectrum(dest, spectrum, image_size):
    """The reference's .npz: `spectrum` float64 [S, S] and `image_size`."""
    spectrum = np.asarray(spectrum)
    assert spectrum.dtype == np.float64 and spectrum.ndim == 2 and spectrum.shape[0] == spectrum.shape[1]
    if os.path.dirname(dest):
        os.makedirs(os.path.dirname(dest), exist_ok=True)
    np.savez(dest, spectrum=spectrum, image_size=image_size)


# ---- display ----

def construct_heatmap(npz_file, smooth):
    """(heatmap in dB [S + 1, S + 1] with the zero frequency at the centre and the first row and column repeated at
    the end, image size) of a saved spectrum; smooth > 0: a Gaussian of sigma = smooth * S / image_size bins."""
    import scipy.ndimage
    with np.load(npz_file) as data:
        spectrum, image_size = data['spectrum'], data['image_size']
    db = np.fft.fftshift(10 * np.log10(spectrum))
    db = np.concatenate([db, db[:1, :]], axis=0)
    db = np.concatenate([db, db[:, :1]], axis=1)
    if smooth > 0:
        db = scipy.ndimage.gaussian_filter(db, sigma=spectrum.shape[0] / image_size * smooth, mode='nearest')
    return db, image_size
