"""Sampling images from a network snapshot: the pieces the three generation CLIs share (gen_images_mi_multimodal.py,
gen_images_style_mixing.py, gen_video.py -- the reference's src/models/gen_images*.py, SG3/gen_images.py and
SG3/gen_video.py).

Everything up to the generator's float output is the trained network (training/networks_stylegan2.py); the output
stage -- float image -> uint8, laid out as tiles of a canvas -- is one launch of sg2_image_tiles_u8
(torch_utils/ops/image_tiles.py) per batch, and only the finished uint8 canvas crosses to the host.  SG2_GEN_FUSED=0
selects the reference's torch composition (image_tiles_u8_ref) instead: the same bytes from 5-7 launches.

The functions that take plain tensors (truncate, mix_styles, interp_ws, seeds_to_z, the parsers) run on any device.
"""
import os
import re

import numpy as np
import torch

from torch_utils.ops import image_tiles


def fused():
    return os.environ.get('SG2_GEN_FUSED', '1') != '0'


# ---- command-line grammar (the reference's) ----

def parse_range(s):
    """'1,2,5-10' -> [1, 2, 5, 6, 7, 8, 9, 10]; a list is returned as it is.  ValueError on anything else."""
    if isinstance(s, list):
        return s
    out = []
    for part in s.split(','):
        m = re.match(r'^(\d+)-(\d+)$', part)
        if m:
            out.extend(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.append(int(part))
    return out


def parse_tuple(s):
    """'4x2' or '4,2' -> (4, 2); a tuple is returned as it is.  ValueError on anything else."""
    if isinstance(s, tuple):
        return s
    m = re.match(r'^(\d+)[x,](\d+)$', s)
    if not m:
        raise ValueError(f'cannot parse tuple {s}')
    return int(m.group(1)), int(m.group(2))


# ---- snapshot ----

def load_snapshot(network_pkl, device):
    """(G_ema on `device`, eval mode, no gradients; the snapshot's training_set_kwargs or None)."""
    import legacy
    with open(network_pkl, 'rb') as f:
        data = legacy.load_network_pkl(f)
    return data['G_ema'].eval().requires_grad_(False).to(device), data['training_set_kwargs']


def load_generator(network_pkl, device):
    return load_snapshot(network_pkl, device)[0]


def snapshot_modalities(G, training_set_kwargs, modalities=None):
    """Channel names: the given comma-separated list, else the snapshot's training-set modalities, else ch0, ch1, ..."""
    if modalities is not None:
        names = [m for m in (modalities if isinstance(modalities, (list, tuple)) else
                             modalities.replace(' ', '').split(',')) if m]
    elif training_set_kwargs and training_set_kwargs.get('modalities'):
        names = list(training_set_kwargs['modalities'])
    else:
        names = [f'ch{i}' for i in range(G.img_channels)]
    if len(names) != G.img_channels:
        raise ValueError(f'{len(names)} modalities {names} for a generator with {G.img_channels} channels')
    return names


# ---- latents ----

def seeds_to_z(seeds, z_dim):
    """float64 [len(seeds), z_dim]: row i is np.random.RandomState(seeds[i]).randn(z_dim)."""
    return torch.from_numpy(np.stack([np.random.RandomState(int(s)).randn(z_dim) for s in seeds]))


def truncate(w, w_avg, psi):
    """The style-mixing script's truncation: w_avg + (w - w_avg) * psi."""
    return w_avg + (w - w_avg) * psi


def _device_of(G):
    return next(G.parameters()).device


def class_label(G, class_idx, n=1):
    """One-hot [n, c_dim] for a conditional generator, None for an unconditional one."""
    if G.c_dim == 0:
        return None
    if class_idx is None or not 0 <= int(class_idx) < G.c_dim:
        raise ValueError(f'a conditional generator needs a class index in 0..{G.c_dim - 1}; got {class_idx}')
    c = torch.zeros([n, G.c_dim], device=_device_of(G))
    c[:, int(class_idx)] = 1
    return c


def map_seeds(G, seeds, c=None, psi=1, cutoff=None, batch=None):
    """ws [len(seeds), num_ws, w_dim] through G.mapping(z, c, truncation_psi, truncation_cutoff) -- gen_images' form.
    c: None or [1 or len(seeds), c_dim].  batch: seeds per mapping call (None: all at once; 1: the per-seed calls of
    the reference's gen_images loop)."""
    dev = _device_of(G)
    z = seeds_to_z(seeds, G.z_dim).to(dev)
    if c is not None and c.shape[0] == 1:
        c = c.expand(len(seeds), -1)
    step = len(seeds) if not batch else int(batch)
    with torch.no_grad():
        return torch.cat([G.mapping(z[i:i + step], None if c is None else c[i:i + step], truncation_psi=psi,
                                    truncation_cutoff=cutoff) for i in range(0, len(seeds), step)])


def mix_styles(w_row, w_col, styles):
    """[num_ws, w_dim]: a clone of w_row with rows `styles` taken from w_col."""
    w = w_row.clone()
    w[styles] = w_col[styles]
    return w


def interp_ws(ws_key, w_frames, wraps=2, kind='cubic'):
    """Yields one float64 [num_ws, w_dim] per frame, len(ws_key) * w_frames frames: gen_video's periodic interpolation
    through the keyframes ws_key [K, num_ws, w_dim] -- scipy.interpolate.interp1d over the keyframes tiled
    2 * wraps + 1 times at the integers -K * wraps .. K * (wraps + 1) - 1, evaluated at frame / w_frames."""
    import scipy.interpolate
    key = ws_key.detach().cpu().numpy() if isinstance(ws_key, torch.Tensor) else np.asarray(ws_key)
    k = key.shape[0]
    knots = np.arange(-k * wraps, k * (wraps + 1))
    curve = scipy.interpolate.interp1d(knots, np.tile(key, [2 * wraps + 1, 1, 1]), kind=kind, axis=0)
    for frame in range(k * w_frames):
        yield torch.from_numpy(np.asarray(curve(frame / w_frames)))


# ---- synthesis into a canvas ----

def new_canvas(G, grid, cout=1, device=None):
    """A black uint8 canvas [gh * H, gw * W, cout] for grid = (gw, gh) tiles of G's resolution."""
    r = G.img_resolution
    return torch.zeros([grid[1] * r, grid[0] * r, cout], dtype=torch.uint8, device=device or _device_of(G))


def tiles_per_image(G, tiles):
    return G.img_channels if tiles == 'grey' else 1


def synthesize_tiles(G, ws, canvas, first_tile=0, noise_mode='const', force_fp32=False, batch=1, mode='trunc', lo=-1.0,
                     hi=1.0, tiles='grey', grid=None, keep=None):
    """G.synthesis under no_grad over consecutive chunks of `batch` rows of ws [n, num_ws, w_dim], each chunk converted
    by ONE image_tiles_u8 call into `canvas` from tile `first_tile` on (grid = (gw, gh) of the canvas; None: one row).
    canvas may be a list of G.img_channels canvases with tiles='channels': canvas[k] then receives channel k of every
    image -- one call per canvas and chunk.  keep: a list that receives each chunk's float image (device tensors), for
    callers that also want the raw output.  Returns the next free tile."""
    convert = image_tiles.image_tiles_u8 if fused() else image_tiles.image_tiles_u8_ref
    per_channel = isinstance(canvas, (list, tuple))
    if per_channel != (tiles == 'channels'):
        raise ValueError("synthesize_tiles: a list of canvases goes with tiles='channels', and only with it")
    if per_channel and len(canvas) != G.img_channels:
        raise ValueError(f'synthesize_tiles: {len(canvas)} canvases for {G.img_channels} channels')
    batch = max(int(batch), 1)
    ws = ws.to(torch.float32)
    with torch.no_grad():
        for i in range(0, ws.shape[0], batch):
            img = G.synthesis(ws[i:i + batch], noise_mode=noise_mode, force_fp32=force_fp32).contiguous()
            kw = dict(mode=mode, lo=lo, hi=hi, grid=grid, first_tile=first_tile)
            if per_channel:
                for k, cv in enumerate(canvas):
                    convert(img, out=cv, tiles=k, **kw)
            else:
                convert(img, out=canvas, tiles=tiles, **kw)
            if keep is not None:
                keep.append(img)
            first_tile += img.shape[0] * tiles_per_image(G, tiles)
    return first_tile


def cell(canvas, index, grid, res):
    """The [res, res, Cout] view of grid cell `index` of a canvas (tensor or array) with grid = (gw, gh)."""
    r, c = divmod(int(index), grid[0])
    return canvas[r * res:(r + 1) * res, c * res:(c + 1) * res]


def save_grey(path, tile):
    """A [H, W] or [H, W, 1] uint8 array as an 8-bit greyscale PNG."""
    import PIL.Image
    tile = np.asarray(tile)
    PIL.Image.fromarray(np.ascontiguousarray(tile[:, :, 0] if tile.ndim == 3 else tile), 'L').save(path)
