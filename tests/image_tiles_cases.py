"""Inputs and a numpy restatement shared by test_generate_host.py and test_image_tiles_gpu.py.

np_tiles() is the reference's output stage restated in numpy, independently of torch_utils/ops/image_tiles.py:
  'trunc'  gen_video.py layout_grid / gen_images*.py: x * 127.5 + 128 in float32 (two roundings), clamp, truncate;
  'rint'   save_image / save_image_grid: rint((x - lo) * (255 / (hi - lo))).clip(0, 255) on a float32 array;
then the reshape / transpose layout pass of save_image_grid ([gh, gw, C, H, W] -> [gh * H, gw * W, C]) on a full grid,
from which the addressed cells are copied into the canvas.
"""
import numpy as np


def boundary_values():
    """The 768 float32 values f32((k - 128) / 127.5), k = 0..255, each with its two float32 neighbours: where
    x * 127.5 + 128 lands on or next to an integer, so one rounding instead of two changes the byte (95 of the 768)."""
    k = np.arange(256, dtype=np.float64)
    x = ((k - 128) / 127.5).astype(np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-4)), x, np.nextafter(x, np.float32(4))]).astype(np.float32)


def tie_values():
    """For rint with lo, hi = 0, 255 (scale exactly 1): the exact ties k + 0.5, integers, and values below 0 and
    above 255 (ties there too)."""
    k = np.arange(-3, 259, dtype=np.float32)
    return np.concatenate([k + np.float32(0.5), k, np.float32([-1e9, -0.5, -0.25, 255.25, 255.5, 256.5, 1e9])])


def fill(shape, values, seed):
    """An array of `shape` drawing from `values` in a seeded random order (every value used if it fits)."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    reps = -(-n // len(values))
    pool = np.tile(values, reps)
    rng.shuffle(pool)
    return pool[:n].reshape(shape).astype(np.float32)


def np_to_u8(x, mode, lo=-1.0, hi=1.0):
    x = np.asarray(x, dtype=np.float32)
    if mode == 'trunc':
        v = x * np.float32(127.5)
        v = v + np.float32(128)
        assert v.dtype == np.float32
        return np.clip(v, 0, 255).astype(np.uint8)
    v = (x - lo) * (255 / (hi - lo))        # Python scalars against a float32 array: float32 arithmetic
    assert v.dtype == np.float32
    return np.rint(v).clip(0, 255).astype(np.uint8)


def n_tiles(shape, tiles):
    return shape[0] * shape[1] if tiles == 'grey' else shape[0]


def np_tiles(x, canvas, mode, lo, hi, tiles, grid, first_tile):
    """canvas (uint8 [gh * H, gw * W, Cout], modified in place and returned) with the tiles of x [N, C, H, W] laid from
    cell first_tile on."""
    n, c, h, w = x.shape
    u8 = np_to_u8(x, mode, lo, hi)
    if tiles == 'grey':
        u8 = u8.reshape(n * c, 1, h, w)
    elif tiles != 'hwc':
        u8 = u8[:, tiles:tiles + 1]
    t, cout = u8.shape[:2]
    gw, gh = grid
    full = np.zeros([gh * gw, cout, h, w], np.uint8)
    full[first_tile:first_tile + t] = u8
    full = full.reshape(gh, gw, cout, h, w).transpose(0, 3, 1, 4, 2).reshape(gh * h, gw * w, cout)
    mask = np.zeros([gh * gw, cout, h, w], bool)
    mask[first_tile:first_tile + t] = True
    mask = mask.reshape(gh, gw, cout, h, w).transpose(0, 3, 1, 4, 2).reshape(gh * h, gw * w, cout)
    canvas[mask] = full[mask]
    return canvas, mask
