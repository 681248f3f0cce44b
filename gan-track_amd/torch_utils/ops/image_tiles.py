"""The generator's output stage: images -> uint8 tiles of an HWC canvas in one launch (HIP kernel sg2_image_tiles_u8,
csrc/imgout.hip).

image_tiles_u8(img, out, mode, lo, hi, tiles, grid, first_tile)   img [N, C, H, W] f32 / f16 / bf16 on a ROCm device
                                                                  -> uint8 canvas [gh * H, gw * W, Cout]
image_tiles_u8_ref(...)                                           the reference's composition in torch, any device

mode 'trunc' is the generator-side convention of the reference -- (x * 127.5 + 128).clamp(0, 255).to(uint8) of
gen_images*.py, gen_video.py layout_grid and metrics/metric_utils.py; mode 'rint' is its save_image / save_image_grid
convention -- rint((x - lo) * (255 / (hi - lo))).clip(0, 255) in float32 numpy.  The kernel is bitwise either one
(include/sg2hip.h has the arithmetic); NaN -> 0, +inf -> 255, -inf -> 0 is this build's definition, where the torch
and numpy casts are undefined (the `_ref` function does NOT define them).

tiles:  an int k   tile n is channel k of image n (a per-modality image),                     Cout = 1
        'grey'     tile n * C + c is channel c of image n (training_loop's to_grey_tiles),    Cout = 1
        'hwc'      tile n is image n, channels interleaved (C must be 1 or 3),                Cout = C
Tile t lands in grid cell first_tile + t of grid = (gw, gh): row (first_tile + t) // gw, column (first_tile + t) % gw.
Canvas bytes outside the addressed tiles are left as they are.  ROCm tensors only for the kernel (no CPU fallback);
not differentiable.
"""
import torch

import sg2hip as _hip

TILES_HWC, TILES_GREY = -1, -2      # SG2_TILES_HWC, SG2_TILES_GREY
MODES = {'trunc': 0, 'rint': 1}     # SG2_U8_TRUNC, SG2_U8_RINT


def _plan(img, out, mode, lo, hi, tiles, grid, first_tile, what):
    """Validated (tiles code, Cout, T, gw, gh, first_tile); every error names its argument."""
    if not isinstance(img, torch.Tensor) or img.ndim != 4 or img.dtype not in _hip._DTYPES:
        raise RuntimeError(f'{what}: img must be a float32, float16 or bfloat16 tensor [N, C, H, W]; got '
                           f'{getattr(img, "dtype", type(img).__name__)} {list(getattr(img, "shape", []))}')
    if not img.is_contiguous():
        raise RuntimeError(f'{what}: img must be contiguous')
    n, c, h, w = img.shape
    if min(n, c, h, w) < 1:
        raise RuntimeError(f'{what}: img must not be empty; got {list(img.shape)}')
    if mode not in MODES:
        raise RuntimeError(f"{what}: mode must be 'trunc' or 'rint'; got {mode!r}")
    if mode == 'rint':
        lo, hi = float(lo), float(hi)
        if not (lo == lo and hi == hi and abs(lo) != float('inf') and abs(hi) != float('inf') and hi != lo):
            raise RuntimeError(f'{what}: lo and hi must be finite and differ; got lo={lo}, hi={hi}')
    if tiles == 'hwc':
        if c not in (1, 3):
            raise RuntimeError(f"{what}: tiles='hwc' needs C = 1 or C = 3; img has C = {c}")
        code, cout, t = TILES_HWC, c, n
    elif tiles == 'grey':
        code, cout, t = TILES_GREY, 1, n * c
    elif isinstance(tiles, int) and not isinstance(tiles, bool):
        if not 0 <= tiles < c:
            raise RuntimeError(f'{what}: tiles={tiles} is not a channel of img (C = {c})')
        code, cout, t = tiles, 1, n
    else:
        raise RuntimeError(f"{what}: tiles must be 'hwc', 'grey' or a channel number; got {tiles!r}")
    gw, gh = (t, 1) if grid is None else (int(grid[0]), int(grid[1]))
    first_tile = int(first_tile)
    if gw < 1 or gh < 1:
        raise RuntimeError(f'{what}: grid must be (gw, gh) with both at least 1; got {grid}')
    if first_tile < 0 or first_tile + t > gw * gh:
        raise RuntimeError(f'{what}: first_tile={first_tile} plus {t} tiles does not fit grid {gw} x {gh}')
    if out is None:
        if first_tile != 0:
            raise RuntimeError(f'{what}: first_tile must be 0 when out is None (a new canvas)')
    else:
        want = [gh * h, gw * w, cout]
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or list(out.shape) != want:
            raise RuntimeError(f'{what}: out must be a uint8 canvas {want}; got '
                               f'{getattr(out, "dtype", type(out).__name__)} {list(getattr(out, "shape", []))}')
        if not out.is_contiguous():
            raise RuntimeError(f'{what}: out must be contiguous')
        if out.device != img.device:
            raise RuntimeError(f'{what}: out is on {out.device}, img on {img.device}')
    return code, cout, t, gw, gh, first_tile


def image_tiles_u8(img, out=None, mode='trunc', lo=-1.0, hi=1.0, tiles='hwc', grid=None, first_tile=0):
    """One launch of sg2_image_tiles_u8.  out=None allocates a zero (black) canvas (first_tile must then be 0);
    grid=None means (T, 1), one row of tiles.  Returns the canvas."""
    _hip.require_device(img, out)
    code, cout, t, gw, gh, first_tile = _plan(img, out, mode, lo, hi, tiles, grid, first_tile, 'image_tiles_u8')
    n, c, h, w = img.shape
    img = img.detach()
    with torch.cuda.device(img.device):
        if out is None:
            out = torch.zeros([gh * h, gw * w, cout], dtype=torch.uint8, device=img.device)
        _hip.check(_hip.lib().sg2_image_tiles_u8(_hip.ptr(out), _hip.ptr(img), _hip.dtype_code(img), n, c, h, w, code,
                                                 MODES[mode], float(lo), float(hi), gw, gh, first_tile,
                                                 _hip.stream_ptr(img.device)), 'sg2_image_tiles_u8')
    return out


# ---- the reference's composition (any device) ----

def to_uint8_ref(img, mode='trunc', lo=-1.0, hi=1.0):
    """The value conversion alone, elementwise, as the reference composes it."""
    x = img.detach().float()
    if mode == 'trunc':
        return (x * 127.5 + 128).clamp(0, 255).to(torch.uint8)
    # numpy: float32 array against Python scalars -- lo and the double quotient 255 / (hi - lo) each become float32
    x = (x - float(lo)) * (255 / (float(hi) - float(lo)))
    return x.round().clamp(0, 255).to(torch.uint8)      # round: half to even, as np.rint


def image_tiles_u8_ref(img, out=None, mode='trunc', lo=-1.0, hi=1.0, tiles='hwc', grid=None, first_tile=0):
    """image_tiles_u8 as a torch composition: the value passes of the reference (4-5 elementwise kernels), then its
    reshape / permute layout pass written into the canvas (up to three copies: a partial first grid row, the whole rows,
    a partial last row).  NaN and infinities are whatever the device's float -> uint8 cast makes of them."""
    code, cout, t, gw, gh, first_tile = _plan(img, out, mode, lo, hi, tiles, grid, first_tile, 'image_tiles_u8_ref')
    n, c, h, w = img.shape
    u8 = to_uint8_ref(img, mode, lo, hi)
    if code == TILES_HWC:
        til = u8.permute(0, 2, 3, 1)                    # [T, H, W, Cout]
    elif code == TILES_GREY:
        til = u8.reshape(n * c, h, w, 1)
    else:
        til = u8[:, code].unsqueeze(-1)
    if out is None:
        out = torch.zeros([gh * h, gw * w, cout], dtype=torch.uint8, device=img.device)
    cells = out.view(gh, h, gw, w, cout)                # [row, y, column, x, channel]
    done = 0
    while done < t:                                     # runs of cells: within one grid row, or whole rows
        cell = first_tile + done
        r, col = divmod(cell, gw)
        if col == 0 and t - done >= gw:
            rows = (t - done) // gw
            cells[r:r + rows].copy_(til[done:done + rows * gw].reshape(rows, gw, h, w, cout).permute(0, 2, 1, 3, 4))
            done += rows * gw
        else:
            k = min(gw - col, t - done)
            cells[r, :, col:col + k].copy_(til[done:done + k].permute(1, 0, 2, 3))
            done += k
    return out
