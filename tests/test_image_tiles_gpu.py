"""sg2_image_tiles_u8 (csrc/imgout.hip) through torch_utils.ops.image_tiles on the GPU.

Bitwise against image_tiles_u8_ref -- the reference's torch composition -- on the same device, and for float32 inputs
also against the numpy restatement (image_tiles_cases.np_tiles): every tile form, mode, dtype, grid and first tile,
inputs and canvases at aligned and misaligned addresses, on values where one rounding instead of two, or a rewritten
rint formula, changes bytes.  The canvas is pre-filled with 0xA5: every byte outside the addressed tiles must still be
0xA5.  Shapes: the widths 4, 7, 12, 20 take the 4-byte-store path (with W = 7 and Cout = 3 nothing in a row is aligned),
W = 32 the 16-byte path (and the 4-byte one once either base is misaligned); 256^2 covers many workgroups."""
import numpy as np
import pytest
import torch

import image_tiles_cases as tc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FILL = 0xA5
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}


def _shifted(x):
    """x's values in a buffer that starts one element later than an allocation does."""
    buf = torch.empty([x.numel() + 1], dtype=x.dtype, device=x.device)
    out = buf[1:].view(x.shape)
    out.copy_(x)
    assert out.is_contiguous() and out.data_ptr() == buf.data_ptr() + x.element_size()
    return out


def _canvas(shape, odd):
    """A 0xA5 canvas; odd: a contiguous view that starts 1 byte into its storage."""
    n = int(np.prod(shape))
    store = torch.full([n + 1], FILL, dtype=torch.uint8, device=DEV)
    cv = store[1 if odd else 0:][:n].view(shape)
    assert cv.is_contiguous() and cv.data_ptr() % 2 == (1 if odd else 0)
    return cv


def _forms(c):
    return ['grey'] + list(range(c)) + (['hwc'] if c in (1, 3) else [])


def _grids(t):
    out = []
    for first in (0, 2):
        out.append(((t + first, 1), first))
        out.append(((3, -(-(t + first + 1) // 3)), first))      # at least one spare cell
    return out


def _check(x_np, dtype, mode, lo, hi, tiles, grid, first, shift_in, odd_out, against_numpy):
    from torch_utils.ops import image_tiles
    n, c, h, w = x_np.shape
    x = torch.from_numpy(x_np).to(DEV).to(dtype)
    if shift_in:
        x = _shifted(x)
    cout = c if tiles == 'hwc' else 1
    shape = [grid[1] * h, grid[0] * w, cout]
    got = image_tiles.image_tiles_u8(x, out=_canvas(shape, odd_out), mode=mode, lo=lo, hi=hi, tiles=tiles, grid=grid,
                                     first_tile=first)
    want = image_tiles.image_tiles_u8_ref(x, out=_canvas(shape, False), mode=mode, lo=lo, hi=hi, tiles=tiles, grid=grid,
                                          first_tile=first)
    what = (x_np.shape, str(dtype), mode, lo, hi, tiles, grid, first, shift_in, odd_out)
    got_np = got.cpu().numpy()
    _, mask = tc.np_tiles(np.zeros_like(x_np), np.zeros(shape, np.uint8), 'trunc', -1, 1, tiles, grid, first)
    assert (got_np[~mask] == FILL).all(), ('bytes outside the tiles were written', what)
    bad = int((got != want).sum())
    assert bad == 0, (f'{bad} bytes differ from the torch composition', what)
    assert (got_np[mask] == FILL).mean() < 0.5, ('the inputs cannot tell a written tile from the fill', what)
    if against_numpy:
        ref_np, _ = tc.np_tiles(x_np, np.full(shape, FILL, np.uint8), mode, lo, hi, tiles, grid, first)
        assert np.array_equal(got_np, ref_np), ('differs from the numpy restatement', what)


def _kinds(mode):
    kinds = [('uniform', -1.0, 1.0), ('boundary', -1.0, 1.0)]
    if mode == 'rint':
        kinds += [('ties', 0.0, 255.0), ('uniform', -0.3, 1.7)]
    return kinds


def _values(kind, shape, seed):
    if kind == 'uniform':
        return np.random.RandomState(seed).uniform(-1.3, 1.3, shape).astype(np.float32)
    return tc.fill(shape, tc.boundary_values() if kind == 'boundary' else tc.tie_values(), seed)


@pytest.mark.parametrize('mode', ['trunc', 'rint'])
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('h,w', [(4, 4), (12, 12), (5, 7), (20, 20), (6, 32)])
def test_bitwise_against_the_composition(h, w, dtype, mode):
    calls = 0
    for c in (1, 2, 3):
        for n in (1, 5):
            for k, (kind, lo, hi) in enumerate(_kinds(mode)):
                x_np = _values(kind, (n, c, h, w), seed=100 * c + 10 * n + k)
                for tiles in _forms(c):
                    t = tc.n_tiles(x_np.shape, tiles)
                    for j, (grid, first) in enumerate(_grids(t)):
                        # every grid at aligned addresses; the misaligned input and canvas take turns over the grids
                        variants = [(False, False), ((j % 2) == 0, (j % 2) == 1)]
                        if kind == 'boundary':
                            variants.append((True, True))
                        for shift_in, odd_out in variants:
                            _check(x_np, DTYPES[dtype], mode, lo, hi, tiles, grid, first, shift_in, odd_out,
                                   against_numpy=dtype == 'f32')
                            calls += 1
    print(f'{calls} kernel calls compared at {h} x {w}, {dtype}, {mode}')


def test_grid_none_and_new_canvas():
    from torch_utils.ops import image_tiles
    x = torch.from_numpy(_values('uniform', (3, 2, 8, 32), 1)).to(DEV)
    for tiles, t, cout in (('grey', 6, 1), (1, 3, 1)):
        got = image_tiles.image_tiles_u8(x, tiles=tiles)
        assert got.shape == (8, t * 32, cout) and got.dtype == torch.uint8
        assert torch.equal(got, image_tiles.image_tiles_u8_ref(x, tiles=tiles))
    got = image_tiles.image_tiles_u8(x, tiles='grey', grid=(4, 2))       # two spare cells stay black
    assert torch.equal(got, image_tiles.image_tiles_u8_ref(x, tiles='grey', grid=(4, 2)))
    assert int(got[8:, 64:].max()) == 0


@pytest.mark.parametrize('mode', ['trunc', 'rint'])
def test_larger_case(mode):
    """256^2, C = 2, N = 8, grey tiles in a 4 x 4 grid: the index arithmetic over 1024 rows of 1024 bytes and the
    16-byte path over 256 workgroups."""
    x_np = _values('uniform', (8, 2, 256, 256), 7)
    x_np.reshape(-1)[:768] = tc.boundary_values()
    _check(x_np, torch.float32, mode, -1.0, 1.0, 'grey', (4, 4), 0, False, False, against_numpy=True)


@pytest.mark.parametrize('mode', ['trunc', 'rint'])
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_nan_and_infinities(dtype, mode):
    """This build's definition: NaN -> 0, +inf -> 255, -inf -> 0 (the torch and numpy casts are undefined)."""
    from torch_utils.ops import image_tiles
    row = torch.tensor([float('nan'), float('inf'), float('-inf'), 0.0, 1.0, -1.0, 3e38, -3e38], dtype=torch.float32)
    want_row = [0, 255, 0, 128 if mode == 'trunc' else 128, 255, 0, 255, 0]
    # trunc: 0 * 127.5 + 128 = 128; rint: (0 + 1) * 127.5 = 127.5 -> 128 (half to even)
    for w in (8, 32):       # the 4-byte and the 16-byte path
        x = row.repeat(w // 8).reshape(1, 1, 1, w).repeat(2, 1, 3, 1).to(DEV).to(DTYPES[dtype])
        got = image_tiles.image_tiles_u8(x, mode=mode, tiles='grey')
        assert got.shape == (3, 2 * w, 1)
        assert got.cpu().flatten().tolist() == want_row * (w // 8) * 2 * 3, (w, dtype, mode)
    x3 = row.reshape(1, 1, 1, 8).repeat(1, 3, 2, 1).to(DEV).to(DTYPES[dtype])       # hwc, Cout = 3
    got = image_tiles.image_tiles_u8(x3, mode=mode, tiles='hwc').cpu()
    assert got.shape == (2, 8, 3)
    assert got[0, :, 1].tolist() == want_row and torch.equal(got[:, :, 0], got[:, :, 2])


def test_argument_errors():
    from torch_utils.ops import image_tiles
    f = image_tiles.image_tiles_u8
    x = torch.zeros(2, 2, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        f(x.cpu(), tiles='grey')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        f(x, tiles='grey', out=torch.zeros(4, 16, 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='contiguous'):
        f(x.permute(0, 1, 3, 2), tiles='grey')
    with pytest.raises(RuntimeError, match='float32'):
        f(x.to(torch.int32), tiles='grey')
    with pytest.raises(RuntimeError, match='hwc'):
        f(x, tiles='hwc')
    with pytest.raises(RuntimeError, match='channel'):
        f(x, tiles=2)
    with pytest.raises(RuntimeError, match='channel'):
        f(x, tiles=-1)
    with pytest.raises(RuntimeError, match='grid'):
        f(x, tiles='grey', grid=(3, 1))
    with pytest.raises(RuntimeError, match='grid'):
        f(x, tiles=0, grid=(2, 2), first_tile=3, out=torch.zeros(8, 8, 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='first_tile'):
        f(x, tiles=0, grid=(2, 2), first_tile=1)
    with pytest.raises(RuntimeError, match='out'):
        f(x, tiles='grey', out=torch.zeros(4, 12, 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='out'):
        f(x, tiles='grey', out=torch.zeros(4, 16, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='out'):
        f(x, tiles='grey', out=torch.zeros(4, 16, 1, dtype=torch.int8, device=DEV))
    with pytest.raises(RuntimeError, match='contiguous'):
        f(x, tiles='grey', out=torch.zeros(4, 32, 1, dtype=torch.uint8, device=DEV)[:, ::2])
    with pytest.raises(RuntimeError, match='lo and hi'):
        f(x, tiles='grey', mode='rint', lo=0.5, hi=0.5)
    with pytest.raises(RuntimeError, match='mode'):
        f(x, tiles='grey', mode='floor')
    torch.cuda.synchronize()
