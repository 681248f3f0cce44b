"""The ADA geometric kernels one at a time: every element, every band, every extent.

The geometric stage (training/augment_mi.py:181-184, :265-281) chains sg2_reflect_pad_dyn, the limited FIR passes of
sg2_upfirdn2d_lim and sg2_affine_grid_sample_fwd / _bwd (dyn_hw) on a dynamically sized image inside static buffers.
Each kernel stores the logical image plus a band and nothing else; here each is run alone, on buffers the test owns,
against CPU float64 of the same operands (tests/elementwise.py), and its result is held in three regions
(EW.assert_regions): the computed region within the elementwise bound (bitwise for the pad, a copy), the zero band
exactly 0.0, and the rest still NaN -- untouched.  No element is exempt.

Poison: this module has no autouse fixture; every test poisons torch.empty / empty_like of reflect_pad, upfirdn2d
and grid_sample_gradfix in its own body (poison.poisoned_empties), so every output buffer of the op under test
starts as NaN.  Inputs fed "as their producer leaves them" hold values inside the region the producer guarantees
(tests/ada_regions.py, pinned without a GPU by test_ada_geom_host.py) and NaN outside it.

Out of scope: the kernel variants chosen by SG2_U1D_VRUN, SG2_U1D_HLDS and SG2_U1D_HTW are read once per process;
only the defaults (upfirdn_1d_vrun<..., 4>, upfirdn_1d_hlds<..., 128>) run here, beside the upfirdn_1d<..., 0, 0>
fallback and upfirdn_generic.  inf / NaN sampling coordinates and coordinates beyond the int range are not
covered: the float-to-int conversion there is not defined by the source.

Worst error / bound ratios measured on an MI355X (each assertion prints its own; all f32 unless marked):
    reflect_pad forward            bitwise (0)          reflect_pad adjoint             0.33
    upfirdn2d_lim up-2 horizontal  0.13 (hlds, 128)     upfirdn2d_lim up-2 vertical     0.11 (vrun, 4)
    upfirdn2d_lim down-2 horiz.    0.18                 upfirdn2d_lim down-2 vertical   0.17
    upfirdn_1d fallback, 5 taps    0.26 / 0.22 (up 2)   upfirdn_generic 4 x 4, up 2     0.09
    upsample2d_limited             forward 0.08, first backward 0.09, second backward 0.07
    grid_sample forward, grid      f32 0.06, f16 0.86, bf16 0.95 (a 16-bit output's own rounding is the bound there)
    grid_sample forward, affine    f32 0.05, f16 0.84, bf16 0.96;  dyn_hw 0.07 (grid) / 0.05 (affine)
    second trips (1450 x 1450)     forward 0.10, scatter 0.19, gather 0.19
    gradient with dyn_hw           scatter 0.003, gather 0.002 (the gather test's tol, far above f32 rounding)
    double backward with dyn_hw    0.06
    chain pairs                    FIR 0.19, sampler 0.04, pad adjoint 0.36
    The forward bound's CPU f32 replay of corners_g and the forward kernel against float64 stood at 0.10
    (20 x 24, 40 x 36, 524 x 530, centre-snapped points included).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import ada_regions as R
import elementwise as EW
import poison

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
NAN = float('nan')
POISONED = ('torch_utils.ops.reflect_pad', 'torch_utils.ops.upfirdn2d', 'torch_utils.ops.grid_sample_gradfix')
GS_KW = dict(mode='bilinear', padding_mode='zeros', align_corners=False)

def _poison(monkeypatch):
    return poison.poisoned_empties(monkeypatch, POISONED)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(what, ratio, dtype=torch.float32):
    print(f'elementwise {what} {str(dtype)[6:]}: worst error / bound {ratio:.3g}')
    return ratio


def _regions(got, computed, band, what, **kw):
    return _report(what, EW.assert_regions(got, computed, band, what, **kw), kw.get('out_dtype', torch.float32))


def _elementwise(got, ref, slack, dtype, what):
    return _report(what, EW.assert_elementwise(got, ref, slack, dtype, what), dtype)


def _embed(inner, shape, fill=NAN):
    """`inner` at the origin of a buffer of `shape`, `fill` elsewhere."""
    out = torch.full(shape, fill, dtype=inner.dtype)
    out[:, :, :inner.shape[2], :inner.shape[3]] = inner
    return out


# ------------------------------------------------------------------ 1. reflect_pad_dyn
def _margin_sets(H, W):
    return [(0, 0, 0, 0), (1, 1, 1, 1), (W - 1, H - 1, W - 1, H - 1), (0, H - 1, W - 1, 0),
            (min(3, W - 1), 0, 0, min(11, H - 1)),          # (3, 0, 0, 11), held to the contract margin <= size - 1
            (2 * W // 3, 2 * H // 3, W // 2, 3 * H // 4)]   # both reflections of an interior row hit one source row


PAD_CASES = [(s, m) for s in [(2, 2, 40, 48), (1, 1, 5, 7)] for m in _margin_sets(s[2], s[3])]
_pad_id = lambda v: 'x'.join(map(str, v))     # noqa: E731


for (_n, _c, _H, _W), (_mx0, _my0, _mx1, _my1) in PAD_CASES[5::6]:
    assert any(_my0 >= iy >= _H - 1 - _my1 for iy in range(1, _H - 1))
    assert any(_mx0 >= ix >= _W - 1 - _mx1 for ix in range(1, _W - 1))


@pytest.mark.parametrize('shape,m', PAD_CASES, ids=[f'{_pad_id(s)}-m{_pad_id(m)}' for s, m in PAD_CASES])
def test_reflect_pad_forward(shape, m, monkeypatch):
    """[:Hd, :Wd] bitwise F.pad(reflect) (a copy); zeros out to +64 (reflect_pad_kernel); NaN beyond."""
    from torch_utils.ops import reflect_pad
    _poison(monkeypatch)
    N, C, H, W = shape
    mx0, my0, mx1, my1 = m
    x = torch.randn(shape, generator=_gen(11))
    y = reflect_pad.reflect_pad_dyn(x.to(DEV), _i32(*m))
    assert tuple(y.shape) == (N, C, 3 * H - 2, 3 * W - 2)
    ref = F.pad(x.double(), (mx0, mx1, my0, my1), mode='reflect')
    Hd, Wd = ref.shape[2:]
    _regions(y, (Hd, Wd), (Hd + R.PAD_BAND, Wd + R.PAD_BAND), f'reflect_pad fwd {shape} {m}', ref=ref, exact=True)


@pytest.mark.parametrize('shape,m', PAD_CASES, ids=[f'{_pad_id(s)}-m{_pad_id(m)}' for s, m in PAD_CASES])
def test_reflect_pad_adjoint(shape, m, monkeypatch):
    """reflect_pad._Adj on a gradient buffer that is NaN outside the padded image: every source pixel within 8 2^-24
    of the same adjoint of |gy| (at most 3 x 3 terms) around the float64 autograd gradient of F.pad(reflect)."""
    from torch_utils.ops import reflect_pad
    _poison(monkeypatch)
    N, C, H, W = shape
    Hd, Wd = H + m[1] + m[3], W + m[0] + m[2]
    gyc = torch.randn(N, C, Hd, Wd, generator=_gen(12))
    gy = _embed(gyc, (N, C, 3 * H - 2, 3 * W - 2))
    gx = reflect_pad._Adj.apply(gy.to(DEV), _i32(*m), H, W)
    ref, slack = EW.reflect_pad_adjoint_ref(gyc.double(), (H, W), m)
    _elementwise(gx, ref, slack, torch.float32, f'reflect_pad adjoint {shape} {m}')


def test_reflect_pad_autograd_chain(monkeypatch):
    """pad -> adjoint -> pad through autograd: the gradient of the pad and the gradient of that gradient."""
    from torch_utils.ops import reflect_pad
    _poison(monkeypatch)
    shape, m = (2, 2, 40, 48), (32, 26, 24, 30)
    N, C, H, W = shape
    Hd, Wd = H + m[1] + m[3], W + m[0] + m[2]
    g = _gen(13)
    x, gyc, v = torch.randn(shape, generator=g), torch.randn(N, C, Hd, Wd, generator=g), torch.randn(shape, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    gyd = _embed(gyc, (N, C, 3 * H - 2, 3 * W - 2)).to(DEV).requires_grad_(True)
    y = reflect_pad.reflect_pad_dyn(xd, _i32(*m))
    gx, = torch.autograd.grad(y, [xd], gyd, create_graph=True)
    ref, slack = EW.reflect_pad_adjoint_ref(gyc.double(), (H, W), m)
    _elementwise(gx, ref, slack, torch.float32, 'reflect_pad chain: first order')
    ggy, = torch.autograd.grad(gx, [gyd], v.to(DEV))
    ref2 = F.pad(v.double(), (m[0], m[2], m[1], m[3]), mode='reflect')
    _regions(ggy, (Hd, Wd), (Hd + R.PAD_BAND, Wd + R.PAD_BAND), 'reflect_pad chain: second order', ref=ref2, exact=True)


# ------------------------------------------------------------------ 2. limited FIR passes
@functools.lru_cache(None)
def _sym6():
    from training.augment_mi import wavelets
    from torch_utils.ops import upfirdn2d as upf
    f = upf.setup_filter(wavelets['sym6'])
    assert f.shape == (12,)
    return f


@functools.lru_cache(None)
def _fir_route(route):
    """-> (x f32 CPU, f2, kernel arguments (upx, upy, downx, downy, px0, px1, py0, py1, flip, gain))."""
    from torch_utils.ops import upfirdn2d as upf
    f = _sym6()
    up_in, down_in = (2, 2, 70, 150), (2, 2, 140, 300)
    # the parameters _SepLimited.backward derives for the up-2 passes of upsample2d_limited (padding (6, 5), gain 4)
    aup, adown, ap, aflip = upf.adjoint_params(f, up_in[2:], down_in[2:], [2, 2], [1, 1], [6, 5, 6, 5], False)
    assert (aup, adown, ap, aflip) == ([1, 1], [2, 2], [5, 5, 5, 5], True)
    f5 = torch.tensor([0.1, 0.3, -0.2, 0.5, 0.3])
    f44 = torch.randn(4, 4, generator=_gen(20)) / 4
    shape, f2, args = {
        # the production routes: upfirdn_1d_hlds<T, 2, 1, 6, 128>, upfirdn_1d_vrun<T, 2, 1, 6, 4> and the down-2 forms
        'up_h': (up_in, f[None], (2, 1, 1, 1, 6, 5, 0, 0, False, 1.0)),
        'up_v': (up_in, f[:, None], (1, 2, 1, 1, 0, 0, 6, 5, False, 4.0)),
        'down_h': (down_in, f[None], (aup[0], 1, adown[0], 1, ap[0], ap[1], 0, 0, aflip, 1.0)),
        'down_v': (down_in, f[:, None], (1, aup[1], 1, adown[1], 0, 0, ap[2], ap[3], aflip, 4.0)),
        # the generic routes: upfirdn_1d<T, HORIZ, KT, 0, 0> (run-time factors) and upfirdn_generic
        'fallback_h5': (up_in, f5[None], (1, 1, 1, 1, 2, 2, 0, 0, False, 1.0)),
        'fallback_v5_up2': (up_in, f5[:, None], (1, 2, 1, 1, 0, 0, 3, 2, True, 2.0)),
        'generic_4x4_up2': (up_in, f44, (2, 2, 1, 1, 2, 1, 2, 1, False, 4.0)),
    }[route]
    x = torch.randn(shape, generator=_gen(21))
    return x, f2.contiguous(), args


@functools.lru_cache(None)
def _fir_case(route):
    """The route's input on the device and its full-buffer float64 reference, computed once for all extents."""
    x, f2, a = _fir_route(route)
    ref, slack = EW.fir_ref(x, f2, torch.float32, up=(a[0], a[1]), down=(a[2], a[3]), padding=list(a[4:8]),
                            flip_filter=a[8], gain=a[9])
    return x.to(DEV), f2.to(DEV), a, ref, slack


def _extents(OH, OW):
    return {'zero': (0, 0), 'one': (1, 1), 'odd': (37, 131),
            'x128': (50, 100),                 # lx + 32 = 132 straddles a 128-column tile of the horizontal pass
            'x256': (61, 230),                 # lx + 32 = 262 straddles a 256-column tile of the vertical pass
            'tail4': (38, 53),                 # ly and ly + 32 = 70 are no multiples of 4: the tail of a run of 4
            'full': (OH, OW), 'over': (OH + 40, OW + 100)}


FIR_CASES = ([(r, e) for r in ('up_h', 'up_v', 'down_h', 'down_v') for e in _extents(0, 0)] +
             [(r, e) for r in ('fallback_h5', 'fallback_v5_up2', 'generic_4x4_up2') for e in ('odd', 'x128', 'over')])


@pytest.mark.parametrize('route,extent', FIR_CASES, ids=[f'{r}-{e}' for r, e in FIR_CASES])
def test_fir_pass_limited(route, extent, monkeypatch):
    """One sg2_upfirdn2d_lim pass: [:ly, :lx] within fir_ref of the full-buffer float64 FIR, zeros out to +32
    (kZeroBand), NaN beyond; an extent past the output clamps to it."""
    from torch_utils.ops import upfirdn2d as upf
    _poison(monkeypatch)
    x, f2, a, ref, slack = _fir_case(route)
    ly, lx = _extents(*ref.shape[2:])[extent]
    y = upf._raw_lim(x, f2, *a, _i32(ly, lx))
    assert y.shape == ref.shape
    _regions(y, (ly, lx), (ly + R.FIR_BAND, lx + R.FIR_BAND), f'upfirdn2d_lim {route} lim ({ly}, {lx})',
             ref=ref, slack=slack)


def test_upsample2d_limited_composite(monkeypatch):
    """upsample2d_limited with four extents through autograd: forward, first backward (the adjoint passes with
    lims[2], lims[3]) and second backward (the forward passes again), each against the unlimited two-pass float64
    FIR inside the last pass's extent, with the slack composed from the two passes (EW.fir_chain_ref)."""
    from torch_utils.ops import upfirdn2d as upf
    _poison(monkeypatch)
    f = _sym6()
    g = _gen(22)
    shape = (2, 2, 70, 150)
    lims = R.lims(20, 50)                       # a 20 x 50 logical image: no extent clamps
    assert lims == [(52, 132), (72, 132), (136, 82), (52, 82)]
    fwd = [dict(f=f[None], up=(2, 1), padding=[6, 5, 0, 0]), dict(f=f[:, None], up=(1, 2), padding=[0, 0, 6, 5], gain=4)]
    bwd = [dict(f=f[None], down=(2, 1), padding=[5, 5, 0, 0], flip_filter=True),
           dict(f=f[:, None], down=(1, 2), padding=[0, 0, 5, 5], flip_filter=True, gain=4)]
    x, v = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    dy = torch.randn(2, 2, 140, 300, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    dyd = dy.to(DEV).requires_grad_(True)
    y = upf.upsample2d_limited(xd, f.to(DEV), [_i32(*l) for l in lims], up=2)
    ref, slack = EW.fir_chain_ref(x, fwd)
    _regions(y, lims[1], (lims[1][0] + 32, lims[1][1] + 32), 'upsample2d_limited forward', ref=ref, slack=slack)
    gx, = torch.autograd.grad(y, [xd], dyd, create_graph=True)
    ref, slack = EW.fir_chain_ref(dy, bwd)
    # the explicit adjoint passes are the adjoint: the float64 autograd gradient of the forward reference
    xr = x.double().requires_grad_(True)
    auto, = torch.autograd.grad(EW.fir_chain_ref(xr, fwd)[0], [xr], dy.double())
    assert float((auto - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    _regions(gx, lims[3], (lims[3][0] + 32, lims[3][1] + 32), 'upsample2d_limited first backward', ref=ref, slack=slack)
    ggy, = torch.autograd.grad(gx, [dyd], v.to(DEV))
    ref, slack = EW.fir_chain_ref(v, fwd)
    _regions(ggy, lims[1], (lims[1][0] + 32, lims[1][1] + 32), 'upsample2d_limited second backward', ref=ref, slack=slack)


# ------------------------------------------------------------------ 3. grid_sample / affine_grid_sample
THETA = torch.tensor([[[1.05, 0.1, 0.03], [-0.08, 0.95, -0.02]], [[1.6, -0.2, 0.1], [0.15, 1.7, 0.05]]])


def _mixed_grid(H, W, Ho, Wo):
    """[2, Ho, Wo, 2] f32.  Sample 0: random points in [-1.3, 1.3].  Sample 1: rows 0 .. H + 3 exactly on input pixel
    centres -- rows on centres -2 .. H + 1, columns on centres -2 .. W + 1 (left to right on even rows, right to left
    on odd ones, so two rows cover all W + 4) -- and the remaining rows far outside, |g| from 1.5 up to 1e4 in one
    coordinate (whatever the other one is, the sample is exactly 0)."""
    g = _gen(30)
    grid = torch.rand(2, Ho, Wo, 2, generator=g) * 2.6 - 1.3
    assert Ho >= H + 4 + 2 and W + 4 <= 2 * Wo
    cx = lambda j: (2 * j + 1).float() / W - 1     # noqa: E731
    cy = lambda i: (2 * i + 1).float() / H - 1     # noqa: E731
    for r in range(H + 4):
        j = torch.arange(-2, Wo - 2) if r % 2 == 0 else torch.arange(W + 1, W + 1 - Wo, -1)
        grid[1, r, :, 0] = cx(j)
        grid[1, r, :, 1] = cy(torch.tensor(r - 2))
    far = Ho - (H + 4)
    mag = torch.logspace(0.18, 4, far * Wo, dtype=torch.float32).view(far, Wo)      # 1.51 .. 1e4
    sign = torch.where(torch.rand(far, Wo, generator=g) < 0.5, -1.0, 1.0)
    axis = (torch.arange(far)[:, None] + torch.arange(Wo)[None]) % 2
    grid[1, H + 4:, :, 0] = torch.where(axis == 0, mag * sign, grid[1, H + 4:, :, 0])
    grid[1, H + 4:, :, 1] = torch.where(axis == 1, mag * sign, grid[1, H + 4:, :, 1])
    return grid


def _layouts(x):
    """(name, the input on the device) for a contiguous, a channels_last and a strided-view input: the view is
    [:, :, :H, :W] of a larger buffer whose remainder is NaN."""
    N, C, H, W = x.shape
    big = _embed(x, (N, C, H + 7, W + 5)).to(DEV)
    return [('contiguous', x.to(DEV)), ('channels_last', x.to(DEV).contiguous(memory_format=torch.channels_last)),
            ('view', big[:, :, :H, :W])]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('route', ['grid', 'affine'])
def test_grid_sample_forward_elementwise(route, dtype, monkeypatch):
    """(2, C, 20, 24) -> (2, C, 30, 26) for C in {1, 3, 5} and three input layouts, every output element within the
    derived bound (EW.grid_sample_ref) of float64 F.grid_sample; far-outside samples are exact zeros."""
    from torch_utils.ops import grid_sample_gradfix as gs
    _poison(monkeypatch)
    H, W, Ho, Wo = 20, 24, 30, 26
    grid32 = _mixed_grid(H, W, Ho, Wo)
    grid = grid32.double() if route == 'grid' else F.affine_grid(THETA.double(), [2, 1, Ho, Wo], align_corners=False)
    worst = 0.0
    for C in (1, 3, 5):
        x = torch.randn(2, C, H, W, generator=_gen(31 + C)).to(dtype)
        ref, slack = EW.grid_sample_ref(x.double(), grid, THETA if route == 'affine' else None)
        if route == 'grid':
            far = ref[1, :, H + 4:]
            assert float(far.abs().max()) == 0.0 and float(slack[1, :, H + 4:].max()) == 0.0    # exact zeros expected
        for name, xd in _layouts(x):
            if route == 'grid':
                y = gs.grid_sample(xd, grid32.to(DEV))
            else:
                y = gs.affine_grid_sample(xd, THETA.to(DEV), [2, C, Ho, Wo])
            assert y.dtype == dtype and tuple(y.shape) == (2, C, Ho, Wo)
            worst = max(worst, _elementwise(y, ref, slack, dtype, f'grid_sample fwd {route} C={C} {name}'))
    _report(f'grid_sample fwd {route}: all cases', worst, dtype)


DYN = (30, 28)


def _dyn_input(shape, seed):
    """A buffer of `shape` holding a DYN-sized image at its origin, NaN elsewhere -> (image, buffer)."""
    x = torch.randn(shape[0], shape[1], *DYN, generator=_gen(seed))
    return x, _embed(x, shape)


@pytest.mark.parametrize('route', ['grid', 'affine'])
def test_grid_sample_forward_dynamic_extent(route, monkeypatch):
    """A (2, 1, 40, 36) buffer, NaN outside its logical 30 x 28 image: finite and within the bound of the cropped
    reference."""
    from torch_utils.ops import grid_sample_gradfix as gs
    _poison(monkeypatch)
    x, buf = _dyn_input((2, 1, 40, 36), 40)
    size = [2, 1, 50, 46]
    grid = F.affine_grid(THETA.double(), size, align_corners=False)
    if route == 'grid':
        grid = grid.float().double()
        y = gs.grid_sample(buf.to(DEV), grid.float().to(DEV), dyn_hw=_i32(*DYN))
    else:
        y = gs.affine_grid_sample(buf.to(DEV), THETA.to(DEV), size, dyn_hw=_i32(*DYN))
    ref, slack = EW.grid_sample_ref(x.double(), grid, THETA if route == 'affine' else None)
    _elementwise(y, ref, slack, torch.float32, f'grid_sample fwd dyn_hw {route}')


@pytest.mark.parametrize('mode', ['scatter', 'gather'])
def test_grid_sample_backward_dynamic_extent(mode, monkeypatch):
    """The input gradient with dyn_hw in a (2, 1, 140, 60) buffer (taller than 30 + 96, narrower than 28 + 96):
    inside the logical image within the gather test's tol, zeros out to dyn + 96 (zero_region_kernel / the gather's
    own band), NaN beyond.  mode: the atomic scatter, or the deterministic gather."""
    import sg2hip
    from torch_utils.ops import grid_sample_gradfix as gs
    _poison(monkeypatch)
    _, buf = _dyn_input((2, 1, 140, 60), 41)
    size = [2, 1, 50, 46]
    dy = torch.randn(size, generator=_gen(42))
    xd = buf.to(DEV).requires_grad_(True)

    def run():
        y = gs.affine_grid_sample(xd, THETA.to(DEV), size, dyn_hw=_i32(*DYN))
        return torch.autograd.grad(y, [xd], dy.to(DEV))[0]
    if mode == 'gather':
        with sg2hip.deterministic():
            gx = run()
    else:
        gx = run()
    grid = F.affine_grid(THETA.double(), size, align_corners=False)
    ref, tol = EW.grid_sample_grad_ref((2, 1, *DYN), grid, dy.double())
    _regions(gx, DYN, (DYN[0] + R.GRAD_BAND, DYN[1] + R.GRAD_BAND), f'grid_sample bwd dyn_hw {mode}', ref=ref, slack=tol)


@pytest.mark.parametrize('dyn', [True, False], ids=['dyn_hw', 'static'])
def test_grid_sample_backward_deterministic_c5_is_refused(dyn, monkeypatch):
    """Deterministic mode handles C <= 4: C = 5 is the clean error, and nothing was launched -- the gradient buffer
    the wrapper had allocated is still all NaN."""
    import sg2hip
    from torch_utils.ops import grid_sample_gradfix as gs
    _poison(monkeypatch)
    made = []

    class Recording(poison.TorchProxy):
        def empty(self, *args, **kwargs):
            t = poison.TorchProxy.empty(self, *args, **kwargs)
            made.append(t)
            return t
    monkeypatch.setattr(gs, 'torch', Recording())
    x = torch.randn(2, 5, 40, 36, generator=_gen(43))
    size = [2, 5, 50, 46]
    xd = x.to(DEV).requires_grad_(True)
    y = gs.affine_grid_sample(xd, THETA.to(DEV), size, dyn_hw=_i32(*DYN) if dyn else None)
    del made[:]
    with sg2hip.deterministic():
        with pytest.raises(RuntimeError, match='deterministic mode supports C <= 4'):
            torch.autograd.grad(y, [xd], torch.ones_like(y))
        torch.cuda.synchronize()
    assert len(made) == 1 and tuple(made[0].shape) == tuple(x.shape)
    assert bool(torch.isnan(made[0]).all()), 'the refused call stored into the gradient buffer'


@functools.lru_cache(None)
def _second_trip():
    """N = 2, C = 1, 1450 x 1450 in and out: 2 x 1450^2 = 4,205,000 output pixels > 8192 x 256 (the forward's and the
    scatter's grid) and as many input pixels > 16384 x 256 (the gather's), so each grid-stride loop runs a second
    trip.  The float64 references are computed once for the three tests."""
    g = _gen(50)
    n = 1450
    x = torch.randn(2, 1, n, n, generator=g)
    dy = torch.randn(2, 1, n, n, generator=g)
    theta = torch.tensor([[[1.01, 0.02, 0.01], [-0.015, 0.99, -0.02]], [[0.98, -0.01, -0.015], [0.02, 1.02, 0.01]]])
    assert 2 * n * n > 8192 * 256 and 2 * n * n > 16384 * 256
    grid = F.affine_grid(theta.double(), [2, 1, n, n], align_corners=False)
    return x, dy, theta, EW.grid_sample_ref(x.double(), grid, theta), EW.grid_sample_grad_ref(x.shape, grid, dy.double())


@pytest.mark.parametrize('what', ['forward', 'scatter', 'gather'])
def test_grid_sample_second_trip(what, monkeypatch):
    import sg2hip
    from torch_utils.ops import grid_sample_gradfix as gs
    _poison(monkeypatch)
    x, dy, theta, (ref, slack), (gref, tol) = _second_trip()
    xd = x.to(DEV).requires_grad_(True)
    y = gs.affine_grid_sample(xd, theta.to(DEV), list(x.shape))
    if what == 'forward':
        _elementwise(y, ref, slack, torch.float32, 'grid_sample fwd second trip')
        return
    if what == 'gather':
        with sg2hip.deterministic():
            gx, = torch.autograd.grad(y, [xd], dy.to(DEV))
    else:
        gx, = torch.autograd.grad(y, [xd], dy.to(DEV))
    _elementwise(gx, gref, tol, torch.float32, f'grid_sample bwd second trip {what}')


def test_grid_sample_double_backward_dynamic_extent(monkeypatch):
    """With dyn_hw the gradient w.r.t. dy is a forward sample of the buffer-sized v, NaN outside the logical image."""
    from torch_utils.ops import grid_sample_gradfix as gs
    _poison(monkeypatch)
    _, buf = _dyn_input((2, 1, 40, 36), 44)
    v, vbuf = _dyn_input((2, 1, 40, 36), 45)
    size = [2, 1, 50, 46]
    xd = buf.to(DEV).requires_grad_(True)
    dyd = torch.randn(size, generator=_gen(46)).to(DEV).requires_grad_(True)
    y = gs.affine_grid_sample(xd, THETA.to(DEV), size, dyn_hw=_i32(*DYN))
    gx, = torch.autograd.grad(y, [xd], dyd, create_graph=True)
    ggo, = torch.autograd.grad(gx, [dyd], vbuf.to(DEV))
    grid = F.affine_grid(THETA.double(), size, align_corners=False)
    ref, slack = EW.grid_sample_ref(v.double(), grid, THETA)
    _elementwise(ggo, ref, slack, torch.float32, 'grid_sample double backward dyn_hw')


# ------------------------------------------------------------------ 4. producer / consumer regions of the chain
def _as_left(full, stage):
    """The buffer as its producer leaves it: `full` (the chain's true values, f32) in the computed region, zeros in
    the producer's band, NaN wherever the producer stores nothing."""
    out = torch.full_like(full, NAN)
    (cy, cx), (wy, wx) = stage['computed'], stage['written']
    out[:, :, :wy, :wx] = 0
    out[:, :, :cy, :cx] = full[:, :, :cy, :cx]
    return out.to(DEV)


def _computed(got, ref, slack, stage, what):
    cy, cx = stage['computed']
    return _elementwise(got[:, :, :cy, :cx], ref[:, :, :cy, :cx], slack[:, :, :cy, :cx], torch.float32, what)


@pytest.mark.parametrize('margins', [(0, 0, 0, 0), (3, 0, 7, 12), (31, 31, 31, 31)], ids=['zero', 'mixed', 'maximal'])
def test_chain_producer_consumer_regions(margins, monkeypatch):
    """Every adjacent pair of the chain at (2, 1, 32, 32): the consumer runs on its input as the producer leaves it
    (ada_regions.chain: values in the computed region, zeros in the band, NaN elsewhere) with the extents of
    augment_mi.py:269-278, and its computed region must be finite and within its bound of the float64 chain on the
    zero-extended logical image.  A band one row too narrow, or a consumer reaching one row too far, meets NaN."""
    from torch_utils.ops import grid_sample_gradfix as gs, reflect_pad, upfirdn2d as upf
    _poison(monkeypatch)
    N, C, h, w = 2, 1, 32, 32
    ch = R.chain(h, w, margins)
    hd, wd, dyn = ch['hd'], ch['wd'], ch['dyn_hw']
    lims = [_i32(*l) for l in ch['lims']]
    f = _sym6()
    fd = f.to(DEV)
    g = _gen(60)
    x = torch.randn(N, C, h, w, generator=g)
    hz_pad = f.shape[0] // 4
    size = [N, C, (h + 2 * hz_pad) * 2, (w + 2 * hz_pad) * 2]
    dy = torch.randn(size, generator=g)
    tag = f'chain {margins}'
    # forward: pad -> horizontal pass -> vertical pass -> sampler
    mx0, my0, mx1, my1 = margins
    p_full = _embed(F.pad(x, (mx0, mx1, my0, my1), mode='reflect'), (N, C, *ch['pad']['buf']), 0.0)
    ref, slack = EW.fir_ref(p_full, f[None], torch.float32, up=(2, 1), padding=[6, 5, 0, 0])
    y = upf._raw_lim(_as_left(p_full, ch['pad']), fd[None], 2, 1, 1, 1, 6, 5, 0, 0, False, 1.0, lims[0])
    _computed(y, ref, slack, ch['fh'], f'{tag}: pad -> horizontal up-2')
    u1 = ref.float()
    ref, slack = EW.fir_ref(u1, f[:, None], torch.float32, up=(1, 2), padding=[0, 0, 6, 5], gain=4)
    y = upf._raw_lim(_as_left(u1, ch['fh']), fd[:, None], 1, 2, 1, 1, 0, 0, 6, 5, False, 4.0, lims[1])
    _computed(y, ref, slack, ch['fv'], f'{tag}: horizontal -> vertical up-2')
    u2 = ref.float()
    grid = F.affine_grid(THETA.double(), size, align_corners=False)
    ref, slack = EW.grid_sample_ref(u2.double()[:, :, :dyn[0], :dyn[1]], grid, THETA)
    y = gs.affine_grid_sample(_as_left(u2, ch['fv']), THETA.to(DEV), size, dyn_hw=_i32(*dyn))
    _elementwise(y, ref, slack, torch.float32, f'{tag}: vertical -> sampler')
    # backward: sampler gradient -> adjoint horizontal -> adjoint vertical -> pad adjoint
    gref, _ = EW.grid_sample_grad_ref((N, C, *dyn), grid, dy.double())
    g_full = _embed(gref.float(), (N, C, *ch['sg']['buf']), 0.0)
    ref, slack = EW.fir_ref(g_full, f[None], torch.float32, down=(2, 1), padding=[5, 5, 0, 0], flip_filter=True)
    y = upf._raw_lim(_as_left(g_full, ch['sg']), fd[None], 1, 1, 2, 1, 5, 5, 0, 0, True, 1.0, lims[2])
    _computed(y, ref, slack, ch['ah'], f'{tag}: sampler gradient -> adjoint horizontal')
    a1 = ref.float()
    ref, slack = EW.fir_ref(a1, f[:, None], torch.float32, down=(1, 2), padding=[0, 0, 5, 5], flip_filter=True, gain=4)
    y = upf._raw_lim(_as_left(a1, ch['ah']), fd[:, None], 1, 1, 1, 2, 0, 0, 5, 5, True, 4.0, lims[3])
    _computed(y, ref, slack, ch['av'], f'{tag}: adjoint horizontal -> adjoint vertical')
    a2 = ref.float()
    ref, slack = EW.reflect_pad_adjoint_ref(a2.double()[:, :, :hd, :wd], (h, w), margins)
    gx = reflect_pad._Adj.apply(_as_left(a2, ch['av']), _i32(*margins), h, w)
    _elementwise(gx, ref, slack, torch.float32, f'{tag}: adjoint vertical -> pad adjoint')
