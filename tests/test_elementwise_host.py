"""Mutation test of the elementwise checker (tests/elementwise.py), on the CPU.

The stand-in "kernel" is a float32 F.conv2d of the rounded operands, rounded once to the output type -- the arithmetic
the MFMA routes promise (exact 16-bit products, f32 accumulation, one final rounding).  The checker must accept it
under each rounding model, with zero exempt elements, and reject every localized fault below; for two of them the
whole-tensor rel_err stays under the suite's tolerance, which is why the checker exists."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise as E
from golden_util import rel_err

SHAPES = [(2, 64, 20, 37, 96), (1, 512, 32, 32, 512)]
BIG = (4, 64, 256, 256, 64)       # the smallest shape the C = 64 ring / persistent routes accept on 256 CUs
DTYPES = [torch.float16, torch.bfloat16]
L2_TOL = {torch.float16: 5e-3, torch.bfloat16: 2e-2}
GAIN, ALPHA, CLAMP, NG = float(np.sqrt(2)), 0.2, 1.5, 0.3


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Operands, the stand-in's f32 accumulators and the float64 reference with its |.| twin, once per case."""
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(5)
    t = dict(x=torch.randn(N, Cin, H, W, generator=g), w=torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9),
             s=torch.rand(N, Cin, generator=g) + 0.5, d=torch.rand(N, Cout, generator=g) + 0.5,
             noise=torch.randn(N, 1, H, W, generator=g), b=torch.randn(Cout, generator=g) * 0.1)
    x16, w16 = t['x'].to(dtype), t['w'].to(dtype)
    t['acc'] = F.conv2d(x16.float(), w16.float(), padding=1)                       # the stand-in, before rounding
    t['ref'] = F.conv2d(x16.double(), w16.double(), padding=1)
    t['slack'] = E.accumulation_slack(9 * Cin, F.conv2d(x16.double().abs(), w16.double().abs(), padding=1))
    return t


def _check(t, acc, dtype, what='stand-in'):
    return E.assert_elementwise(acc.to(dtype), t['ref'], t['slack'], dtype, what)


def _rejected(t, acc, dtype, where=None):
    with pytest.raises(AssertionError, match='outside the elementwise bound') as ei:
        _check(t, acc, dtype, 'fault')
    if where is not None:
        assert where in str(ei.value), str(ei.value)


# ------------------------------------------------------------------ the faults (on the f32 accumulators)
def stale_halo_tile(t, dtype, n, y0, x0):
    """One 4 x 32 tile whose top halo row is the previous tile's (4 rows up): only the tile's first row reads it."""
    x16 = t['x'].to(dtype).float()[n:n + 1].clone()
    x16[:, :, y0 - 1] = x16[:, :, y0 - 5]
    bad = F.conv2d(x16, t['w'].to(dtype).float(), padding=1)
    acc = t['acc'].clone()
    acc[n, :, y0, x0:x0 + 32] = bad[0, :, y0, x0:x0 + 32]
    return acc


def corner_tap_dropped(t, dtype):
    """The diagonal tap dropped at the four image corners, all channels."""
    x16, w16 = t['x'].to(dtype).float(), t['w'].to(dtype).float()
    acc = t['acc'].clone()
    for (oy, ky) in ((0, 2), (-1, 0)):
        for (ox, kx) in ((0, 2), (-1, 0)):
            iy, ix = (1 if oy == 0 else -2), (1 if ox == 0 else -2)
            acc[:, :, oy, ox] -= torch.einsum('oc,nc->no', w16[:, :, ky, kx], x16[:, :, iy, ix])
    return acc


def last_channel_5pct(t):
    acc = t['acc'].clone()
    acc[:, -1] *= 1.05
    return acc


def last_row_zeroed(t):
    acc = t['acc'].clone()
    acc[-1, :, -1] = 0
    return acc


def wrapped_halo_column(t, dtype):
    """The last column reads, for its right halo, the pixel that follows in memory (the next row's first column)
    instead of zero."""
    x16 = t['x'].to(dtype).float()
    H = x16.shape[2]
    xp = F.pad(x16, (1, 1, 1, 1))
    xp[:, :, 1:H, -1] = x16[:, :, 1:H, 0]
    acc = t['acc'].clone()
    acc[..., -1] = F.conv2d(xp, t['w'].to(dtype).float())[..., -1]
    return acc


def channel_duplicated(t):
    acc = t['acc'].clone()
    acc[:, 1] = acc[:, 0]
    return acc


# ------------------------------------------------------------------ the checker accepts the stand-in
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_accepts_plain(shape, dtype):
    t = _case(shape, dtype)
    assert 0 < _check(t, t['acc'], dtype) <= 1


def _mod_case(t, dtype, side):
    """(f32 accumulators, float64 reference, slack) of the modulated conv, rounding on the x or the weight side."""
    Cin = t['x'].shape[1]
    if side == 'x':
        xm = E.mod_x(t['x'], t['s'], dtype)
        w16 = t['w'].to(dtype)
        acc = F.conv2d(xm.float(), w16.float(), padding=1)
        ref = F.conv2d(xm, w16.double(), padding=1)
        A = F.conv2d(xm.abs(), w16.double().abs(), padding=1)
    else:
        wm = E.mod_w(t['w'], t['s'], dtype)
        x16 = t['x'].to(dtype)
        acc = E.conv_per_sample(x16.float(), wm.float(), padding=1)
        ref = E.conv_per_sample(x16.double(), wm, padding=1)
        A = E.conv_per_sample(x16.double().abs(), wm.abs(), padding=1)
    return acc, ref, E.accumulation_slack(9 * Cin, A)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_accepts_each_modulation_side(shape, dtype):
    """round(x round(s)) against its own reference and round(W round(s)) against its own both pass."""
    t = _case(shape, dtype)
    ax, rx, sx = _mod_case(t, dtype, 'x')
    aw, rw, sw = _mod_case(t, dtype, 'w')
    assert E.assert_elementwise(ax.to(dtype), rx, sx, dtype, 'x-side') <= 1
    assert E.assert_elementwise(aw.to(dtype), rw, sw, dtype, 'weight-side') <= 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_rejects_the_wrong_modulation_side(dtype):
    """Crossed, the two models fail: they differ by one 16-bit rounding per product, u sqrt(K) |product| in sum, which
    the L2 tolerance absorbs and this bound does not -- at K = 9 * 64.  (2, 64, 20, 37, 96): 32 245 of 142 080
    elements violate in bf16 (worst ratio 9.0), 35 in fp16 (1.41).

    Not at K = 9 * 512.  The slack is a worst case, linear in K (2 K 2^-24 A with A ~ K |product|), and passes
    u sqrt(K) |product| once K^1.5 > u 2^23: K > 256 (fp16), 1024 (bf16), leaving only the elements where the
    reference cancels.  At (1, 512, 32, 32, 512) the crossed worst ratios are 0.10 (fp16) and 0.52 / 0.59 (bf16)
    against 0.08 and 0.36 / 0.40 for the matching reference: nothing to assert, so the rounding side is pinned by the
    C <= 128 GPU cases (the ring kernels, the only weight-side routes, are C = 64 and C = 32)."""
    t = _case(SHAPES[0], dtype)
    ax, rx, sx = _mod_case(t, dtype, 'x')
    aw, rw, sw = _mod_case(t, dtype, 'w')
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        E.assert_elementwise(aw.to(dtype), rx, sx, dtype, 'weight-side kernel, x-side reference')
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        E.assert_elementwise(ax.to(dtype), rw, sw, dtype, 'x-side kernel, weight-side reference')
    assert rel_err(aw.to(dtype).float(), rx) < L2_TOL[dtype]        # ... and rel_err does not see the difference
    # the reference the tests used before, round(x s) with s unrounded, is a third model: an x-side kernel fails it
    w16 = t['w'].to(dtype).double()
    xo = (t['x'].to(dtype).float() * t['s'][:, :, None, None]).to(dtype).double()
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        E.assert_elementwise(ax.to(dtype), F.conv2d(xo, w16, padding=1),
                             E.accumulation_slack(9 * t['x'].shape[1], F.conv2d(xo.abs(), w16.abs(), padding=1)),
                             dtype, 'x-side kernel, unrounded-style reference')


def _epilogue(t, c, dtype, f32):
    d = t['d'][:, :, None, None]
    nz = t['noise'].to(dtype)
    b = t['b'].to(dtype)[None, :, None, None]
    if f32:     # the kernel's order, in f32
        v = c * d + nz.float() * np.float32(NG) + b.float()
        v = torch.where(v > 0, v, v * np.float32(ALPHA)) * np.float32(GAIN)
        return v.clamp(-CLAMP, CLAMP)
    z = c * d.double() + nz.double() * NG + b.double()
    return (F.leaky_relu(z, ALPHA) * GAIN).clamp(-CLAMP, CLAMP)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_accepts_full_epilogue(shape, dtype):
    t = _case(shape, dtype)
    acc, ref, slack = _mod_case(t, dtype, 'x')
    yr = _epilogue(t, ref, dtype, False)
    sl = E.epilogue_slack(slack, ref, t['d'][:, :, None, None], t['noise'].to(dtype).double() * NG,
                          E.bias_rounded(t['b'], dtype), GAIN, ALPHA)
    y = _epilogue(t, acc, dtype, True).to(dtype)
    assert E.assert_elementwise(y, yr, sl, dtype, 'epilogue') <= 1
    # a neighbouring channel's bias (b is ~0.1) in channel 0
    bad = y.float().clone()
    bad[:, 0] = _epilogue(t, acc + (t['b'][1] - t['b'][0]).to(dtype).float() / t['d'][:, :1, None, None], dtype, True)[:, 0]
    bad = bad.to(dtype)
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        E.assert_elementwise(bad, yr, sl, dtype, 'epilogue, offset')


def test_f32_output_has_no_rounding_term():
    t = _case(SHAPES[0], torch.float16)
    assert E.assert_elementwise(t['acc'], t['ref'], t['slack'], torch.float32, 'f32 out') <= 1
    with pytest.raises(AssertionError):
        E.assert_elementwise(t['acc'].half(), t['ref'], t['slack'], torch.float32, 'rounded, judged as f32')


# ------------------------------------------------------------------ ... and rejects every fault
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_rejects_faults(shape, dtype):
    t = _case(shape, dtype)
    N, Cin, H, W, Cout = shape
    # the bounding box names the place: sample N - 1, tile row 8, columns 0 .. 31
    _rejected(t, stale_halo_tile(t, dtype, N - 1, 8, 0), dtype, where=f'span ({N - 1}, 0, 8, 0) .. ({N - 1}, {Cout - 1}, 8, 31)')
    _rejected(t, corner_tap_dropped(t, dtype), dtype, where=f'.. ({N - 1}, {Cout - 1}, {H - 1}, {W - 1})')
    _rejected(t, last_channel_5pct(t), dtype, where=f'span (0, {Cout - 1}, 0, 0)')
    _rejected(t, last_row_zeroed(t), dtype, where=f'span ({N - 1}, 0, {H - 1}, 0) .. ({N - 1}, {Cout - 1}, {H - 1}, {W - 1})')
    _rejected(t, wrapped_halo_column(t, dtype), dtype, where=f'{W - 1}) ..')
    _rejected(t, channel_duplicated(t), dtype, where=f'span (0, 1, 0, 0) .. ({N - 1}, 1, {H - 1}, {W - 1})')


def test_l2_tolerance_passes_the_channel_fault():
    """Why the helper exists: the last channel 5 % off everywhere sits under the bf16 L2 tolerance (5.5e-3 of 2e-2)."""
    dtype = torch.bfloat16
    t = _case(SHAPES[0], dtype)
    bad = last_channel_5pct(t)
    assert rel_err(bad.to(dtype).float(), t['ref']) < L2_TOL[dtype]
    _rejected(t, bad, dtype)


def test_ring_shape_faults_pass_l2_and_fail_elementwise():
    """(4, 64, 256, 256, 64) bf16, once: a stale-halo tile, the dropped corner taps and the 5 % channel each stay under
    the 2e-2 L2 tolerance (the per-sample 2 x tolerance too) and each fails the elementwise bound."""
    dtype = torch.bfloat16
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    t = _case(BIG, dtype)
    assert _check(t, t['acc'], dtype) <= 1
    for bad in (stale_halo_tile(t, dtype, 3, 128, 64), corner_tap_dropped(t, dtype), last_channel_5pct(t)):
        assert rel_err(bad.to(dtype).float(), t['ref']) < L2_TOL[dtype]
        assert rel_err(bad[3].to(dtype).float(), t['ref'][3]) < 2 * L2_TOL[dtype]
        _rejected(t, bad, dtype)
    _case.cache_clear()


# ------------------------------------------------------------------ weight gradients: which shapes the bound resolves
# (N, A, B, OH, OW, stride, k) of the weight-gradient cases test_ops_gpu.py checks elementwise: test_wgrad3x3_halo's
# five shapes, test_conv3x3_dot_and_scaled_wgrad's small one, and test_wgrad_halo_phases' conv_s2 / convT_s2 (the same sums with the operands' roles swapped),
# conv_1x1 and conv_s2_big.
WGRAD_SHAPES = [(2, 64, 64, 32, 32, 1, 3), (3, 128, 96, 20, 37, 1, 3), (1, 512, 512, 32, 32, 1, 3),
                (2, 8, 40, 16, 16, 1, 3), (2, 72, 64, 17, 48, 1, 3), (2, 96, 64, 20, 33, 1, 3),
                (2, 72, 64, 16, 20, 2, 3), (2, 72, 64, 24, 20, 1, 1), (3, 64, 136, 33, 32, 2, 3)]
WGRAD_TOO_LARGE = (6, 128, 64, 64, 48, 2, 3)      # conv_s2_wide, N OH OW = 18 432: stays on rel_err


def _wgrad_case(shape, dtype):
    N, A, B, OH, OW, st, k = shape
    gen = torch.Generator().manual_seed(21)
    pad = 1 if (k == 3 and st == 1) else 0
    H, W = (OH - 1) * st + k - 2 * pad, (OW - 1) * st + k - 2 * pad
    g = torch.randn(N, A, OH, OW, generator=gen).to(dtype).double()
    x = torch.randn(N, B, H, W, generator=gen).to(dtype).double()
    dw, slack = E.wgrad_ref(g, x, [A, B, k, k], stride=st, padding=pad)
    x_tap = x[:, :, 0:st * (OH - 1) + 1:st, 0:st * (OW - 1) + 1:st]   # tap (pad, pad): g[oy, ox] meets x[st oy, st ox]
    return g, x, x_tap, dw, slack, pad, st


@pytest.mark.parametrize('shape', WGRAD_SHAPES)
def test_wgrad_bound_resolves_one_dropped_term(shape):
    """The slack of a weight gradient grows as (N OH OW)^2, one term does not.  At every shape the GPU tests check
    elementwise, dropping any single (n, y, x) term from the float64 sum pushes at least one element over the bound
    (the f32 output has u = 0, so the bound is the slack); the stand-in (an f32 sum) passes it."""
    dtype = torch.bfloat16
    g, x, x_tap, dw, slack, pad, st = _wgrad_case(shape, dtype)
    N, A, B, OH, OW, _, k = shape
    r = E.min_dropped_term_ratio(g, x_tap, slack[:, :, pad, pad])
    print(f'wgrad {shape}: N OH OW = {N * OH * OW}, smallest dropped-term ratio {r:.1f}')
    assert r > 1
    got = torch.nn.grad.conv2d_weight(x.float(), [A, B, k, k], g.float(), stride=st, padding=pad)
    assert E.assert_elementwise(got, dw, slack, torch.float32, 'wgrad stand-in') <= 1
    bad = got.double() - torch.einsum('a,b->ab', g[-1, :, -1, -1], x_tap[-1, :, -1, -1])[:, :, None, None] * \
        torch.nn.functional.one_hot(torch.tensor(pad * k + pad), k * k).reshape(k, k)
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        E.assert_elementwise(bad, dw, slack, torch.float32, 'wgrad, last pixel dropped at one tap')


def test_wgrad_bound_too_wide_at_18432_terms():
    """conv_s2_wide (N OH OW = 18 432): a dropped term stays inside the bound, so that case keeps rel_err only."""
    g, x, x_tap, dw, slack, pad, st = _wgrad_case(WGRAD_TOO_LARGE, torch.bfloat16)
    assert E.min_dropped_term_ratio(g, x_tap, slack[:, :, pad, pad]) < 1


# ------------------------------------------------------------------ the FIR reference
@pytest.mark.parametrize('kw', [dict(padding=[1, 1, 1, 1], gain=4), dict(padding=2), dict(down=2, padding=[1, 1, 1, 1]),
                                dict(up=2, padding=[2, 1, 2, 1], gain=4), dict(up=2, padding=[3, 0, 1, 2], flip_filter=True),
                                dict(up=2, padding=[0, 0, 0, 0], gain=4)])
def test_fir_reference_matches_the_oracle(kw):
    """fir_ref (zero-stuff, pad, correlate, decimate in float64 torch) against the CPU oracle's upfirdn2d on an
    asymmetric filter, and the stand-in (f32 FMAs, one rounding) inside its bound; a tap dropped in the last column
    is not."""
    from oracle import sg2_oracle as O
    g = torch.Generator().manual_seed(3)
    f = torch.tensor([1., 2., 5., 3.])
    f = (f[:, None] * f[None, :] / f.sum() ** 2).float()
    x = torch.randn(2, 8, 9, 13, generator=g)
    for dtype in DTYPES:
        ref, slack = E.fir_ref(x, f, dtype, **kw)
        r = O.upfirdn2d(x.to(dtype).double(), f.double(), **kw)
        assert ref.shape == r.shape and rel_err(ref, r) < 1e-12
        fk = {k: v for k, v in kw.items() if k != 'gain'}
        fg = f * torch.tensor(kw.get('gain', 1), dtype=torch.float32)
        got = E._upfirdn(x.to(dtype).float(), fg, **{**dict(up=1, down=1, padding=0, flip_filter=False), **fk})
        assert E.assert_elementwise(got.to(dtype), ref, slack, dtype, 'fir stand-in') <= 1
        bad = got.clone()
        bad[..., -1] -= (fg.max() * x.to(dtype).float().abs().amax()) * 0.25
        with pytest.raises(AssertionError, match='outside the elementwise bound'):
            E.assert_elementwise(bad.to(dtype), ref, slack, dtype, 'fir, last column off')
