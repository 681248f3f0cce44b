"""The judges of tests/test_bias_act_gpu.py, checked without a GPU.

The GPU file holds sg2_bias_act (csrc/bias_act.hip) -- forward, first- and second-order gradient -- to a float64
reference of the operands the kernel reads (elementwise.bias_act_ref), bitwise on an exact grid (Judge 1) and within a
bound derived from the kernel's f32 operations on random operands (Judge 2).  Here, on the CPU:

  * the reference against two independent sources: the recorded vectors of tests/golden/bias_act.npz, and float64
    autograd of the oracle on inputs that hold no |y| == clamp (the only points where autograd's inclusive clamp mask
    and the kernel's strict one differ);
  * the contract, written out literally: y == 0, +-clamp, one ulp inside, one ulp outside, NaN; the forward of NaN and
    +-Inf with and without a clamp; swish's recomputed yref; inv_gain at gain 0;
  * teeth: every mutant of MUTANTS, applied to the reference output of every case family it can reach, lands at least
    one element above error / bound 1, and where it cannot reach a family the structural reason is asserted;
  * the preconditions of the GPU cases: the exact fixture survives bf16 and fp16, no swish fixture with a clamp has
    an element whose recomputed |y| is within the forward slack of the clamp, the autograd-wiring fixtures have
    one-signed sums and no element within its slack of a rounding tie;
  * the C ABI's argument edges (no device work is issued).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import elementwise as EW
from golden_util import load
from oracle import sg2_oracle as O

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
NAME = {F16: 'fp16', BF16: 'bf16', F32: 'f32'}
DTYPES = [F32, F16, BF16]
NAN, INF = float('nan'), float('inf')
BA = load('bias_act.npz')


def _T(a):
    return torch.from_numpy(np.array(a)).double()


def _same(got, want):
    g, w = torch.as_tensor(got).double().flatten(), torch.tensor(want).double()
    return torch.equal(g.isnan(), w.isnan()) and torch.equal(g.nan_to_num(0.0, 7e77, -7e77), w.nan_to_num(0.0, 7e77, -7e77))


# ------------------------------------------------------------------ the reference against independent sources
def test_spec_table_is_the_products():
    from torch_utils.ops import bias_act
    assert list(EW.BA_SPEC) == list(bias_act.activation_funcs)
    for name, (alpha, gain, ref, second) in EW.BA_SPEC.items():
        s = bias_act.activation_funcs[name]
        assert (float(s.def_alpha), float(s.def_gain), s.ref, s.has_2nd_grad) == (alpha, gain, ref, second), name


@pytest.mark.parametrize('name', [str(n) for n in BA['names']])
def test_ref_matches_golden(name):
    """Forward, dx, db and ddx of the recorded f32 vectors, per element: |ref - recorded| <= 1e-6 (|recorded| + M).
    The recorded values are f32 results of f32 arithmetic, so their own rounding is relative to their TERMS: where a
    derivative cancels (1 - y y near saturation, a db that sums both signs) a bound relative to the cancelled result
    alone would measure the recording, not the reference.  M is the uncancelled scale: 0 for y, |dy| gain for dx,
    |dy v| gain for ddx, sum |dx| for db.  The gradients take the recorded y as yref, as the recording's backward did."""
    z = BA
    act, g, c = name.split('_g')[0], name.split('_g')[1].split('_c')[0], name.split('_c')[1]
    gain = None if g == 'None' else float(g)
    clamp = None if c == 'None' else float(c)
    kw = dict(dim=1, alpha=None, gain=gain, clamp=clamp, dtype=F32)
    x, b, dy, v = _T(z['x']), _T(z['b']), _T(z['dy']), _T(z['v'])
    gn = EW.f32(EW.BA_SPEC[act][1] if gain is None else gain)

    def close(ref, want, M, what):
        want = _T(want)
        bad = (ref - want).abs() > 1e-6 * (want.abs() + M)
        assert not bool(bad.any()), (name, what, int(bad.sum()), float(((ref - want).abs() / (want.abs() + M + 1e-300)).max()))

    y, _ = EW.bias_act_ref(0, act, x, b, **kw)
    close(y, z[f'{name}_y'], 0.0, 'y')
    yr = _T(z[f'{name}_y'])
    dx, _ = EW.bias_act_ref(1, act, dy, b, x, yr, None, **kw)
    close(dx, z[f'{name}_dx'], dy.abs() * gn, 'dx')
    close(dx.sum([0, 2, 3]), z[f'{name}_db'], dx.abs().sum([0, 2, 3]), 'db')
    if f'{name}_ddx' in z.files:
        ddx, _ = EW.bias_act_ref(2, act, v, b, x, yr, dy, **kw)
        close(ddx, z[f'{name}_ddx'], (dy * v).abs() * gn, 'ddx')
    else:
        assert not EW.BA_SPEC[act][3]


@pytest.mark.parametrize('clamp', [None, 0.9], ids=['noclamp', 'c0.9'])
@pytest.mark.parametrize('gain', [None, 0.7], ids=['gdef', 'g0.7'])
@pytest.mark.parametrize('act', list(EW.BA_SPEC))
def test_ref_matches_float64_autograd(act, gain, clamp):
    """Float64 autograd of the oracle (torch.clamp's inclusive mask) on operands that hold no |y| == clamp and no
    x + b == 0: forward, dx, db, the R1 product d_dy, and the second-order dx and db.  The reference's inv_gain is an f32
    value, the oracle divides exactly: 1e-6 of the uncancelled scale."""
    g = torch.Generator().manual_seed(11)
    shape = (3, 5, 4, 6)
    x, dy, v = (torch.randn(shape, generator=g, dtype=F64) for _ in range(3))
    b = torch.randn(5, generator=g, dtype=F64)
    al, gn = EW.f32(EW.BA_SPEC[act][0]), EW.f32(EW.BA_SPEC[act][1] if gain is None else gain)
    cl = EW.f32(clamp) if clamp is not None else None
    kw = dict(dim=1, alpha=al, gain=gn, clamp=cl, dtype=F64)
    xa, ba = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ya = O.bias_act(xa, ba, act=act, alpha=al, gain=gn, clamp=cl)
    pre = O.bias_act(x, b, act=act, alpha=al, gain=gn)          # before the clamp: where it saturates both mask
    assert not bool(((x + b[:, None, None]) == 0).any()) and (cl is None or not bool((pre.abs() == cl).any()))
    gx, gb = torch.autograd.grad(ya, [xa, ba], dy, create_graph=True)
    y, _ = EW.bias_act_ref(0, act, x, b, **kw)
    dx, _ = EW.bias_act_ref(1, act, dy, b, x, y, None, **kw)
    ddy, _ = EW.bias_act_ref(1, act, v, b, x, y, None, **kw)
    ddx, _ = EW.bias_act_ref(2, act, v, b, x, y, dy, **kw)

    def close(ref, want, M):
        assert bool(((ref - want.detach()).abs() <= 1e-6 * (want.detach().abs() + M)).all())
    close(y, ya, 0.0)
    close(dx, gx, dy.abs() * gn)
    close(dx.sum([0, 2, 3]), gb, dx.abs().sum([0, 2, 3]))
    if gx.requires_grad:
        hx, hb = torch.autograd.grad(gx, [xa, ba], v, allow_unused=True)
        hx = hx if hx is not None else torch.zeros_like(x)
        hb = hb if hb is not None else torch.zeros_like(b)
        close(ddx, hx, (dy * v).abs() * gn * 4)
        close(ddx.sum([0, 2, 3]), hb, ddx.abs().sum([0, 2, 3]) + 1e-30)
    else:
        assert not bool(ddx.any())
    # d_dy: the gradient is linear in dy, so its derivative along v is the same operator applied to v
    dyr = dy.clone().requires_grad_(True)
    gx2, = torch.autograd.grad(O.bias_act(xa, ba, act=act, alpha=al, gain=gn, clamp=cl), [xa], dyr, create_graph=True)
    want, = torch.autograd.grad(gx2, [dyr], v)
    close(ddy, want, v.abs() * gn)


# ------------------------------------------------------------------ the contract, literally
# the literal tables live beside the reference (elementwise.BA_EDGE_*, BA_FWD_NONFINITE): the device runs them too


@pytest.mark.parametrize('dtype', DTYPES, ids=list(NAME.values()))
def test_contract_table(dtype):
    y = torch.tensor(EW.BA_EDGE_Y[dtype], dtype=F64)
    assert torch.equal(EW.rnd(y, dtype).nan_to_num(9.0), y.nan_to_num(9.0))
    lo, at, hi = EW.ba_neighbours(2.5, dtype)
    assert [lo, at, hi] == [EW.BA_EDGE_Y[dtype][4], 2.5, EW.BA_EDGE_Y[dtype][6]]
    dy = torch.ones_like(y)
    dx, slack = EW.bias_act_ref(1, 'lrelu', dy, None, None, y, None, clamp=2.5, dtype=dtype, **EW.BA_EDGE_KW)
    assert dx.tolist() == EW.BA_EDGE_DX and float(slack[[2, 3, 6, 7, 8]].abs().max()) == 0.0
    free, _ = EW.bias_act_ref(1, 'lrelu', dy, None, None, y, None, clamp=None, dtype=dtype, **EW.BA_EDGE_KW)
    assert free.tolist() == EW.BA_EDGE_DX_FREE
    # the mask ASSIGNS: a NaN gradient under a masked y is 0, under a passing y it stays NaN
    dxn, _ = EW.bias_act_ref(1, 'lrelu', torch.full_like(y, NAN), None, None, y, None, clamp=2.5, dtype=dtype, **EW.BA_EDGE_KW)
    assert _same(dxn, [NAN, NAN, 0.0, 0.0, NAN, NAN, 0.0, 0.0, 0.0])


@pytest.mark.parametrize('act', list(EW.BA_SPEC))
def test_forward_nonfinite_table(act):
    x = torch.tensor([NAN, INF, -INF], dtype=F64)
    clamped, free = EW.BA_FWD_NONFINITE[act]
    assert _same(EW.bias_act_ref(0, act, x, None, alpha=0.25, gain=2.0, clamp=2.5)[0], clamped), act
    assert _same(EW.bias_act_ref(0, act, x, None, alpha=0.25, gain=2.0, clamp=None)[0], free), act


def test_mirrored_details():
    one = torch.ones(4, dtype=F64)
    # swish recomputes yref from xs: a stored y that would pass (0) or mask (9) changes nothing
    xs = torch.tensor([0.0, 1.0, 3.0, -3.0], dtype=F64)
    want = EW.bias_act_ref(1, 'swish', one, None, xs, None, None, gain=1.0, clamp=0.9)[0]
    assert want[2] == 0.0 and want[0] == 0.5 and want[1] != 0 and want[3] != 0      # swish(3) = 2.86 > 0.9
    for stored in (0.0, 9.0):
        got = EW.bias_act_ref(1, 'swish', one, None, xs, torch.full_like(xs, stored), None, gain=1.0, clamp=0.9)[0]
        assert torch.equal(got, want)
    # any other activation masks by the stored y, whatever x says
    got = EW.bias_act_ref(1, 'tanh', one, None, xs, torch.tensor([0.0, 0.5, 0.9, -0.5], dtype=F64), None, clamp=0.9,
                          dtype=F64)[0]
    assert got.tolist() == [1.0, 0.75, 0.0, 0.75]
    # inv_gain is 0 at gain 0: yy = 0, every result exactly 0 and finite (yref / gain would be Inf or NaN)
    y = torch.tensor([0.0, 1.0, -1.0, 2.0], dtype=F64)
    for act in EW.BA_SPEC:
        for grad in (1, 2):
            r, s = EW.bias_act_ref(grad, act, one, None, y, y, one, gain=0.0, clamp=None)
            assert r.tolist() == [0.0] * 4 and bool(torch.isfinite(s).all()), (act, grad)
    # inv_gain is the f32 quotient: yy = y fl(1 / 0.7f), and 1 - yy yy sees it
    r, _ = EW.bias_act_ref(1, 'tanh', one[:1], None, None, torch.tensor([0.5], dtype=F64), None, gain=0.7)
    inv = float(torch.tensor(1.0) / torch.tensor(0.7))
    assert float(r) == (1 - (0.5 * inv) ** 2) * EW.f32(0.7)
    # the cut-offs: softplus forwards v above 20, swish' is g above 40 and its second derivative 0
    assert EW.bias_act_ref(0, 'softplus', torch.tensor([20.5], dtype=F64))[0].tolist() == [20.5]
    assert EW.bias_act_ref(1, 'swish', one[:1], None, torch.tensor([40.5], dtype=F64), None, None, gain=2.0)[0].tolist() == [2.0]
    assert EW.bias_act_ref(2, 'swish', one[:1], None, torch.tensor([40.5], dtype=F64), None, one[:1], gain=2.0)[0].tolist() == [0.0]


def test_slack_model_constants():
    """The three documented constants and the shape of the model: one f32 rounding for a sum, an absolute bound
    through a cancellation, (2 |x| + 4) 2^-24 for __expf."""
    assert (EW.BA_EXP_HW_ULPS, EW.BA_TANH_ULPS, EW.BA_LOG1P_ULPS) == (4, 5, 2)
    e = EW.EPS32
    one = torch.ones((), dtype=F64)
    assert float(EW._ba_add(EW._z(one), EW._z(-one))[1]) == 2 * e            # 1 - 1: absolute, of the terms
    v, s = EW._ba_exp(EW._z(3 * one))
    assert abs(float(s) - (10 * e * float(v) + 2.0 ** -126)) < 1e-20
    y, s = EW.bias_act_ref(0, 'tanh', one.view(1))
    assert abs(float(s) - (5 * 2 * e * float(y) + e * float(y) * (1 + 10 * e))) < 1e-12     # tanh, then the gain
    y, s = EW.bias_act_ref(0, 'lrelu', -one.view(1), torch.tensor([0.5], dtype=F64), alpha=0.25, gain=2.0, clamp=0.125)
    assert y.tolist() == [-0.125] and s.tolist() == [0.0]                      # a clamp the value cannot leave


# ------------------------------------------------------------------ teeth
MUTANTS = ('bias_shift_tail', 'bias_other_layout', 'tail_stale', 'second_sweep', 'alpha_dropped', 'gain_twice',
           'inclusive_mask', 'swish_mask_open', 'd2_dy_dropped')
SWEEP_FAMILIES = [f'sweep{k}' for k in (0, 1)]
FAMILIES = list(EW.BA_CASES) + SWEEP_FAMILIES


def _family(name, dtype):
    if name in EW.BA_CASES:
        return EW.BA_CASES[name]
    return (EW.ba_sweep_shape(dtype, EW.ba_sweep_extras(dtype)[int(name[-1])]), 1, False, True, None)


@functools.lru_cache(maxsize=4)
def _fix(name, dtype, act, gain, clamp):
    shape, dim, cl, bias, view = _family(name, dtype)
    op = EW.ba_fixture(shape, dim, bias, dtype, act, gain=gain, clamp=clamp)
    if view == 'expanded_dy':
        op['dy'] = torch.ones_like(op['dy'])
    return op


def _lands(mut, ref, slack, dtype):
    return float(EW.ratios(mut.nan_to_num(1e30), ref, slack, dtype).max()) > 1


def _by_flat(op, cl, fn):
    """A bias given per element through fn(flat index) -> channel."""
    i = torch.arange(op['x'].numel())
    return EW.ba_unflat(op['b'][fn(i)], op['shape'], cl)


@pytest.mark.parametrize('dtype', DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize('family', FAMILIES)
def test_mutants_are_refused(family, dtype):
    """Every mutant on every family: it lands above the bound, or it cannot reach the family for the stated reason."""
    shape, dim, cl, bias, view = _family(family, dtype)
    big = family in SWEEP_FAMILIES
    V, n = EW.BA_V[dtype], int(np.prod(shape))
    tail, C = n % V, shape[dim]
    step = EW.ba_step(shape, dim, cl)
    landed = {}
    # ---- the index mutants: lrelu forward without a clamp (every element depends on its bias), swish at the gradients
    outs = [('lrelu', 0)] if big else [('lrelu', 0), ('swish', 0), ('swish', 1), ('swish', 2)]
    for act, grad in outs:
        op = _fix(family, dtype, act, None, None)
        ref, slack = EW.ba_ref(op, grad)
        flat = EW.ba_flat(ref, cl)
        if bias and C > 1 and tail:
            m = EW.ba_flat(EW.ba_ref(op, grad, b=op['b'].roll(1))[0], cl)
            mut = flat.clone()
            mut[n - tail:] = m[n - tail:]
            landed['bias_shift_tail', act, grad] = _lands(EW.ba_unflat(mut, shape, cl), ref, slack, dtype)
        other = 1 if step != 1 else int(np.prod(shape[dim + 1:]))
        if bias and C > 1 and other != step and not big:
            assert torch.equal(_by_flat(op, cl, lambda i: (i // step) % C), EW.ba_bias(op['b'], op['x'], dim).expand(shape))
            m = EW.ba_ref(op, grad, b=_by_flat(op, cl, lambda i: (i // other) % C))[0]
            landed['bias_other_layout', act, grad] = _lands(m, ref, slack, dtype)
        if tail and n > tail:
            mut = flat.clone()
            mut[n - tail:] = mut[n - tail - 1]
            landed['tail_stale', act, grad] = _lands(EW.ba_unflat(mut, shape, cl), ref, slack, dtype)
        if big:
            S = EW.BA_SWEEP * V
            assert n > S
            mut = flat.clone()
            mut[S:] = flat[:n - S]
            landed['second_sweep', act, grad] = _lands(EW.ba_unflat(mut, shape, cl), ref, slack, dtype)
    if not big:
        assert n <= EW.BA_SWEEP * V         # one sweep: the second_sweep mutant has nothing to move
    # ---- the arithmetic mutants
    for grad in ((0,) if big else (0, 1)):
        op = _fix(family, dtype, 'lrelu', None, None)
        ref, slack = EW.ba_ref(op, grad)
        landed['alpha_dropped', 'lrelu', grad] = _lands(EW.ba_ref(op, grad, alpha=0.0)[0], ref, slack, dtype)
    if not big:
        for act in ('lrelu', 'swish'):
            op = _fix(family, dtype, act, 0.7, None)
            ref, slack = EW.ba_ref(op, 1)
            landed['gain_twice', act, 1] = _lands(ref * EW.f32(0.7), ref, slack, dtype)
        op = _fix(family, dtype, 'lrelu', None, 256.0)
        ref, slack = EW.ba_ref(op, 1)
        at = op['y'].abs() == 256.0
        assert int(at.sum()) >= 2 and bool((ref[at] == 0).all())
        landed['inclusive_mask', 'lrelu', 1] = _lands(torch.where(at, EW.ba_ref(op, 1, clamp=None)[0], ref), ref, slack, dtype)
        op = _fix(family, dtype, 'swish', None, 0.9)
        for grad in (1, 2):
            ref, slack = EW.ba_ref(op, grad)
            masked = EW.bias_act_ref(0, 'swish', op['x'], op['b'], **dict(op['kw'], clamp=None))[0].abs() >= EW.f32(0.9)
            if bool(masked.any()):
                landed['swish_mask_open', 'swish', grad] = _lands(EW.ba_ref(op, grad, clamp=None)[0], ref, slack, dtype)
            else:
                assert n < 15, 'only the smallest families may hold no masked element'
        if view != 'expanded_dy':           # (dy is all ones there: dropping the factor changes nothing)
            op = _fix(family, dtype, 'swish', None, None)
            ref, slack = EW.ba_ref(op, 2)
            landed['d2_dy_dropped', 'swish', 2] = _lands(EW.ba_ref(op, 2, dy=torch.ones_like(op['dy']))[0], ref, slack, dtype)
    missed = [k for k, v in landed.items() if not v]
    assert not missed, f'{family} {NAME[dtype]}: mutants inside the bound: {missed}'
    # what could not reach this family, and why
    reached = {k[0] for k in landed}
    for m in set(MUTANTS) - reached:
        why = {'bias_shift_tail': not (bias and C > 1 and tail), 'tail_stale': not (tail and n > tail),
               'bias_other_layout': big or not bias or C == 1 or (1 if step != 1 else int(np.prod(shape[dim + 1:]))) == step,
               'second_sweep': not big, 'gain_twice': big, 'inclusive_mask': big, 'swish_mask_open': big or n < 15,
               'd2_dy_dropped': big or view == 'expanded_dy'}[m]
        assert why, (family, m)


def test_every_mutant_reaches_a_family():
    """The union over the families leaves no mutant without teeth (each family's own test asserts its landings)."""
    reach = {m: 0 for m in MUTANTS}
    for family in FAMILIES:
        shape, dim, cl, bias, view = _family(family, F16)
        n, big = int(np.prod(shape)), family in SWEEP_FAMILIES
        tail, C, step = n % 8, shape[dim], EW.ba_step(shape, dim, cl)
        other = 1 if step != 1 else int(np.prod(shape[dim + 1:]))
        reach['bias_shift_tail'] += bool(bias and C > 1 and tail)
        reach['bias_other_layout'] += bool(bias and C > 1 and other != step and not big)
        reach['tail_stale'] += bool(tail and n > tail)
        reach['second_sweep'] += big
        for m in ('alpha_dropped',):
            reach[m] += 1
        for m in ('gain_twice', 'inclusive_mask', 'swish_mask_open'):
            reach[m] += not big
        reach['d2_dy_dropped'] += not big and view != 'expanded_dy'
    assert all(v >= 2 for v in reach.values()), reach
    assert reach['bias_other_layout'] >= 8 and reach['bias_shift_tail'] >= 12


# ------------------------------------------------------------------ preconditions of the GPU cases
@pytest.mark.parametrize('family', list(EW.BA_CASES))
def test_exact_fixture_precondition(family):
    """Judge 1: every operand, the forward and the gradient of linear, relu and lrelu (alpha 0.25, gain 2, clamp 2.5
    and none) is a bf16 and an fp16 value, and y == 0 and |y| == clamp are frequent where the family is not tiny."""
    shape, dim, cl, bias, view = EW.BA_CASES[family]
    zero = at = total = 0
    for act in ('linear', 'relu', 'lrelu'):
        for clamp in (EW.BA_EXACT['clamp'], None):
            op = EW.ba_fixture(shape, dim, bias, BF16, act, gain=EW.BA_EXACT['gain'], clamp=clamp,
                               alpha=EW.BA_EXACT['alpha'], exact=True, plant=False)
            y, sy = EW.ba_ref(op, 0)
            dx, _ = EW.ba_ref(op, 1)
            EW.lb_assert_exact([], [(k, op[k]) for k in ('x', 'dy', 'y')] + [('y ref', y), ('dx', dx)])
            assert torch.equal(op['y'], y)
            if clamp is not None:
                zero, at, total = zero + int((y == 0).sum()), at + int((y.abs() == clamp).sum()), total + y.numel()
    if total >= 3 * 78:
        assert zero > 0.02 * total and at > 0.1 * total, (zero, at, total)


def _swish_margin(op):
    """min over the elements of (| |y| - clamp | - forward slack) for the RECOMPUTED y of a swish fixture."""
    y, s = EW.bias_act_ref(0, 'swish', op['x'], op['b'], **dict(op['kw'], clamp=None))
    return float(((y.abs() - EW.f32(op['kw']['clamp'])).abs() - s).min())


@pytest.mark.parametrize('dtype', DTYPES, ids=list(NAME.values()))
def test_swish_clamp_precondition(dtype):
    """No random swish fixture with a clamp holds an element whose recomputed |y| is within the forward slack of the
    clamp: the kernel's f32 recomputation and float64 then fall on the same side of the strict mask everywhere."""
    for family in EW.BA_CASES:
        shape, dim, cl, bias, view = EW.BA_CASES[family]
        for gain in EW.BA_GAINS:
            for clamp in EW.BA_CLAMPS[1:]:
                op = EW.ba_fixture(shape, dim, bias, dtype, 'swish', gain=gain, clamp=clamp)
                assert _swish_margin(op) > 0, (family, gain, clamp)


def test_sweep_shapes():
    for dtype in DTYPES:
        V = EW.BA_V[dtype]
        for extra in EW.ba_sweep_extras(dtype):
            R, C = EW.ba_sweep_shape(dtype, extra)
            n = R * C
            assert C > 1 and n > EW.BA_SWEEP * V and n % V != 0 and n - EW.BA_SWEEP * V <= 4 * 256 * V + V, (R, C)
    assert EW.BA_SWEEP == 1048576


@pytest.mark.parametrize('dtype', [F32, F16], ids=['f32', 'fp16'])
def test_wiring_fixture_precondition(dtype):
    """The autograd-wiring sums: every term of gb and of the second-order d_b has one sign (so the bound's u |ref|
    term is the whole sum's), and in fp16 no reference element is within its slack of a rounding tie (so the stored
    dx is the rounded reference and the float64 sum of the rounded reference is what the device sums)."""
    for act, clamp in EW.BA_WIRING:
        for cl in (False, True):
            for dim in (1, 2):
                op = EW.ba_wiring_fixture(act, clamp, dtype, dim)
                assert op['seed'] < 16 and (clamp is None or _swish_margin(op) > 0)
                for grad in (1, 2):
                    ref, slack = EW.ba_ref(op, grad)
                    assert bool((ref >= 0).all()) or bool((ref <= 0).all()), (act, grad)
                    assert not bool(EW.ba_near_tie(ref, slack, dtype).any()), (act, grad, dim)


# ------------------------------------------------------------------ the C ABI's edges (no device work is issued)
def test_abi_edges():
    import sg2hip
    lib = sg2hip.lib()
    p = ctypes.c_void_p(16)

    def call(numel=10, size_b=1, step_b=1, grad=0, b=None):
        return lib.sg2_bias_act(p, p, b, None, None, None, 0, numel, size_b, step_b, grad, 3, 0.2, 1.0, -1.0, None)
    assert call(grad=3) < 0 and b'grad must be 0, 1 or 2' in lib.sg2_last_error()
    assert call(grad=-1) < 0
    assert call(numel=2 ** 31) < 0 and b'too large' in lib.sg2_last_error()
    assert call(numel=-1) < 0
    assert call(b=p, size_b=0) < 0 and b'bias geometry' in lib.sg2_last_error()
    assert call(b=p, step_b=0) < 0 and b'bias geometry' in lib.sg2_last_error()
    assert call(numel=0) == 0
    assert call(numel=0, b=p, size_b=3, step_b=1, grad=2) == 0
    # an empty tensor has no storage: numel == 0 is a no-op whatever the pointers are
    assert lib.sg2_bias_act(None, None, None, None, None, None, 0, 0, 1, 1, 0, 3, 0.2, 1.0, -1.0, None) == 0
