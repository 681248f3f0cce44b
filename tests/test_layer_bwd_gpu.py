"""The layer-backward kernels (csrc/layer_bwd.hip: sg2_layer_bwd, sg2_dot_hw, sg2_vjp_axpy) per lane layout, option
and mode, against CPU float64 of the rounded operands (tests/elementwise.py) -- never a kernel or a wrapper.

Layouts: a lane owns 8 channels of a pixel, LP = C / 8 lanes a pixel, PPP = 256 // LP pixels a pass.  C in
{8, 24, 64, 96, 512, 520, 1024, 2048} (LP 1, 3, 8, 12, 64, 65, 128, 256) reaches the one-lane pixel, the idle-thread
layouts, the shuffle and the LDS noise routes and a pixel that straddles waves; HW in {1, PPP + 1, one workgroup, one
workgroup + 1, 37 PPP + 5} reaches the masked tail of the 4-pixel unroll and the second workgroup; N in {1, 3} makes
the per-sample rows differ.  Both modes: float atomics, and sg2hip.deterministic() on a NaN-filled scratch.

Judge 1 (test_*_exact): operands whose every product and sum is exact in f32 and a bf16 value (EW.lb_exact_operands;
the precondition is asserted on the reference, and again in test_layer_bwd_host.py), so every output is held BITWISE
in any summation order: a dropped, doubled or misrouted term cannot hide under a tolerance.
Judge 2 (test_*_bound): random normal operands, every element within the bound derived from the kernel's arithmetic
(EW.layer_bwd_slack, vjp_axpy_slack, dot_hw_slack: roundings per term plus the longest chain of f32 additions).
Every output buffer starts as NaN: each test poisons torch.empty / empty_like of conv2d_gradfix in its own body.

Out of scope: 16-byte misaligned views, tensors at or above the 2 GB offset limit, and the kernels' speed (bench.py
times layer_bwd).

Worst error / bound ratios of Judge 2 measured on an MI355X, atomic / deterministic, the worst of fp16, bf16 and f32
(each assertion prints its own):
    layer_bwd  C     dc (16-bit; f32)   db               dd               dnoise
               24    0.995; 0.82        0.0012 / 0.0012  0.0035 / 0.0032  0.18 / 0.18
               64    0.994; 0.86        0.0036 / 0.0032  0.011 / 0.011    0.096 / 0.096
               1024  0.997; 0.86        0.023 / 0.027    0.080 / 0.061    0.0055 / refused
    vjp_axpy   C     out (16-bit; f32)  dot                      dot_hw  C     dot
    ('all')    24    0.997; 0.75        0.0044 / 0.0027                  24    0.0022 / 0.0016
               64    0.996; 0.75        0.0071 / 0.014                   64    0.0047 / 0.0039
               1024  0.996; 0.74        0.067 / 0.061                    1024  0.021 / 0.019
A 16-bit dc / out sits at its own rounding (the bound there is the output type's half ulp plus the 3 or 4 f32
roundings); the reductions sit far inside a worst-case chain bound, which still refuses a dz rounded to 16 bits (4 to
3000 x the bound in dd and dnoise) and a 16-bit accumulator (4 to 4000 x): test_layer_bwd_host.py.  The deterministic
figures equal the host replay's digit for digit where the order is fixed (vjp_axpy dot, dot_hw).
"""
import contextlib
import functools

import pytest
import torch

import elementwise as EW
import poison
import sg2hip

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CL = torch.channels_last
POISONED = ('torch_utils.ops.conv2d_gradfix',)
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAME = {F16: 'fp16', BF16: 'bf16', F32: 'f32'}
ACT = dict(act=1, **EW.LB_EXACT)
LIN = dict(act=0, alpha=0.25, gain=2.0, clamp=-1.0)
RND = dict(act=1, alpha=0.2, gain=2.0 ** 0.5, clamp=2.5)


def _cases(cs, dtypes):
    return [pytest.param(C, dt, det, id=f"{C}-{NAME[dt]}-{'det' if det else 'atomic'}")
            for C in cs for dt in dtypes for det in (False, True)]


@pytest.fixture(autouse=True)
def _scratch_left_zeroed():
    """The deterministic scratch is left as a fresh process sees it, so no later test depends on the poison."""
    yield
    poison.zero_det_scratch(DEV)


def _poison(monkeypatch):
    return poison.poisoned_empties(monkeypatch, POISONED)


@contextlib.contextmanager
def _mode(det):
    with (sg2hip.deterministic() if det else contextlib.nullcontext()):
        yield


def _run(det, fn, *args, **kw):
    """One call of a wrapper; in deterministic mode on a scratch that holds NaN."""
    if det:
        poison.poison_det_scratch(DEV)
    return fn(*args, **kw)


def _dev(op, dtype):
    """The operands on the device: activations as `dtype` in NHWC memory, the per-(n, c) factors as f32."""
    return {k: (v.to(dtype).to(DEV).contiguous(memory_format=CL) if v.dim() == 4 else v.float().to(DEV))
            for k, v in op.items()}


def _report(what, ratios):
    print(f'elementwise {what}: worst error / bound ' + ', '.join(f'{k} {r:.3g}' for k, r in ratios.items()))


# ------------------------------------------------------------------ references (computed once per shape, shared)
@functools.lru_cache(maxsize=16)
def _exact(N, C, HW):
    op = EW.lb_exact_operands(N, C, HW)
    lb = EW.layer_bwd_ref(op['dy'], op['y'], op['c'], op['d'], **ACT)
    lin = EW.layer_bwd_ref(op['dy'], op['y'], op['c'], op['d'], **LIN)
    EW.lb_assert_exact([(k, r[k]) for r in (lb, lin) for k in ('A_db', 'A_dd', 'A_dnoise')],
                       [(k, r[k]) for r in (lb, lin) for k in ('dc', 'dz')])
    return op, lb, lin


# ------------------------------------------------------------------ sg2_layer_bwd
# name -> (c given, d given, the reference's options, cg.layer_bwd keywords, acc)
LB_SETS = {
    'full': (True, True, ACT, {}, None),
    'node': (True, True, ACT, dict(want_db=False, want_dnoise=False), None),      # the create-graph node's call
    'no_c': (False, True, ACT, dict(want_dd=False), None),
    'no_d': (False, False, ACT, dict(want_dnoise=False), None),
    'linear': (True, True, LIN, {}, None),
    'acc': (True, True, ACT, {}, 'db+dd'),                                        # _fast_backward's route
    'acc_dd': (True, True, ACT, dict(want_db=False, want_dnoise=False), 'dd'),
}
ACC_FILL, ACC_TAIL = 3.0, 5


def _layer_bwd(cg, x, N, C, det, name, noise_ok=True):
    """One option set -> (the outputs it returned, acc or None); what it must and must not return is asserted."""
    has_c, has_d, opts, kw, acc_form = LB_SETS[name]
    kw = dict(kw)
    if not noise_ok:
        kw['want_dnoise'] = False
    acc = None
    if acc_form:
        acc = torch.full([(C if acc_form == 'db+dd' else 0) + N * C + ACC_TAIL], ACC_FILL, device=DEV)
        kw['acc'] = acc
    dc, db, dd, dn = _run(det, cg.layer_bwd, x['dy'], x['y'], x['c'] if has_c else None, x['d'] if has_d else None,
                          **opts, **kw)
    want = dict(dc=True, db=kw.get('want_db', True), dd=kw.get('want_dd', True) and has_c and has_d,
                dnoise=kw.get('want_dnoise', True))
    got = dict(dc=dc, db=db, dd=dd, dnoise=dn)
    for k, w in want.items():
        assert (got[k] is not None) == w, f'{name}: {k} {"missing" if w else "returned"}'
    assert dc.dtype == x['dy'].dtype and dc.is_contiguous(memory_format=CL)
    return {k: v for k, v in got.items() if v is not None}, acc


def _layer_bwd_want(ref, name, got):
    """The reference of an option set: without d, dc is dz itself; with acc, the sums sit on the fill."""
    want = dict(ref, dc=ref['dc'] if LB_SETS[name][1] else ref['dz'])
    if LB_SETS[name][4]:
        want = dict(want, **{k: want[k] + ACC_FILL for k in ('db', 'dd') if k in got})
    return want


@pytest.mark.parametrize('C,dtype,det', _cases(EW.LB_CS, (F16, BF16, F32)))
def test_layer_bwd_exact(C, dtype, det, monkeypatch):
    """Judge 1: dc, db, dd and dnoise bitwise the float64 reference for every option set at every extent and N.  With
    acc, the sums are ADDED to the caller's buffer (filled with 3.0 here) in both modes and its tail is untouched.  In
    deterministic mode the noise gradient stops at C = 512 (test_refusals): above, the sets run without it."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    noise_ok = not (det and C > 512)
    with _mode(det):
        for HW in EW.lb_hws(C):
            for N in EW.LB_NS:
                op, lb, lin = _exact(N, C, HW)
                x = _dev(op, dtype)
                for name in LB_SETS:
                    got, acc = _layer_bwd(cg, x, N, C, det, name, noise_ok)
                    ref = lin if LB_SETS[name][2] is LIN else lb
                    EW.lb_judge_exact(got, _layer_bwd_want(ref, name, got), f'layer_bwd {name} C {C} HW {HW} N {N}')
                    if acc is not None:
                        used = acc.numel() - ACC_TAIL
                        assert got['dd'].data_ptr() == acc[used - N * C:].data_ptr()
                        assert torch.equal(acc[used:].cpu(), torch.full([ACC_TAIL], ACC_FILL)), f'{name}: acc tail'


@pytest.mark.parametrize('C,dtype,det', _cases(EW.LB_BOUND_CS, (F16, BF16, F32)))
def test_layer_bwd_bound(C, dtype, det, monkeypatch):
    """Judge 2 at HW = 37 PPP + 5, N = 3: every element of dc within 3 f32 roundings before its own, every element of
    db, dd and dnoise within gamma(roundings per term + longest addition chain) of the same reduction of |terms|."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    HW, N = EW.lb_hws(C)[4], 3
    op = EW.lb_random_operands(N, C, HW, dtype)
    x = _dev(op, dtype)
    noise_ok = not (det and C > 512)
    with _mode(det):
        dc, db, dd, dn = _run(det, cg.layer_bwd, x['dy'], x['y'], x['c'], x['d'], want_dnoise=noise_ok, **RND)
    ref = EW.layer_bwd_ref(op['dy'], op['y'], op['c'], op['d'], **RND)
    got = dict(dc=dc, db=db, dd=dd, **(dict(dnoise=dn) if noise_ok else {}))
    _report(f'layer_bwd C {C} {NAME[dtype]} det {det}',
            EW.lb_judge_bound(got, ref, EW.layer_bwd_slack(ref, C, HW, N, det), dtype, 'layer_bwd'))


# ------------------------------------------------------------------ sg2_vjp_axpy
# form -> (operands given, with the activation); modconv._LayerVJP calls every one but 'all'
AX_FORMS = {
    'G_dot': (('sa', 'b', 'sb', 'e'), False),
    'axpy': (('b', 'sb'), False),
    'act': (('b', 'sb', 'y'), True),
    'scale_only': (('sa',), False),
    'a_y': (('y',), True),
    'sa_y': (('sa', 'y'), True),
    'sa_e': (('sa', 'e'), False),
    'b_no_sb': (('b',), False),
    'all': (('sa', 'b', 'sb', 'y', 'e'), True),
}


def _vjp_axpy(cg, op, x, det, form, opts):
    """One form -> (got, ref)."""
    names, act = AX_FORMS[form]
    kw = dict(opts) if act else {}
    out, dot = _run(det, cg.vjp_axpy, x['a'], **{k: x[k] for k in names}, **kw)
    assert (dot is not None) == ('e' in names)
    assert out.dtype == x['a'].dtype and out.is_contiguous(memory_format=CL)
    ref = EW.vjp_axpy_ref(op['a'], **{k: op[k] for k in names}, **kw)
    return dict(out=out, **(dict(dot=dot) if dot is not None else {})), ref


def _ax_assert_exact(ref):
    EW.lb_assert_exact([('A_dot', ref['A_dot'])] if 'dot' in ref else [], [('out', ref['out'])])


@pytest.mark.parametrize('C,dtype,det', _cases(EW.LB_CS, (F16, BF16, F32)))
def test_vjp_axpy_exact(C, dtype, det, monkeypatch):
    """Judge 1: out and dot bitwise the float64 reference for every operand form at every extent and N."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    with _mode(det):
        for HW in EW.lb_hws(C):
            for N in EW.LB_NS:
                op = _exact(N, C, HW)[0]
                x = _dev(op, dtype)
                for form in AX_FORMS:
                    got, ref = _vjp_axpy(cg, op, x, det, form, ACT)
                    _ax_assert_exact(ref)
                    EW.lb_judge_exact(got, ref, f'vjp_axpy {form} C {C} HW {HW} N {N}')


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=list(NAME.values()))
def test_vjp_axpy_narrow_exact(dtype, monkeypatch):
    """C = 3 (toRGB's output side): the wrapper's torch route, held to the same reference."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    for HW in (1, 37):
        op = EW.lb_exact_operands(3, 3, HW)
        x = _dev(op, dtype)
        for form in AX_FORMS:
            got, ref = _vjp_axpy(cg, op, x, False, form, ACT)
            _ax_assert_exact(ref)
            EW.lb_judge_exact(got, ref, f'vjp_axpy {form} C 3 HW {HW}')


@pytest.mark.parametrize('C,dtype,det', _cases(EW.LB_BOUND_CS, (F16, BF16, F32)))
def test_vjp_axpy_bound(C, dtype, det, monkeypatch):
    """Judge 2 at HW = 37 PPP + 5, N = 3: out within 4 f32 roundings (a sa, the fused b sb + v, gain, alpha) of the
    expression of |operands| before its own rounding; dot within gamma(longest addition chain) of sum |a e|."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    HW, N = EW.lb_hws(C)[4], 3
    op = EW.lb_random_operands(N, C, HW, dtype)
    x = _dev(op, dtype)
    with _mode(det):
        for form in ('all', 'G_dot', 'act'):
            got, ref = _vjp_axpy(cg, op, x, det, form, RND)
            _report(f'vjp_axpy {form} C {C} {NAME[dtype]} det {det}',
                    EW.lb_judge_bound(got, ref, EW.vjp_axpy_slack(ref, C, HW, N, det), dtype, f'vjp_axpy {form}'))


# ------------------------------------------------------------------ sg2_dot_hw
@pytest.mark.parametrize('C,dtype,det', _cases(EW.LB_CS, (F16, BF16)))
def test_dot_hw_exact(C, dtype, det, monkeypatch):
    """Judge 1 at the extents of a 32-pass workgroup."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    with _mode(det):
        for HW in EW.lb_hws(C, passes=32):
            for N in EW.LB_NS:
                op = EW.lb_exact_operands(N, C, HW)
                dot, A = EW.dot_hw_ref(op['a'], op['b'], dtype)
                EW.lb_assert_exact([('A', A)], [('a b', op['a'] * op['b'])])
                x = _dev(dict(a=op['a'], b=op['b']), dtype)
                got = _run(det, cg.dot_hw, x['a'], x['b'])
                assert got.dtype == F32
                EW.lb_judge_exact(dict(dot=got), dict(dot=dot), f'dot_hw C {C} HW {HW} N {N}')


@pytest.mark.parametrize('C,dtype,det', _cases(EW.LB_BOUND_CS, (F16, BF16)))
def test_dot_hw_bound(C, dtype, det, monkeypatch):
    """Judge 2: the sum of the ROUNDED products (as torch's a * b rounds them) within gamma(longest chain) sum |.|."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    HW, N = EW.lb_hws(C, passes=32)[4], 3
    op = EW.lb_random_operands(N, C, HW, dtype)
    x = _dev(dict(a=op['a'], b=op['b']), dtype)
    with _mode(det):
        got = _run(det, cg.dot_hw, x['a'], x['b'])
    dot, A = EW.dot_hw_ref(op['a'], op['b'], dtype)
    _report(f'dot_hw C {C} {NAME[dtype]} det {det}',
            EW.lb_judge_bound(dict(dot=got), dict(dot=dot), dict(dot=EW.dot_hw_slack(A, C, HW, N, det)), dtype, 'dot_hw'))


# ------------------------------------------------------------------ edge semantics
NAN = float('nan')
EDGE_Y = [0.0, -0.0, 2.5, -2.5, 2.4375, -2.4375, NAN, NAN, 1.0, -1.0]      # one pixel each, all 8 channels alike
EDGE_V = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, NAN, 3.0, 3.0]
# gain 2, alpha 0.25, clamp 2.5: y == 0 takes alpha; |y| == clamp is masked (strict); a NaN y gives exactly 0 even
# under a NaN gradient (the mask assigns); without a clamp nothing is masked and a NaN y takes the alpha branch
EDGE_CLAMPED = [0.5, 0.5, 0.0, 0.0, 2.0, 0.5, 0.0, 0.0, 6.0, 1.5]
EDGE_FREE = [0.5, 0.5, 2.0, 0.5, 2.0, 0.5, 0.5, NAN, 6.0, 1.5]


def _edge(vals, dtype):
    return torch.tensor(vals).view(1, 1, -1, 1).expand(1, 8, -1, 1).to(dtype).to(DEV).contiguous(memory_format=CL)


def _same(got, want):
    g, w = got.double().cpu().flatten(), torch.tensor(want).double()
    return torch.equal(g.isnan(), w.isnan()) and torch.equal(g.nan_to_num(0.0), w.nan_to_num(0.0))


@pytest.mark.parametrize('dtype', [F16, BF16, F32], ids=list(NAME.values()))
def test_edge_semantics(dtype, monkeypatch):
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    y, v = _edge(EDGE_Y, dtype), _edge(EDGE_V, dtype)
    kw = dict(act=1, alpha=0.25, gain=2.0)
    for clamp, want in ((2.5, EDGE_CLAMPED), (-1.0, EDGE_FREE)):
        dc, db, _, dn = cg.layer_bwd(v, y, clamp=clamp, **kw)
        out, _ = cg.vjp_axpy(v, y=y, clamp=clamp, **kw)
        for c in range(8):
            assert _same(dc[0, c], want), (clamp, c, dc[0, c].flatten().tolist())
            assert _same(out[0, c], want), (clamp, c, out[0, c].flatten().tolist())
        assert _same(dn, [8 * t for t in want]), (clamp, dn.flatten().tolist())
        assert _same(db, [sum(want)] * 8), (clamp, db.tolist())       # 11.0 with the clamp, NaN without
    # the oracle has the same edges (pinned on the host too)
    ref = EW.layer_bwd_ref(v.double().cpu(), y.double().cpu(), clamp=2.5, **kw)
    assert _same(ref['dz'][0, 0], EDGE_CLAMPED)


# ------------------------------------------------------------------ refusals
def _small(N, C, HW, dtype=F16):
    return _dev(EW.lb_exact_operands(N, C, HW), dtype)


def test_refusals(monkeypatch):
    """No launch: a channel count off the lane layout, and an operand of another dtype, raise with the reason."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    for C in (12, 2056):
        x = _small(1, C, 4)
        with pytest.raises(RuntimeError, match=r'sg2_layer_bwd: C must be a multiple of 8 \(<= 2048\)'):
            cg.layer_bwd(x['dy'], x['y'], x['c'], x['d'], **ACT)
    x = _small(1, 2056, 4)
    with pytest.raises(RuntimeError, match=r'sg2_vjp_axpy: C must be a multiple of 8 \(<= 2048\)'):
        cg.vjp_axpy(x['a'], x['sa'], x['b'], x['sb'])
    x = _small(2, 64, 33)
    for k in ('b', 'y', 'e'):
        with pytest.raises(RuntimeError, match='dtype'):
            cg.vjp_axpy(x['a'], x['sa'], **{k: x[k].float()}, **(dict(sb=x['sb']) if k == 'b' else {}))
    torch.cuda.synchronize()


@pytest.mark.parametrize('C', [520, 1024])
def test_det_noise_gradient_refused_above_512(C, monkeypatch):
    """Deterministic mode has no ordered noise sum for a pixel wider than a wave: the call raises, and the same
    call without the noise gradient is exact."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    HW, N = EW.lb_hws(C)[1], 3
    op, lb, _ = _exact(N, C, HW)
    x = _dev(op, BF16)
    with _mode(True):
        with pytest.raises(RuntimeError, match='C <= 512'):
            _run(True, cg.layer_bwd, x['dy'], x['y'], x['c'], x['d'], want_dnoise=True, **ACT)
        dc, db, dd, dn = _run(True, cg.layer_bwd, x['dy'], x['y'], x['c'], x['d'], want_dnoise=False, **ACT)
    assert dn is None
    EW.lb_judge_exact(dict(dc=dc, db=db, dd=dd), lb, f'layer_bwd C {C} without dnoise')


def test_dot_hw_f32_falls_back_to_torch(monkeypatch):
    """f32 operands are not the kernel's: the wrapper's torch sum, still the reference."""
    from torch_utils.ops import conv2d_gradfix as cg
    _poison(monkeypatch)
    op = EW.lb_exact_operands(3, 64, 33)
    x = _dev(dict(a=op['a'], b=op['b']), F32)
    got = cg.dot_hw(x['a'], x['b'])
    EW.lb_judge_exact(dict(dot=got), dict(dot=(op['a'] * op['b']).sum([2, 3])), 'dot_hw f32')
