"""The f32 convolutions of csrc/conv.hip per arithmetic form, reduction form and dispatch edge, against CPU float64 of
the operands as the kernels round them (tests/elementwise.py) -- never a kernel or a product wrapper.

Arithmetic forms: 's3' (the three-way bf16 split staged in-loop), 'p3' (the planes of sg2_split3, where
conv2d_gradfix._p3 holds) and 'exact' (SG2_F32_EXACT=1, the f32-input MFMA).  Reduction forms: no split (the wrapper
passes no workspace), atomic split-K, and sg2hip.deterministic() on a NaN-filled scratch; dw: atomic and
deterministic, and under p3 the parameter-layout slot sums (sg2_conv2d_wgrad_oikk, plain and 'swap').  Every output
buffer starts as NaN (torch.empty of conv2d_gradfix is poisoned).

Judge 1 (test_*_exact): the integer fixture -- every product and partial sum exact in f32 in any order and in all three
forms (the precondition is asserted on the reference; test_conv_f32_host.py) -- held BITWISE for y, aux, dot and dw.
Judge 1 (test_*_planes): three fixtures with one product per output on which the six-product scheme is exact and each
plane product is load-bearing (x24: l h', m h', h h'; w24: h l', h m', h h'; mm: m m', m h', h m', h h'): a dropped,
doubled or misrouted plane is a bitwise mismatch, where it would be 2^-16 of a result under any tolerance.
Judge 2 (test_*_bound): seeded normal operands, every element within the derived bound (EW.conv_f32_slack through
EW.epilogue_slack); a NaN fails.  Each assertion prints its worst error / bound ratio.

The shapes (EW.CF_FWD_CASES, EW.CF_WGRAD_CASES) are the smallest that reach each edge of the host dispatch: ragged M, N
and K tiles, a tile spanning samples, short and empty splits, the early-return tile of a short transposed phase, the
scalar-load form, the 1x1 small-depth kernels in f32 and their generic fall-through (test_conv_f32_host.py asserts the
reach on EW.conv_fwd_plan / conv_wgrad_plan).  The plans assume the default split targets, so SG2_CONV_SPLIT_WGS and
SG2_CWGRAD_WGS must be unset.

Out of scope: f32 subnormals (operands, or residuals of the split below 2^-126), 16-byte misaligned views, more than
four phases (stride > 2 transposed), and speed.

Worst error / bound ratios of Judge 2 measured on an MI355X (records, not thresholds; each assertion prints its own).
The generic GEMM at K >= 24, no split / atomic split-K / deterministic (dw: atomic / deterministic):
                 s3                          p3                          exact
    y, aux       0.0087 / 0.0026 / 0.0087    0.013 / 0.0026 / 0.013      0.059 / 0.017 / 0.059
    dot          0.0020 / 0.00046 / 0.00092  0.0016 / 0.00052 / 0.00085  0.0097 / 0.0028 / 0.0095
    dw           0.0052 / 0.0052             0.0052 / 0.0052             0.041 / 0.037
    dw, parameter layout (plain / swap)      0.0052 / 0.0052
K = 3 on the generic GEMM (fk40): y, aux 0.12 (s3), 0.23 (exact); dot 0.015, 0.026.  The small-depth 1x1 kernels (f32
FMAs whatever the form): y, aux 0.39, dot 0.046, dw 0.0038 -- with K <= 3 the bound is a few f32 ulps.
A library with l h' or m m' taken out of mfma_s3, or with the m and l planes of x exchanged in the P3 weight-gradient
staging, fails the x24 / mm plane tests of every route it touches and, of everything else here, one K = 3 bound case.
"""
import contextlib
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import elementwise as EW
import poison
import sg2hip

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CL = torch.channels_last
F32 = torch.float32
FWD, WGRAD = EW.CF_FWD_CASES, EW.CF_WGRAD_CASES
FULL = dict(in_scale=True, out_scale=True, noise=True, bias=True, residual=True)
MODES = {'plain': None, 'full': dict(aux_mode=2, **FULL), 'dot': dict(aux_mode=1, dot=True, **FULL)}


def _cg():
    from torch_utils.ops import conv2d_gradfix as cg
    return cg


@pytest.fixture(autouse=True)
def _poisoned(monkeypatch):
    assert 'SG2_CONV_SPLIT_WGS' not in os.environ and 'SG2_CWGRAD_WGS' not in os.environ, 'the plans assume the defaults'
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.conv2d_gradfix'])
    yield
    poison.zero_det_scratch(DEV)


def _set_form(monkeypatch, form):
    cg = _cg()
    monkeypatch.setattr(cg, 'presplit', form == 'p3')
    monkeypatch.setattr(cg, 'presplit_fwd', form == 'p3')
    if form == 'exact':
        monkeypatch.setenv('SG2_F32_EXACT', '1')      # read by the library at every launch
    else:
        monkeypatch.delenv('SG2_F32_EXACT', raising=False)
    return cg


@contextlib.contextmanager
def _reduction(monkeypatch, red):
    """'nosplit': no workspace reaches the library; 'atomic': the default; 'det': fixed-order slots (of a scratch
    that _poison_scratch fills with NaN before every call)."""
    with monkeypatch.context() as mp:
        if red == 'nosplit':
            mp.setattr(_cg(), '_WS_LIMIT', 0)
        if red == 'det':
            with sg2hip.deterministic():
                yield
        else:
            yield


def _poison_scratch():
    """Before every deterministic call: NaN into the scratch whose slots the call must write before it reads them."""
    if sg2hip.det_active():
        poison.poison_det_scratch(DEV)


def _nhwc(t):
    return t.float().to(DEV).contiguous(memory_format=CL)


def _fwd_params(names=None):
    return [pytest.param(n, f, id=f'{n}-{f}') for n in (names or FWD) for f in EW.cf_forms(FWD[n][5])]


def _wgrad_forms(name):
    A, B, k = WGRAD[name][:3]
    return EW.cf_forms((A, B), wgrad_1x1_small=k == 1 and min(A, B) <= 4)


def _wgrad_params(names=None):
    return [pytest.param(n, f, id=f'{n}-{f}') for n in (names or WGRAD) for f in _wgrad_forms(n)]


def _fwd_reductions(case, form):
    reds = ['nosplit']
    if EW.conv_fwd_plan(*case, form=form)['splits'] > 1:
        reds.append('atomic')
    return reds + ['det']


# ------------------------------------------------------------------ forward and input gradient
@functools.lru_cache(maxsize=None)
def _fwd_exact(name):
    return EW.cf_fwd_exact_refs(FWD[name])


@functools.lru_cache(maxsize=None)
def _fwd_random_op(name):
    return EW.cf_fwd_operands(FWD[name], 'random')


@functools.lru_cache(maxsize=None)
def _fwd_random_ref(name, slack_form, S, depth, mode):
    kw = MODES[mode]
    kw = dict(epi=EW.CF_RANDOM, **kw) if kw else {}
    return EW.cf_fwd_ref(FWD[name], _fwd_random_op(name), slack_form, S, depth, **kw)


def _fwd_dev(case, op):
    d = {k: (_nhwc(v) if v.dim() == 4 and k != 'noise' else v.float().to(DEV).contiguous())
         for k, v in op.items() if k != 'w'}
    d['wp'] = EW.cf_pack(op['w'], case[3]).float().to(DEV)
    return d


def _fwd_call(cg, case, d, mode, epi, form):
    k, stride, pad, tr, N, Cin, H, W, Cout = case
    OH, OW = EW.cf_out_hw(k, stride, pad, tr, H, W)
    if form == 'p3':
        assert cg.presplit_fwd and cg._p3(d['x'], Cin), 'the case does not take the pre-split route'
    _poison_scratch()
    if mode == 'plain':
        return dict(y=cg._conv_raw(d['x'], d['wp'], Cout, OH, OW, k, k, stride, (pad, pad), tr))
    out = cg.conv_fused(d['x'], d['wp'], Cout, OH, OW, k, k, stride, (pad, pad), transpose=tr, in_scale=d['in_scale'],
                        out_scale=d['out_scale'], noise=d['noise'], noise_gain=epi['noise_gain'], bias=d['bias'],
                        act=epi['act'], alpha=epi['alpha'], gain=epi['gain'], clamp=epi['clamp'], residual=d['residual'],
                        aux_mode=MODES[mode]['aux_mode'], dot_src=d['dot_src'] if mode == 'dot' else None)
    got = dict(y=out[0], aux=out[1])
    if mode == 'dot':
        got['dot'] = out[2]
    return got


def _assert_workspace_clean(cg):
    ws = cg._CLEAN_WS.get(DEV)
    assert ws is not None, 'no split-K call took the persistent workspace'
    assert not bool(ws.any()), 'an atomic split-K call left the persistent workspace dirty'


@pytest.mark.parametrize('name,form', _fwd_params())
def test_fwd_exact(name, form, monkeypatch):
    """Judge 1 on the integer fixture: y, aux and dot bitwise, in every reduction form, plain and with the full
    epilogue (in_scale, out_scale, noise, bias, lrelu, gain, clamp, residual; aux_mode 2, and aux_mode 1 with dot)."""
    cg = _set_form(monkeypatch, form)
    case = FWD[name]
    op, refs = _fwd_exact(name)
    d = _fwd_dev(case, op)
    for red in _fwd_reductions(case, form):
        with _reduction(monkeypatch, red):
            for mode in MODES:
                got = _fwd_call(cg, case, d, mode, EW.CF_EXACT, form)
                EW.lb_judge_exact(got, refs[mode], f'conv_f32 fwd {name} {form} {red} {mode}')
        if red == 'atomic':
            _assert_workspace_clean(cg)


@pytest.mark.parametrize('name,form', _fwd_params())
def test_fwd_plan_split_matches_library(name, form, monkeypatch):
    """The plan's split decision is the library's: with 1.0 planted in the persistent workspace, a call that splits K
    adds into it (every y is the exact result + 1, and the finalize leaves what it read zeroed); a call that does not
    split never touches it."""
    cg = _set_form(monkeypatch, form)
    case = FWD[name]
    op, refs = _fwd_exact(name)
    d = _fwd_dev(case, op)
    split = EW.conv_fwd_plan(*case, form=form)['splits'] > 1
    _fwd_call(cg, case, d, 'plain', None, form)         # (creates the workspace on a fresh process)
    ws, clean = cg._workspace(d['x'], refs['plain']['y'].numel())
    assert clean and ws is cg._CLEAN_WS[DEV]
    try:
        ws.fill_(1.0)
        got = _fwd_call(cg, case, d, 'plain', None, form)
        EW.lb_judge_exact(got, dict(y=refs['plain']['y'] + (1.0 if split else 0.0)), f'conv_f32 fwd {name} {form} planted')
        n = refs['plain']['y'].numel()
        assert float(ws[:n].abs().max()) == (0.0 if split else 1.0) and float(ws[n:].min()) == 1.0
    finally:
        ws.zero_()


@pytest.mark.parametrize('name,form', _fwd_params())
def test_fwd_bound(name, form, monkeypatch):
    """Judge 2 on seeded normal operands: every element of y, aux and dot within the derived bound."""
    cg = _set_form(monkeypatch, form)
    case = FWD[name]
    d = _fwd_dev(case, _fwd_random_op(name))
    for red in _fwd_reductions(case, form):
        with _reduction(monkeypatch, red):
            for mode in MODES:
                plan = EW.conv_fwd_plan(*case, form=form, workspace=red != 'nosplit', dot=mode == 'dot')
                slack_form = form if plan['family'] == 'generic' else 'exact'       # the 1x1 small-depth kernels: f32 FMAs
                depth = plan['dot_depth'](red == 'det') if mode == 'dot' else 1
                ref = _fwd_random_ref(name, slack_form, plan['splits'], depth, mode)
                got = _fwd_call(cg, case, d, mode, EW.CF_RANDOM, form)
                what = f'conv_f32 fwd {name} {form} {red} {mode}'
                r = {k: EW.assert_elementwise(v, ref[k], ref[f'slack_{k}'], F32, f'{what} {k}') for k, v in got.items()}
                print(f'elementwise {what}: worst error / bound ' + ', '.join(f'{k} {v:.3g}' for k, v in r.items()))


def _plane_params(names, forms_of):
    return [pytest.param(n, f, kind, id=f'{n}-{f}-{kind}') for n in names for f in forms_of(n) if f != 'exact'
            for kind in EW.CF_PLANE_FIXTURES]


@pytest.mark.parametrize('name,form,kind', _plane_params(EW.CF_PLANE_FWD, lambda n: EW.cf_forms(FWD[n][5])))
def test_fwd_planes(name, form, kind, monkeypatch):
    """Judge 1 on the plane fixtures: one product per output, each plane product load-bearing; bitwise."""
    cg = _set_form(monkeypatch, form)
    case = FWD[name]
    k, stride, pad, tr, N, Cin, H, W, Cout = case
    for sparse in ('a', 'b'):
        x, w = EW.cf_plane_fwd_operands(case, kind, sparse)
        terms = F.conv2d((x != 0).double(), (w != 0).double(), stride=stride, padding=pad)
        ref = F.conv2d(x, w, stride=stride, padding=pad)
        EW.cf_plane_assert_one_term(terms, ref, (name, kind, sparse))
        d = dict(x=_nhwc(x), wp=EW.cf_pack(w, tr).float().to(DEV))
        for red in ('nosplit', 'det'):
            with _reduction(monkeypatch, red):
                got = _fwd_call(cg, case, d, 'plain', None, form)
            EW.lb_judge_exact(got, dict(y=ref), f'conv_f32 fwd planes {name} {form} {kind} sparse {sparse} {red}')


# ------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=None)
def _wgrad_exact(name):
    return EW.cf_wgrad_exact_refs(WGRAD[name])


@functools.lru_cache(maxsize=None)
def _wgrad_random_op(name):
    return EW.cf_wgrad_operands(WGRAD[name], 'random')


def _wgrad_dev(op):
    return {k: (_nhwc(v) if v.dim() == 4 else v.float().to(DEV).contiguous()) for k, v in op.items()}


def _wgrad_call(cg, case, d, scaled, alpha, form, param_layout=False):
    A, B, k, stride, pad, N, OH, OW = case
    if form == 'p3':
        assert cg._p3(d['g'], 8) and A % 8 == 0 and B % 8 == 0 and not (k == 1 and min(A, B) <= 4), 'not a pre-split case'
        assert not param_layout or (sg2hip.det_active() and B % 4 == 0 and k * k <= 9)
    _poison_scratch()
    dw = cg._wgrad_raw(d['g'], d['x'], k, k, stride, (pad, pad), x_scale=d['x_scale'] if scaled else None,
                       g_scale=d['g_scale'] if scaled else None, alpha=alpha, param_layout=param_layout)
    assert tuple(dw.shape) == (A, B, k, k)
    return dw


def _wgrad_routes(case, form):
    """(reduction, param_layout, label)"""
    routes = [('atomic', False, 'atomic'), ('det', False, 'det')]
    if form == 'p3' and case[1] % 4 == 0:
        routes += [('det', True, 'det-oikk'), ('det', 'swap', 'det-oikk-swap')]
    return routes


@pytest.mark.parametrize('name,form', _wgrad_params())
def test_wgrad_exact(name, form, monkeypatch):
    """Judge 1 on the integer fixture: dw bitwise with both scales and alpha, and with none."""
    cg = _set_form(monkeypatch, form)
    case = WGRAD[name]
    op, refs = _wgrad_exact(name)
    d = _wgrad_dev(op)
    for red, layout, label in _wgrad_routes(case, form):
        with _reduction(monkeypatch, red):
            for which, scaled, alpha in (('scaled', True, EW.CF_WGRAD_ALPHA['exact']), ('plain', False, 1.0)):
                dw = _wgrad_call(cg, case, d, scaled, alpha, form, layout)
                EW.lb_judge_exact(dict(dw=dw), dict(dw=refs[which]), f'conv_f32 dw {name} {form} {label} {which}')


@pytest.mark.parametrize('name,form', _wgrad_params())
def test_wgrad_bound(name, form, monkeypatch):
    """Judge 2 on seeded normal operands."""
    cg = _set_form(monkeypatch, form)
    case = WGRAD[name]
    op = _wgrad_random_op(name)
    d = _wgrad_dev(op)
    plan = EW.conv_wgrad_plan(*case, form=form)
    slack_form = form if plan['family'] == 'generic' else 'exact'
    for red, layout, label in _wgrad_routes(case, form):
        S = plan['depth'](red == 'det', bool(layout))
        with _reduction(monkeypatch, red):
            for which, scaled, alpha in (('scaled', True, EW.CF_WGRAD_ALPHA['random']), ('plain', False, 1.0)):
                ref, _, slack = EW.cf_wgrad_ref(case, op, slack_form, S, scaled, alpha)
                dw = _wgrad_call(cg, case, d, scaled, alpha, form, layout)
                what = f'conv_f32 dw {name} {form} {label} {which}'
                r = EW.assert_elementwise(dw, ref, slack, F32, what)
                print(f'elementwise {what}: worst error / bound dw {r:.3g}')


@pytest.mark.parametrize('name,form,kind', _plane_params(EW.CF_PLANE_WGRAD, _wgrad_forms))
def test_wgrad_planes(name, form, kind, monkeypatch):
    """Judge 1 on the plane fixtures (g is the GEMM's A operand, x its B operand)."""
    cg = _set_form(monkeypatch, form)
    case = WGRAD[name]
    A, B, k, stride, pad = case[:5]
    for sparse in ('a', 'b'):
        g, x = EW.cf_plane_wgrad_operands(case, kind, sparse)
        kw = dict(stride=stride, padding=pad)
        terms = torch.nn.grad.conv2d_weight((x != 0).double(), (A, B, k, k), (g != 0).double(), **kw)
        ref = torch.nn.grad.conv2d_weight(x, (A, B, k, k), g, **kw)
        EW.cf_plane_assert_one_term(terms, ref, (name, kind, sparse))
        d = dict(g=_nhwc(g), x=_nhwc(x))
        for red, layout, label in _wgrad_routes(case, form):
            with _reduction(monkeypatch, red):
                dw = _wgrad_call(cg, case, d, False, 1.0, form, layout)
            EW.lb_judge_exact(dict(dw=dw), dict(dw=ref), f'conv_f32 dw planes {name} {form} {kind} sparse {sparse} {label}')


# ------------------------------------------------------------------ sg2_split3
def _bits(t):
    return t.contiguous().view(torch.int16)


def _split3_values(kind, n, g):
    if kind == 'normal':
        return torch.randn(n, generator=g)
    if kind == 'zeros':         # +-0 among normals: a zero splits into (+-0, +0, +0)
        v = torch.randn(n, generator=g)
        v[::3] = 0.0
        v[1::6] = -0.0
        return v
    if kind == 'extreme':       # magnitudes around 2^+-100 with full significands: every residual stays normal
        m = 1 + torch.randint(0, 2 ** 23, (n,), generator=g).double() * 2.0 ** -23
        e = torch.tensor([100.0, 99.0, -100.0, -99.0])[torch.randint(0, 4, (n,), generator=g)].double()
        return (m * 2.0 ** e * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).float()
    # the plane fixtures' three value sets: 24 significant bits, +-2^k, 1 + q 2^-11
    return EW.cf_plane_values(*{'x24': ('x24', 'a'), 'pow2': ('x24', 'b'), 'mm': ('mm', 'a')}[kind], g, n).float()


@pytest.mark.parametrize('kind', ['normal', 'zeros', 'extreme', 'x24', 'pow2', 'mm'])
@pytest.mark.parametrize('layout', ['act', 'act-scaled', 'packed', 'packed-scaled'])
def test_split3(kind, layout):
    """cg.split3: the three planes bitwise EW.s3_split of the f32-rounded product x * scale, in the operand's memory
    order; 735 groups of 8 (two full blocks and a ragged third).  f32 subnormals are out of scope."""
    cg = _cg()
    g = torch.Generator().manual_seed(len(kind) * 131 + len(layout))
    N, C, H, W = 3, 40, 7, 7
    scaled = layout.endswith('scaled') and kind != 'extreme'
    if layout.startswith('act'):
        x = _split3_values(kind, N * C * H * W, g).view(N, C, H, W)
        s = (torch.rand(N, C, generator=g) + 0.5) if scaled else None
        xm = x * s[:, :, None, None] if scaled else x
        flat = xm.permute(0, 2, 3, 1).reshape(-1)
        planes = cg.split3(_nhwc(x), s.to(DEV) if scaled else None)
    else:
        x = _split3_values(kind, N * H * W * C, g).view(N * H, W, C)     # a packed weight [.., C] in its memory order
        s = (torch.rand(N * H * W, C, generator=g) + 0.5) if scaled else None
        xm = x * s.view_as(x) if scaled else x
        flat = xm.reshape(-1)
        planes = cg.split3(x.to(DEV), s.to(DEV) if scaled else None, packed=True)
    ref = torch.stack(EW.s3_split(flat)).bfloat16()
    assert tuple(planes.shape) == (3, flat.numel())
    assert torch.equal(_bits(planes.cpu()), _bits(ref)), f'split3 {kind} {layout}: planes differ bitwise'
    assert torch.equal(ref.double().sum(0), flat.double()), 'h + m + l is not x on this fixture'


def test_split3_grid_stride():
    """More groups than one trip of the grid covers (256 * 64 blocks of 256 lanes), and a ragged last trip."""
    cg = _cg()
    n = 8 * (256 * 64 * 256 + 777)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(n // 8, 8, generator=g, device=DEV)
    planes = cg.split3(x, packed=True)
    ref = torch.stack(EW.s3_split(x.cpu().reshape(-1))).bfloat16()
    assert torch.equal(_bits(planes.cpu()), _bits(ref))
