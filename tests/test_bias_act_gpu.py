"""sg2_bias_act (csrc/bias_act.hip, wrapper torch_utils/ops/bias_act.py): the forward and both gradient orders, every
element against CPU float64 of the operands the kernel reads (elementwise.bias_act_ref) -- never autograd of clamp, never
a product wrapper.  Every torch.empty / empty_like of the wrapper comes back NaN-filled, so an element the kernel
leaves unwritten fails.

Judge 1 (test_exact): linear, relu and lrelu at alpha 0.25, gain 2, clamp 2.5 and none, on x and b in halves and dy in
small integers: every value is a bf16, fp16 and f32 value and y == 0 and |y| == clamp are frequent; the forward and dx
are held BITWISE in all three types on every case family.
Judge 2 (test_bound, test_shapes, test_second_sweep): all nine activations x {f32, fp16, bf16} x grad {0, 1, and 2
where the activation has a second-order term}, random operands rounded to the type, gain in {default, 0.7} and clamp
in {None, 0.9, 256}: |got - ref| <= u |ref| + (1 + u) slack + tiny per element, slack derived from the kernel's f32
operations (bias_act_ref's docstring).  The model's three documented constants: __expf (2 |x| + 4) 2^-24 relative
(twice the hardware exp2's specified 1 ulp, plus the rounded log2e product and constant) and 2^-126 for a flushed
result; tanhf 5 ulp and log1pf 2 ulp of 2^-23 (OCML at the OpenCL full-profile limits).  None is fitted to a run.

The gradient kernels are driven with a y the TEST supplies -- the rounded float64 forward with 0, -0, +-clamp, one ulp
either side of it and NaN written over its first and last elements -- through bias_act_grad(dy, y) for the activations
expressed through y and through Grad.apply(dy, x, b, y) for swish; grad 2 through autograd of that Grad op.  The kernel
then is a pure function of what the reference sees and no forward tie can leak in.

Case families (elementwise.BA_CASES): numel < V; full vectors plus a tail of V - 1 with C coprime to V, both layouts;
no tail; dim 0, 2, 3 in both layouts; 2-D, 3-D, 5-D; C = 1; (N, C, 1, 1); no bias; a 16-byte misaligned x, dy and y;
a strided x; an expanded dy; and the second trip of the grid-stride loop (1,048,576 V elements a sweep) in all three
types.  test_bias_act_host.py plants each fault these must see into each family's reference and asserts that it lands.

Autograd wiring (test_wiring_*): bias_act -> grad -> grad hands the kernels the right tensors: gx bitwise the direct
Grad op, gb and the second-order d_b within u |ref| + gamma(K) A of the float64 sum, d_dy (the R1 path) bitwise the
Grad op on v, d_x bitwise the grad-2 launch; None where the activation has no second-order term.

Worst error / bound of Judge 2 on an MI355X over test_bound's gains, clamps and layouts (each test prints its own;
a 16-bit output sits at its own rounding, the f32 column is the f32 model alone):
    activation   grad 0: f32 fp16 bf16      grad 1: f32 fp16 bf16      grad 2: f32 fp16 bf16
    linear       0.77  0.994 0.996          0.88  0.977 0.988
    relu         0.77  0.984 0.885          0.866 0.943 0.988
    lrelu        0.77  0.984 0.955          0.866 0.943 0.988
    tanh         0.146 0.968 0.897          0.509 0.952 0.978          0.459 0.928 0.972
    sigmoid      0.505 0.949 0.968          0.394 0.93  0.968          0.306 0.904 0.968
    elu          0.77  0.994 0.996          0.863 0.969 0.988          0.431 0.92  0.949
    selu         0.728 0.962 0.946          0.66  0.963 0.932          0.38  0.959 0.926
    softplus     0.296 0.948 0.98           0.37  0.99  0.958          0.205 0.959 0.948
    swish        0.456 0.97  0.912          0.225 0.955 0.946          0.198 0.923 0.94
"""
import pytest
import torch

import elementwise as EW
import poison

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CL = torch.channels_last
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAME = {F16: 'fp16', BF16: 'bf16', F32: 'f32'}
DTYPES = [F32, F16, BF16]
IDS = list(NAME[d] for d in DTYPES)


@pytest.fixture(autouse=True)
def _poisoned_empties(monkeypatch):
    """An output element the kernel leaves unwritten is NaN and fails every judge."""
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.bias_act'])


# ------------------------------------------------------------------ operands on the device
def _dev(t, dtype, cl=False, view=None):
    """A float64 operand as the device tensor of a case: dense in its layout, or one of the views."""
    if t is None:
        return None
    t = t.to(dtype)
    if view == 'mis':           # a flat buffer sliced from element 1: data_ptr() % 16 != 0
        buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 != 0 and out.is_contiguous()
        return out
    if view == 'strided':       # base[:, :, ::2]
        shape = list(t.shape)
        shape[2] *= 2
        out = torch.zeros(shape, dtype=dtype, device=DEV)[:, :, ::2]
        out.copy_(t)
        assert not out.is_contiguous()
        return out
    if view == 'expanded':
        assert bool((t == 1).all())
        return torch.ones((), dtype=dtype, device=DEV).expand(t.shape)
    t = t.to(DEV)
    return t.contiguous(memory_format=CL) if cl and t.dim() == 4 else t.contiguous()


def _operands(op, cl, view):
    dt = op['dtype']
    return dict(x=_dev(op['x'], dt, cl, {'mis_x': 'mis', 'strided_x': 'strided'}.get(view)),
                b=_dev(op['b'], dt),
                dy=_dev(op['dy'], dt, cl, {'mis_dy': 'mis', 'expanded_dy': 'expanded'}.get(view)),
                y=_dev(op['y'], dt, cl, {'mis_y': 'mis'}.get(view)),
                v=_dev(op['v'], dt, cl))


def _fixture(family, dtype, act, gain=None, clamp=None, alpha=None, exact=False):
    shape, dim, cl, bias, view = EW.BA_CASES[family]
    op = EW.ba_fixture(shape, dim, bias, dtype, act, gain=gain, clamp=clamp, alpha=alpha, exact=exact, plant=not exact)
    if view == 'expanded_dy':
        op['dy'] = torch.ones_like(op['dy'])
    return op, _operands(op, cl, view), cl


# ------------------------------------------------------------------ drivers
def _scalars(op):
    """alpha, gain, clamp as bias_act() hands them to the kernel."""
    kw = op['kw']
    spec = EW.BA_SPEC[op['act']]
    return (float(spec[0] if kw['alpha'] is None else kw['alpha']), float(spec[1] if kw['gain'] is None else kw['gain']),
            float(kw['clamp'] if kw['clamp'] is not None else -1))


def _fn(op):
    from torch_utils.ops import bias_act
    return bias_act._bias_act_fn(op['dim'], op['act'], *_scalars(op))


def _fwd(op, d):
    from torch_utils.ops import bias_act
    kw = op['kw']
    return bias_act.bias_act(d['x'], d['b'], dim=op['dim'], act=op['act'], alpha=kw['alpha'], gain=kw['gain'],
                             clamp=kw['clamp'])


def _grad1(op, d, g='dy'):
    """The first-order kernel on the gradient d[g]: the public bias_act_grad(dy, y) for an activation expressed
    through y (or nothing), Grad.apply(dy, x, b, y) for swish."""
    from torch_utils.ops import bias_act
    kw = op['kw']
    if EW.BA_SPEC[op['act']][2] == 'x':
        return _fn(op).Grad.apply(d[g], d['x'], d['b'], d['y'])
    return bias_act.bias_act_grad(d[g], d['y'], act=op['act'], alpha=kw['alpha'], gain=kw['gain'], clamp=kw['clamp'],
                                  dim=op['dim'])


def _grad2(op, d):
    """The second-order kernel through autograd of the Grad op -> (d_x, d_b or None)."""
    x = d['x'].detach().requires_grad_(True)
    b = d['b'].detach().requires_grad_(True) if d['b'] is not None else None
    dx = _fn(op).Grad.apply(d['dy'], x, b, d['y'])
    got = torch.autograd.grad(dx, [x] + ([b] if b is not None else []), d['v'])
    return got[0], (got[1] if b is not None else None)


def _judge(got, ref, slack, op, grad, what, cl=False, table=None):
    dtype = op['dtype']
    assert got.dtype == dtype and got.device.type == 'cuda', what
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(slack).all()), f'{what}: the reference is not finite'
    if got.dim() == 4:
        assert got.is_contiguous(memory_format=CL if cl else torch.contiguous_format), what
    r = EW.assert_elementwise(got, ref, slack, dtype, what)
    if table is not None:
        key = (op['act'], grad, NAME[dtype])
        table[key] = max(table.get(key, 0.0), r)
    return r


def _run_grads(op, d, cl, what, grads, table=None):
    """The forward, grad 1 and grad 2 of one fixture under Judge 2."""
    for grad in grads:
        ref, slack = EW.ba_ref(op, grad)
        got = _fwd(op, d) if grad == 0 else _grad1(op, d) if grad == 1 else _grad2(op, d)[0]
        _judge(got, ref, slack, op, grad, f'{what} grad {grad}', cl, table)


def _grads_of(act):
    return (0, 1, 2) if EW.BA_SPEC[act][3] else (0, 1)


# ------------------------------------------------------------------ Judge 1
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('act', ['linear', 'relu', 'lrelu'])
def test_exact(act, dtype):
    """The forward and dx bitwise the float64 reference on the exact grid, on every case family, with clamp 2.5
    (|y| == clamp masked, strictly) and without."""
    for family in EW.BA_CASES:
        for clamp in (EW.BA_EXACT['clamp'], None):
            op, d, cl = _fixture(family, dtype, act, gain=EW.BA_EXACT['gain'], clamp=clamp, alpha=EW.BA_EXACT['alpha'],
                                 exact=True)
            what = f'{act} {family} clamp {clamp}'
            y, dx = _fwd(op, d), _grad1(op, d)
            assert y.dtype == dtype and dx.dtype == dtype
            EW.lb_judge_exact(dict(y=y, dx=dx), dict(y=EW.ba_ref(op, 0)[0], dx=EW.ba_ref(op, 1)[0]), what)


# ------------------------------------------------------------------ Judge 2
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('act', list(EW.BA_SPEC))
def test_bound(act, dtype):
    """Every activation, type and gradient order at gain in {default, 0.7} and clamp in {None, 0.9, 256}, both
    layouts (315 elements: full vectors and a tail of 3)."""
    mine = {}
    for family in ('bound', 'bound_cl'):
        for gain in EW.BA_GAINS:
            for clamp in EW.BA_CLAMPS:
                op, d, cl = _fixture(family, dtype, act, gain=gain, clamp=clamp)
                _run_grads(op, d, cl, f'{act} {family} gain {gain} clamp {clamp}', _grads_of(act), mine)
    print('\n' + EW.ba_report(mine))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('family', [f for f in EW.BA_CASES if not f.startswith('bound')])
def test_shapes(family, dtype):
    """Every case family, forward and grad 1 (and swish's grad 2): lrelu with clamp 256 (y holds +-256, its
    neighbours, 0 and NaN at both ends, so in the tail vector too) and swish with clamp 0.9 (the gradient kernels
    read x and b there, so the bias index is live at every order, and the mask is the recomputed one)."""
    for act, clamp in (('lrelu', 256.0), ('swish', 0.9)):
        op, d, cl = _fixture(family, dtype, act, clamp=clamp)
        _run_grads(op, d, cl, f'{act} {family}', _grads_of(act))


@pytest.mark.parametrize('extra', [0, 1], ids=['tail', 'plus1'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_second_sweep(dtype, extra):
    """The grid is capped at 4096 workgroups of 256 lanes: past 1,048,576 vectors a lane takes a second trip.  numel =
    1,048,576 V + 3 256 V + (V - 1) and 1,048,576 V + 1 as a 2-D [R, C] with a live bias: lrelu forward and grad 1
    (clamp 256, y planted at both ends), tanh at grad 2."""
    shape = EW.ba_sweep_shape(dtype, EW.ba_sweep_extras(dtype)[extra])
    op = EW.ba_fixture(shape, 1, True, dtype, 'lrelu', clamp=256.0)
    d = _operands(op, False, None)
    _run_grads(op, d, False, f'lrelu {shape}', (0, 1))
    # the same operands under tanh: its own rounded forward as y
    op = dict(op, act='tanh', kw=dict(op['kw'], clamp=None))
    op['y'] = EW.rnd(EW.ba_ref(op, 0)[0], dtype)
    d['y'] = _dev(op['y'], dtype)
    _run_grads(op, d, False, f'tanh {shape}', (2,))


# ------------------------------------------------------------------ the non-finite table on the device
def _same(got, want, dtype):
    g, w = got.double().cpu().flatten(), EW.rnd(torch.tensor(want, dtype=torch.float64), dtype)
    return torch.equal(g.isnan(), w.isnan()) and torch.equal(g.nan_to_num(0.0, 7e77, -7e77), w.nan_to_num(0.0, 7e77, -7e77))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_nonfinite_and_edge_table(dtype):
    from torch_utils.ops import bias_act
    x = torch.tensor([EW.NAN, EW.INF, -EW.INF], dtype=dtype, device=DEV)
    for act, (clamped, free) in EW.BA_FWD_NONFINITE.items():
        for clamp, want in ((2.5, clamped), (None, free)):
            got = bias_act.bias_act(x, act=act, alpha=0.25, gain=2.0, clamp=clamp)
            assert _same(got, want, dtype), (act, clamp, got.tolist())
    y = torch.tensor(EW.BA_EDGE_Y[dtype], dtype=dtype, device=DEV)
    assert y.double().cpu().nan_to_num(9.0).tolist() == torch.tensor(EW.BA_EDGE_Y[dtype]).double().nan_to_num(9.0).tolist()
    for clamp, want in ((2.5, EW.BA_EDGE_DX), (None, EW.BA_EDGE_DX_FREE)):
        got = bias_act.bias_act_grad(torch.ones_like(y), y, act='lrelu', clamp=clamp, **EW.BA_EDGE_KW)
        assert _same(got, want, dtype), (clamp, got.tolist())
    # the mask assigns: a NaN gradient under a masked y is 0
    got = bias_act.bias_act_grad(torch.full_like(y, EW.NAN), y, act='lrelu', clamp=2.5, **EW.BA_EDGE_KW)
    assert _same(got, [EW.NAN, EW.NAN, 0.0, 0.0, EW.NAN, EW.NAN, 0.0, 0.0, 0.0], dtype), got.tolist()


# ------------------------------------------------------------------ the autograd wiring
def _saved(op, d):
    """(x, b, y) as BiasAct saves them for its Grad op."""
    spec = EW.BA_SPEC[op['act']]
    keep_x = 'x' in spec[2] or spec[3]
    keep_y = 'y' in spec[2] or op['kw']['clamp'] is not None
    return (d['x'] if keep_x else None, d['b'] if keep_x else None, d['y'] if keep_y else None)


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    assert bool((err <= bound).all()), f'{what}: {float((err / bound).max()):.3g} x the bound'


def _wire(op, cl):
    """y = bias_act(x, b); gx, gb = grad(y, [x, b], dy, create_graph) -> everything the checks below need."""
    dt = op['dtype']
    d = _operands(op, cl, None)
    x, b, dy = (d[k].detach().requires_grad_(True) for k in ('x', 'b', 'dy'))
    y = _fwd(op, dict(d, x=x, b=b))
    gx, gb = torch.autograd.grad(y, [x, b], dy, create_graph=True)
    d = dict(d, y=y.detach())
    sx, sb, sy = _saved(op, d)
    assert torch.equal(gx, _fn(op).Grad.apply(d['dy'], sx, sb, sy)), 'gx is not the Grad op on (dy, saved x, b, y)'
    # the reference reads what the kernel read: the device's own y
    o = dict(op, y=y.detach().double().cpu())
    dims = [i for i in range(x.dim()) if i != op['dim']]
    ref, slack = EW.ba_ref(o, 1)
    EW.assert_elementwise(gx, ref, slack, dt, 'gx')
    want, bound = EW.ba_sum_bound(ref, slack, dims, dt)
    _within(gb, want, bound, 'gb')
    assert gb.dtype == dt and gb.shape == b.shape
    return d, o, x, b, dy, gx, dims


@pytest.mark.parametrize('dtype', [F32, F16], ids=['f32', 'fp16'])
@pytest.mark.parametrize('act,clamp', EW.BA_WIRING, ids=[a for a, _ in EW.BA_WIRING])
def test_wiring_second_order(act, clamp, dtype):
    """An activation with a second-order term, both layouts, dim 1 and 2: d_dy bitwise the Grad op on v, d_x bitwise
    the grad-2 launch, d_b its sum.  The fixture keeps every sum one-signed and every stored element off a rounding
    tie (elementwise.ba_wiring_fixture), so in fp16 y and gx ARE the rounded reference, bitwise."""
    from torch_utils.ops import bias_act
    for cl in (False, True):
        for dim in (1, 2):
            op = EW.ba_wiring_fixture(act, clamp, dtype, dim)
            d, o, x, b, dy, gx, dims = _wire(op, cl)
            if dtype != F32:
                assert torch.equal(d['y'].double().cpu(), op['y']), 'y is not the rounded reference'
                assert torch.equal(gx.double().cpu(), EW.rnd(EW.ba_ref(o, 1)[0], dtype))
            d_dy, d_x, d_b = torch.autograd.grad(gx, [dy, x, b], d['v'])
            sx, sb, sy = _saved(op, d)
            assert torch.equal(d_dy, _fn(op).Grad.apply(d['v'], sx, sb, sy)), 'd_dy is not the Grad op on v'
            direct = bias_act._launch(d['v'], d['b'], d['x'], sy, d['dy'], 2, dim, bias_act.activation_funcs[act],
                                      *_scalars(op))
            assert torch.equal(d_x, direct), 'd_x is not the grad-2 launch'
            ref, slack = EW.ba_ref(o, 2)
            EW.assert_elementwise(d_x, ref, slack, dtype, 'd_x')
            want, bound = EW.ba_sum_bound(ref, slack, dims, dtype)
            _within(d_b, want, bound, f'{act} d_b dim {dim}')
            ref, slack = EW.ba_ref(o, 1, dy=op['v'])
            EW.assert_elementwise(d_dy, ref, slack, dtype, 'd_dy')


@pytest.mark.parametrize('dtype', [F32, F16], ids=['f32', 'fp16'])
@pytest.mark.parametrize('act,clamp', [('relu', None), ('lrelu', 2.5), ('linear', 2.5)], ids=['relu', 'lrelu', 'linear'])
def test_wiring_r1_path(act, clamp, dtype):
    """relu, lrelu and linear with a clamp on the exact grid: d_dy = Grad.apply(d_dx, x, b, y) is present and bitwise
    the reference; the Grad op returns None for d_x and d_b."""
    for cl in (False, True):
        for dim in (1, 2):
            op = EW.ba_fixture(EW.BA_WIRING_SHAPE, dim, True, dtype, act, gain=EW.BA_EXACT['gain'], clamp=clamp,
                               alpha=EW.BA_EXACT['alpha'], exact=True, plant=False)
            d, o, x, b, dy, gx, dims = _wire(op, cl)
            assert torch.equal(d['y'].double().cpu(), op['y'])
            EW.lb_judge_exact(dict(gx=gx), dict(gx=EW.ba_ref(op, 1)[0]), f'{act} gx')
            d_dy, d_x, d_b = torch.autograd.grad(gx, [dy, x, b], d['v'], allow_unused=True)
            EW.lb_judge_exact(dict(d_dy=d_dy), dict(d_dy=EW.ba_ref(op, 1, dy=op['v'])[0]), f'{act} d_dy')
            # x and b reach gx only through the saved y, whose gradient the Grad op leaves undefined: autograd hands
            # BiasAct.backward zeros for it, so through the whole graph d_x and d_b are None or exactly zero
            for t in (d_x, d_b):
                assert t is None or not bool(t.any())
            # at the Grad op itself, with x and b as its own inputs: None
            xr, br, dyr = (d[k].detach().requires_grad_(True) for k in ('x', 'b', 'dy'))
            g = _fn(op).Grad.apply(dyr, xr, br, d['y'])
            assert torch.equal(g, gx)
            e_dy, e_x, e_b = torch.autograd.grad(g, [dyr, xr, br], d['v'], allow_unused=True)
            assert e_x is None and e_b is None and torch.equal(e_dy, d_dy)


def test_trivial_and_empty():
    from torch_utils.ops import bias_act
    x = torch.randn(2, 5, 3, 3, device=DEV, requires_grad=True)
    y = bias_act.bias_act(x)                        # linear, gain 1, no clamp, no bias: x itself
    assert y.data_ptr() == x.data_ptr() and torch.equal(y, x)
    dy = torch.randn_like(x)
    gx, = torch.autograd.grad(y, [x], dy)
    assert torch.equal(gx, dy)
    for dtype in DTYPES:
        e = torch.zeros(0, 5, 3, 3, device=DEV, dtype=dtype)
        b = torch.zeros(5, device=DEV, dtype=dtype)
        for act in ('linear', 'lrelu', 'swish'):
            out = bias_act.bias_act(e, b, act=act, clamp=0.9)
            assert out.shape == e.shape and out.dtype == dtype
            assert bias_act.bias_act(e, act=act).shape == e.shape
    torch.cuda.synchronize()
