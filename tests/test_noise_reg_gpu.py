"""The projector's fused noise-step kernels (sg2_noise_reg_fwd / _bwd, sg2_noise_normalize_multi;
torch_utils/ops/noise_reg.py) against a float64 numpy restatement of the reference's arithmetic
(SG3/genlib/projector/projector.py:259-268, :294-298).

Buffer sets: R below the stop size (4), the stop boundary (8), one pool (16), seven buffers of mixed size, a multi-tile
level whose circular shift crosses tile and chunk borders (128), six levels over several tiles (256, 256), and the
largest size, which takes the pool kernel's 8 x 8-patch variant for every buffer of the call (16, 1024).

Bounds.  Value and per-buffer gradient: relative L2 error <= 2e-6 on correlated noise (every level mean well away from
zero) -- ten times what torch's own float32 composition shows against float64 on such inputs on a CPU (2.6e-7 on the
value, 1.9e-7 on the gradient when the bound was set; 1.3e-7 and 1.4e-7 with the seeds used here); the factor leaves
room for another summation order.  Measured on the MI355X: value <= 1.9e-7, gradient <= 9.8e-8.  Level means on white noise (means
near zero, so a relative bound has no meaning): within 64 * 2^-24 * mean|n roll n| of float64, the bound of a tree
reduction with serial runs of up to ~32 terms (torch's float32 composition uses 2 % of it).  normalize_noise_: 2e-6
relative L2, same reasoning (torch float32 on a CPU: 6.3e-8 at these sizes; the kernel: 6.2e-8)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SETS = [[4], [8], [16], [4, 8, 8, 16, 16, 32, 32], [128], [256, 256], [16, 1024]]
HEAD = 10           # a head that is no multiple of 4: make_table pads it
TOL = 2e-6


def _ids(s):
    return 'x'.join(str(r) for r in s)


def _inputs(sizes, correlated, seed=0):
    """float32 numpy buffers; correlated: v + 0.5 roll_x v + 0.5 roll_y v, renormalised."""
    rng = np.random.RandomState(seed + 17 * len(sizes) + sizes[0])
    out = []
    for r in sizes:
        v = rng.randn(r, r)
        if correlated:
            v = v + 0.5 * np.roll(v, 1, 1) + 0.5 * np.roll(v, 1, 0)
            v = v - v.mean()
            v = v / np.sqrt((v * v).mean())
        out.append(v.astype(np.float32))
    return out


def _pyramid64(buf):
    lv = [buf.astype(np.float64)]
    while lv[-1].shape[0] > 8:
        a = lv[-1]
        s = a.shape[0] // 2
        lv.append(a.reshape(s, 2, s, 2).mean(axis=(1, 3)))
    return lv


def _ref64(bufs):
    """value, per-buffer gradients, per-level (mx, my) and per-level (mean|n roll_x n|, mean|n roll_y n|)."""
    value, grads, means, mags = 0.0, [], [], []
    for buf in bufs:
        lv = _pyramid64(buf)
        g = np.zeros_like(lv[0])
        for l, a in enumerate(lv):
            px, py = a * np.roll(a, 1, 1), a * np.roll(a, 1, 0)
            mx, my = px.mean(), py.mean()
            value += mx * mx + my * my
            means.append((mx, my))
            mags.append((np.abs(px).mean(), np.abs(py).mean()))
            ga = (2 * mx * (np.roll(a, 1, 1) + np.roll(a, -1, 1)) + 2 * my * (np.roll(a, 1, 0) + np.roll(a, -1, 0))) / a.size
            g += np.kron(ga, np.ones((2 ** l, 2 ** l))) / 4 ** l
        grads.append(g)
    return value, grads, np.array(means), np.array(mags)


def _flat(bufs):
    from torch_utils.ops import noise_reg
    table, total = noise_reg.make_table(HEAD, [b.shape[0] for b in bufs])
    flat = torch.zeros([total], dtype=torch.float32)
    flat[:HEAD] = torch.arange(HEAD, dtype=torch.float32)
    for (off, r), b in zip(table, bufs):
        flat[off:off + r * r] = torch.from_numpy(b).reshape(-1)
    return flat.to(DEV), table


def _rel(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _run(flat, table, weight=1.0):
    from torch_utils.ops import noise_reg
    x = flat.clone().requires_grad_(True)
    reg, means = noise_reg.noise_regularizer(x, table, return_means=True)
    (reg * weight).backward()
    return reg.detach(), means, x.grad


@pytest.mark.parametrize('sizes', SETS, ids=_ids)
def test_value_and_gradient(sizes):
    bufs = _inputs(sizes, correlated=True)
    value, grads, means64, _ = _ref64(bufs)
    flat, table = _flat(bufs)
    reg, means, g = _run(flat, table, weight=3.0)
    err = abs(float(reg) - value) / value
    print(f'{_ids(sizes)}: value rel err {err:.3g}')
    g = g.cpu().numpy()
    errs = [_rel(g[o:o + r * r], 3.0 * gr) for (o, r), gr in zip(table, grads)]
    print(f'{_ids(sizes)}: gradient rel L2 {max(errs):.3g}')
    assert means.shape == means64.shape
    assert err <= TOL
    assert max(errs) <= TOL
    assert np.array_equal(g[:table[0][0]], np.zeros(table[0][0], np.float32)), 'the head has no gradient'


@pytest.mark.parametrize('sizes', SETS, ids=_ids)
def test_level_means_on_white_noise(sizes):
    bufs = _inputs(sizes, correlated=False, seed=5)
    _, _, means64, mags = _ref64(bufs)
    flat, table = _flat(bufs)
    _, means, _ = _run(flat, table)
    used = np.abs(means.cpu().numpy().astype(np.float64) - means64) / (64 * 2.0 ** -24 * mags)
    print(f'{_ids(sizes)}: worst level mean uses {used.max():.3g} of the bound')
    assert used.max() <= 1.0


def test_reproducible_bits():
    bufs = _inputs(SETS[3], correlated=True) + _inputs([256], correlated=True)
    flat, table = _flat(bufs)
    a, b = _run(flat, table), _run(flat, table)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_accumulate_and_assign():
    from torch_utils.ops import noise_reg
    bufs = _inputs(SETS[3], correlated=True)
    _, grads, _, _ = _ref64(bufs)
    flat, table = _flat(bufs)
    fn = noise_reg._NoiseReg
    x = flat.clone().requires_grad_(True)
    reg, means = fn.apply(x, table)
    scratch = reg.grad_fn.saved_tensors[2]
    greg = torch.full([], 2.0, device=DEV)
    g0 = torch.full_like(flat, float('nan'))
    noise_reg.noise_regularizer_backward(g0, greg, flat, means, scratch, table, accumulate=0)
    g1 = torch.full_like(flat, 0.5)
    noise_reg.noise_regularizer_backward(g1, greg, flat, means, scratch, table, accumulate=1)
    g0, g1 = g0.cpu().numpy(), g1.cpu().numpy()
    for (o, r), gr in zip(table, grads):
        assert np.isfinite(g0[o:o + r * r]).all(), 'accumulate=0 must overwrite every element of every buffer'
        assert _rel(g0[o:o + r * r], 2.0 * gr) <= TOL
        # (one rounding of difference: the add may be contracted into the multiply by greg)
        assert np.abs(g1[o:o + r * r] - (g0[o:o + r * r] + np.float32(0.5))).max() <= 2.0 ** -23
    assert np.isnan(g0[:table[0][0]]).all() and (g1[:table[0][0]] == 0.5).all(), 'the head is not the kernel\'s'


def test_second_order_is_refused():
    bufs = _inputs([16], correlated=True)
    flat, table = _flat(bufs)
    from torch_utils.ops import noise_reg
    x = flat.clone().requires_grad_(True)
    reg = noise_reg.noise_regularizer(x, table)
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(reg, x, create_graph=True)


def test_launch_count():
    """Forward + backward of the seven-buffer set: at most 8 device kernels, no memset (the reference's composition
    issues several hundred)."""
    from torch.profiler import ProfilerActivity, profile
    flat, table = _flat(_inputs(SETS[3], correlated=True))
    _run(flat, table)                    # warm-up: library load, allocator
    torch.cuda.synchronize()
    x = flat.clone().requires_grad_(True)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        from torch_utils.ops import noise_reg
        noise_reg.noise_regularizer(x, table).backward()
        torch.cuda.synchronize()
    dev = [e.name for e in prof.events() if e.device_type.name == 'CUDA']
    print(f'{len(dev)} device events: {dev}')
    assert 1 <= len(dev) <= 8
    assert not [n for n in dev if 'memset' in n.lower()]
    assert sum('nr_' in n for n in dev) == 4, 'pool, corr, finalize, backward'


def _normalize64(b):
    b = b.astype(np.float64)
    b = b - b.mean()
    return b / np.sqrt((b * b).mean())


def test_normalize_noise():
    from torch_utils.ops import noise_reg
    from torch.profiler import ProfilerActivity, profile
    rng = np.random.RandomState(3)
    bufs = [(rng.randn(r, r) * 1.7 + 0.3).astype(np.float32) for r in (4, 8, 32, 256)]
    flat, table = _flat(bufs)
    noise_reg.normalize_noise_(flat.clone(), table)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        noise_reg.normalize_noise_(flat, table)
        torch.cuda.synchronize()
    dev = [e.name for e in prof.events() if e.device_type.name == 'CUDA']
    assert len(dev) == 1, dev
    got = flat.cpu().numpy()
    assert np.array_equal(got[:HEAD], np.arange(HEAD, dtype=np.float32)), 'the head is untouched'
    for (o, r), b in zip(table, bufs):
        err = _rel(got[o:o + r * r].reshape(r, r), _normalize64(b))
        print(f'normalize R={r}: rel L2 {err:.3g}')
        assert err <= TOL


def test_normalize_constant_buffer():
    """A constant buffer: x - mean = 0 and 0 * rsqrt(0) is NaN, in torch's composition and in the kernel."""
    from torch_utils.ops import noise_reg
    bufs = [np.full((8, 8), 0.5, np.float32), _inputs([16], correlated=False)[0]]
    want = [torch.from_numpy(b.copy()) for b in bufs]
    noise_reg.normalize_noise_ref_(want)
    flat, table = _flat(bufs)
    got = noise_reg.normalize_noise_(flat, table).cpu()
    (o0, r0), (o1, r1) = table
    assert torch.isnan(want[0]).all() and torch.isnan(got[o0:o0 + r0 * r0]).all()
    assert torch.isfinite(got[o1:o1 + r1 * r1]).all()


def test_unflatten_gradient_is_one_flat_tensor():
    from torch_utils.ops import noise_reg
    flat, table = _flat(_inputs([8, 16], correlated=False))
    x = flat.clone().requires_grad_(True)
    head, views = noise_reg.unflatten(x, table, head=HEAD)
    assert head.shape == (HEAD,) and [tuple(v.shape) for v in views] == [(8, 8), (16, 16)]
    assert views[1].data_ptr() == x.data_ptr() + 4 * table[1][0], 'views share the flat storage'
    (head.sum() * 2.0 + (views[1] * 3.0).sum()).backward()      # views[0] gets no gradient
    g = x.grad.cpu()
    want = torch.zeros_like(g)
    want[:HEAD] = 2.0
    want[table[1][0]:] = 3.0
    assert torch.equal(g, want)


def test_unsupported_table_is_an_error():
    from torch_utils.ops import noise_reg
    flat = torch.zeros([64], device=DEV)
    assert not noise_reg.supported(((0, 6),)) and not noise_reg.supported(((2, 4),))
    with pytest.raises(RuntimeError, match='power of two'):
        noise_reg.noise_regularizer(flat, ((0, 6),))
