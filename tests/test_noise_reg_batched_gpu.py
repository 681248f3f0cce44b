"""The batched noise-step kernels (sg2_noise_reg_fwd_batched / _bwd_batched, sg2_noise_normalize_batched;
torch_utils/ops/noise_reg.py) against the batch-1 kernels, bit for bit.

The batched entry points run the batch-1 kernels' device functions with the sample as the grid's y, so the contract is
equality of bits, not a bound: sample b's reg, level means, gradient (assigned and accumulated) and normalised buffers
are what noise_regularizer / noise_regularizer_backward / normalize_noise_ return on that sample's buffers copied into
a batch-1 flat tensor.  The batch-1 kernels themselves are held to float64 in test_noise_reg_gpu.py.

Side sets: a single level (4), two levels (8, 16), the projector fixture's seven buffers, one and several pool tiles
(64, 128), and the 8 x 8-patch pool path (1024).  w_dim 32 and 30 (a padded latent row).  Every torch.empty of the
wrapper (outputs, scratch, the flat gradient) is NaN-poisoned, and the flat tensors carry a guard behind `total`."""
import ctypes

import numpy as np
import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SETS = [[4], [8, 16], [4, 8, 8, 16, 16, 32, 32], [64, 128], [1024]]
BATCHES = [1, 2, 3]
W_DIMS = [32, 30]
GUARD = 64          # floats behind `total` that nothing may write
SENTINEL = 7.25


def _ids(s):
    return 'x'.join(str(r) for r in s)


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.noise_reg'])


def _samples(sizes, B, seed=0):
    """[B][nbuf] float32 numpy buffers: correlated noise with an offset and a scale of its own per sample, so no two
    samples share a mean or a second moment."""
    rng = np.random.RandomState(seed + 31 * len(sizes) + sizes[0])
    out = []
    for b in range(B):
        bufs = []
        for r in sizes:
            v = rng.randn(r, r)
            v = v + 0.5 * np.roll(v, 1, 1) + 0.5 * np.roll(v, 1, 0)
            bufs.append((v * (1.0 + 0.3 * b) + 0.1 * (b + 1)).astype(np.float32))
        out.append(bufs)
    return out


def _w_rows(B, w_dim):
    return torch.arange(B * w_dim, dtype=torch.float32).view(B, w_dim) + 1


def _batched_flat(samples, w_dim):
    from torch_utils.ops import noise_reg
    B, sizes = len(samples), [b.shape[0] for b in samples[0]]
    table, total = noise_reg.make_batched_table(B, w_dim, sizes)
    wp = (w_dim + 3) // 4 * 4
    flat = torch.full([total + GUARD], SENTINEL, dtype=torch.float32)
    flat[:B * wp].view(B, wp)[:, :w_dim] = _w_rows(B, w_dim)
    for k, (off, r) in enumerate(table):
        for b in range(B):
            flat[off + b * r * r:off + (b + 1) * r * r] = torch.from_numpy(samples[b][k]).reshape(-1)
    return flat.to(DEV), table, total


def _single_flat(bufs, w_dim):
    from torch_utils.ops import noise_reg
    table, total = noise_reg.make_table(w_dim, [b.shape[0] for b in bufs])
    flat = torch.full([total], SENTINEL, dtype=torch.float32)
    for (off, r), b in zip(table, bufs):
        flat[off:off + r * r] = torch.from_numpy(b).reshape(-1)
    return flat.to(DEV), table


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _mask(table, B, numel):
    """True where a noise buffer lies."""
    m = torch.zeros([numel], dtype=torch.bool)
    for off, r in table:
        m[off:off + B * r * r] = True
    return m


@pytest.mark.parametrize('w_dim', W_DIMS)
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('sizes', SETS, ids=_ids)
def test_per_sample_bits_equal_batch_1(sizes, B, w_dim):
    from torch_utils.ops import noise_reg
    samples = _samples(sizes, B)
    flat, table, total = _batched_flat(samples, w_dim)
    weights = torch.tensor([3.0, 0.5, 1.75][:B], device=DEV)
    inside = _mask(table, B, flat.numel())

    # forward and the autograd gradient
    x = flat.clone().requires_grad_(True)
    reg, means = noise_reg.noise_regularizer_batched(x, table, B, return_means=True)
    assert reg.shape == (B,) and means.shape == (B, sum(noise_reg.num_levels(r) for r in sizes), 2)
    scratch = reg.grad_fn.saved_tensors[2]
    (reg * weights).sum().backward()
    g = x.grad
    assert torch.isfinite(g).all(), 'every element of the flat gradient is assigned'
    assert not g[~inside.to(DEV)].any(), 'the latent rows, padding and everything behind the buffers take a zero gradient'

    # the raw backward: assign over a poisoned gradient, accumulate over a constant one
    g0 = torch.full_like(flat, float('nan'))
    noise_reg.noise_regularizer_batched_backward(g0, weights, flat, means, scratch, table, B, accumulate=0)
    g1 = torch.full_like(flat, 0.5)
    noise_reg.noise_regularizer_batched_backward(g1, weights, flat, means, scratch, table, B, accumulate=1)
    assert torch.isnan(g0[~inside.to(DEV)]).all() and (g1[~inside.to(DEV)] == 0.5).all(), \
        'the raw backward writes nothing outside the buffers (the guard behind `total` included)'
    assert _same(g0[inside.to(DEV)], g[inside.to(DEV)]), 'the autograd gradient is the assigning launch'

    # the normalisation
    normed = noise_reg.normalize_noise_batched_(flat.clone(), table, B)
    assert _same(normed[~inside.to(DEV)], flat[~inside.to(DEV)]), \
        'the normalisation leaves the latent rows, the padding and the guard untouched'

    for b in range(B):
        one, t1 = _single_flat(samples[b], w_dim)
        y = one.clone().requires_grad_(True)
        reg1, means1 = noise_reg.noise_regularizer(y, t1, return_means=True)
        scratch1 = reg1.grad_fn.saved_tensors[2]
        (reg1 * weights[b]).backward()
        assert _same(reg[b], reg1), f'sample {b}: reg'
        assert _same(means[b], means1), f'sample {b}: means'
        h1 = torch.full_like(one, 0.5)
        noise_reg.noise_regularizer_backward(h1, weights[b].clone(), one, means1, scratch1, t1, accumulate=1)
        n1 = noise_reg.normalize_noise_(one.clone(), t1)
        for (off, r), (off1, _) in zip(table, t1):
            lo, lo1, n = off + b * r * r, off1, r * r
            assert _same(g[lo:lo + n], y.grad[lo1:lo1 + n]), f'sample {b}, R = {r}: gradient (assign)'
            assert _same(g1[lo:lo + n], h1[lo1:lo1 + n]), f'sample {b}, R = {r}: gradient (accumulate)'
            assert _same(normed[lo:lo + n], n1[lo1:lo1 + n]), f'sample {b}, R = {r}: normalised buffer'


@pytest.mark.parametrize('sizes', SETS, ids=_ids)
def test_batch_1_is_the_batch_1_op(sizes):
    """At B = 1 the layout is make_table's and the op returns noise_regularizer's bits on the same flat tensor."""
    from torch_utils.ops import noise_reg
    flat, table, total = _batched_flat(_samples(sizes, 1), 30)
    assert (table, total) == noise_reg.make_table(30, sizes)
    x, y = flat.clone().requires_grad_(True), flat.clone().requires_grad_(True)
    reg, means = noise_reg.noise_regularizer_batched(x, table, 1, return_means=True)
    reg1, means1 = noise_reg.noise_regularizer(y, table, return_means=True)
    (reg.sum() * 2.0).backward()
    (reg1 * 2.0).backward()
    assert _same(reg[0], reg1) and _same(means[0], means1) and _same(x.grad, y.grad)
    assert _same(noise_reg.normalize_noise_batched_(flat.clone(), table, 1), noise_reg.normalize_noise_(flat.clone(), table))


def test_reproducible_bits():
    from torch_utils.ops import noise_reg
    flat, table, _ = _batched_flat(_samples(SETS[2] + [128], 3), 32)

    def run():
        x = flat.clone().requires_grad_(True)
        reg, means = noise_reg.noise_regularizer_batched(x, table, 3, return_means=True)
        reg.sum().backward()
        return reg.detach(), means, x.grad, noise_reg.normalize_noise_batched_(flat.clone(), table, 3)

    for a, b in zip(run(), run()):
        assert _same(a, b)


def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type.name == 'CUDA']


def test_launch_counts_do_not_grow_with_the_batch():
    """B = 3, seven buffers: 3 kernels forward, 1 backward, 1 for the normalisation (the sample is a grid dimension)."""
    from torch_utils.ops import noise_reg
    flat, table, _ = _batched_flat(_samples(SETS[2], 3), 32)
    x = flat.clone().requires_grad_(True)
    noise_reg.noise_regularizer_batched(x, table, 3).sum().backward()        # warm-up: library load, allocator
    noise_reg.normalize_noise_batched_(flat.clone(), table, 3)
    x.grad = None
    out = []
    fwd = _device_events(lambda: out.append(noise_reg.noise_regularizer_batched(x, table, 3)))
    loss = out[0].sum()
    bwd = _device_events(loss.backward)
    work = flat.clone()
    nrm = _device_events(lambda: noise_reg.normalize_noise_batched_(work, table, 3))
    print(f'forward {fwd}\nbackward {bwd}\nnormalize {nrm}')
    assert sum('nr_' in n for n in fwd) == 3 and all('batched' in n for n in fwd if 'nr_' in n)
    assert sum('nr_' in n for n in bwd) == 1 and any('nr_bwd_batched' in n for n in bwd)
    assert [('nr_normalize_batched' in n) for n in nrm] == [True]
    assert not [n for n in fwd + bwd + nrm if 'memset' in n.lower()]


def test_second_order_is_refused():
    from torch_utils.ops import noise_reg
    flat, table, _ = _batched_flat(_samples([16], 2), 32)
    x = flat.clone().requires_grad_(True)
    reg = noise_reg.noise_regularizer_batched(x, table, 2)
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(reg.sum(), x, create_graph=True)


@pytest.mark.parametrize('B', [0, 65])
def test_batch_out_of_range_is_an_argument_error(B):
    import sg2hip
    from torch_utils.ops import noise_reg
    flat, table, _ = _batched_flat(_samples([8], 1), 32)
    with pytest.raises(RuntimeError, match='B must be in 1..64'):
        noise_reg.noise_regularizer_batched(flat, table, B)
    with pytest.raises(RuntimeError, match='B must be in 1..64'):
        noise_reg.normalize_noise_batched_(flat, table, B)
    L, before = sg2hip.lib(), flat.clone()
    ct = sg2hip.i64arr([v for row in table for v in row])
    nbytes, p, s = ctypes.c_int64(-1), sg2hip.ptr(flat), sg2hip.stream_ptr(flat.device)
    for rc in (L.sg2_noise_reg_batched_scratch_bytes(ctypes.byref(nbytes), ct, 1, B),
               L.sg2_noise_reg_fwd_batched(p, p, p, ct, 1, B, p, s),
               L.sg2_noise_reg_bwd_batched(p, p, p, p, ct, 1, B, p, 0, s),
               L.sg2_noise_normalize_batched(p, ct, 1, B, s)):
        assert rc != 0 and b'B must be in 1..64' in L.sg2_last_error()
    assert _same(flat, before), 'no device work'
