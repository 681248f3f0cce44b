"""The per-sample projection-loss kernels on the GPU (csrc/proj_loss.hip through torch_utils/ops/proj_loss.py), against
the torch composition (proj_loss.prep_ref / sqdist_rows_ref) in float64 on the CPU.  Every torch.empty of the wrapper
(outputs, scratch, gradients) is NaN-poisoned.  u = 2^-24 (half an ulp), eps = 2 u.

prep, C in {1, 2, 3} x H in {4, 8, 32} and (C, H) = (1, 512) (f = 2), B in {1, 3}:

  det_in, f = 1: bitwise the f32 torch composition (synth + 1) * (255 / 2) and the split, on the device.
  det_in, f = 2: the kernel rounds s = (x + 1) * 127.5 per element (2 roundings: relative 2 u), adds the four s of a
    window one after another (3 additions, each at most u times the running sum <= sum |s|) and scales by 1/4
    (exact).  torch's area interpolation adds the same four f32 values in an order of its own, so the two f32 results
    differ by roundings taken in a different order, not by arithmetic; against float64 the kernel is within
    (2 + 3) u sum|s| / 4 = 2.5 eps mean|s| -- a few ulp of the result.
  pix[b][m] = (sum_i d_i^2) / n, d = t - s.  Per term: s carries 2 u |s|, the subtraction u |d|, so d is off by
    u |d| + 2 u |s| and d^2 by 2 |d| (u |d| + 2 u |s|), the square adds u d^2: 3 u d^2 + 4 u |d| |s|.  The tree adds
    f^2 terms serially per accumulator, then 2 + 6 + 2 levels in the workgroup, 1 + 6 + 2 over the partials, and one
    division: D = f^2 + 20 roundings, each at most u times the sum of the (non-negative) terms.  Together
    |pix - pix64| <= u ((D + 3) sum d^2 + 4 sum |d| |s|) / n = eps ((D + 3) / 2 sum d^2 + 2 sum |d| |s|) / n.
  gsynth = 127.5 (G / f^2 + gp (s - t)), G = the sum of the 1 or 3 det_in cotangents over (b, c), gp = 2 gpix / n.
    Roundings: G 2 (three channels), / f^2 exact, gp 2 (times 2 exact), s - t 1, the product 1, the sum 1, times
    127.5 1: at most 8, each at most u times A = 127.5 (sum|gdet| / f^2 + |gp| |s - t|), the sum of absolute terms;
    and s's own 2 u |s| passes through as 127.5 |gp| 2 u |s|.  Per element
    |gsynth - gsynth64| <= eps (4 A + 127.5 |gp| |s|).  (A fused multiply-add only removes roundings.)

sqdist_rows, F in {1, 7, 8192, 8193, 20000} x rows in {1, 6}: all terms are non-negative, so the relative error against
  float64 is at most (serial runs + tree depth + 3) u with the tree's documented constants (proj_loss.sqdist_tree:
  sg2_lpips_pair_dist's): the subtraction's rounding, doubled by the square, and the square's are the 3.  The gradient
  2 g (f - tf) takes two roundings (the doubling is exact): every element within 2.001 u of float64, relatively.
"""
import numpy as np
import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24
EPS = 2.0 ** -23
PREP_CASES = [(c, h) for c in (1, 2, 3) for h in (4, 8, 32)] + [(1, 512)]


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.proj_loss'])


def _shifted(t, shift):
    """A contiguous copy of t that starts `shift` floats into a 16-byte aligned buffer."""
    buf = torch.empty([t.numel() + 8], dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[shift:shift + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _images(B, C, H):
    g = torch.Generator().manual_seed(1000 * C + H)
    synth = torch.rand([3, C, H, H], generator=g) * 2.4 - 1.2           # the generator overshoots [-1, 1]
    target = torch.rand([3, C, H, H], generator=g) * 255.0
    gdet = torch.randn([3, C if C not in (1, 3) else 1, 3, min(H, 256), min(H, 256)], generator=g)   # [b, m, 3, ., .]
    gpix = torch.randn([3, C if C not in (1, 3) else 1], generator=g)
    # the first B samples: sample b is the same tensor alone and in every batch
    return synth[:B].contiguous(), target[:B].contiguous(), gdet[:B].transpose(0, 1).reshape(-1, 3, *gdet.shape[3:]), gpix[:B]


_cache = {}


def _reference(B, C, H):
    """The composition in float64 on the CPU: det_in, pix, gsynth and the magnitudes the bounds are made of."""
    key = (B, C, H)
    if key not in _cache:
        from torch_utils.ops import proj_loss
        synth, target, gdet, gpix = _images(B, C, H)
        x = synth.double().requires_grad_(True)
        det_in, pix = proj_loss.prep_ref(x, target.double())
        ((det_in * gdet.double()).sum() + (pix * gpix.double()).sum()).backward()
        _cache[key] = dict(det_in=det_in.detach(), pix=pix.detach(), gsynth=x.grad)
    return _cache[key]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C,H', PREP_CASES)
def test_prep(C, H, B):
    from torch_utils.ops import proj_loss
    synth, target, gdet, gpix = _images(B, C, H)
    ref = _reference(B, C, H)
    M, (Hd, f) = proj_loss.num_modalities(C), proj_loss.det_side(H)
    nsrc = 3 if C == 3 else 1
    n = nsrc * H * H
    x = synth.to(DEV).requires_grad_(True)
    det_in, pix = proj_loss.prep(x, target.to(DEV))
    assert det_in.shape == (M * B, 3, Hd, Hd) and pix.shape == (B, M) and det_in.dtype == pix.dtype == torch.float32
    ((det_in * gdet.to(DEV)).sum() + (pix * gpix.to(DEV)).sum()).backward()
    assert x.grad.shape == x.shape and torch.isfinite(x.grad).all(), 'every element of gsynth is assigned'

    s32 = (synth + 1) * (255 / 2)                   # f32, as torch composes it (the CPU rounds as the device does)
    s64, t64 = (synth.double() + 1) * (255 / 2), target.double()
    if f == 1:
        want, _ = proj_loss.prep_ref(synth.to(DEV), target.to(DEV))
        assert torch.equal(det_in, want), 'f = 1: bitwise the torch composition'
        assert torch.equal(det_in.cpu(), proj_loss.split_rows(s32))
    else:
        mean_abs = proj_loss.split_rows(torch.nn.functional.avg_pool2d(s64.abs(), f))
        used = (det_in.detach().cpu().double() - ref['det_in']).abs() / (2.5 * EPS * mean_abs)
        print(f'prep C={C} H={H} B={B}: det_in at f = {f} uses {float(used.max()):.3g} of its bound')
        assert float(used.max()) <= 1.0

    # pix: every (b, m)
    D = f * f + 20
    d = (t64 - s64).abs()
    per_channel = lambda v: v.sum(dim=(2, 3))       # [B, C]
    sum_d2, sum_ds = per_channel(d * d), per_channel(d * s64.abs())
    if C == 3:
        sum_d2, sum_ds = sum_d2.sum(1, keepdim=True), sum_ds.sum(1, keepdim=True)
    bound = EPS * ((D + 3) / 2 * sum_d2 + 2 * sum_ds) / n
    used = (pix.detach().cpu().double() - ref['pix']).abs() / bound
    print(f'prep C={C} H={H} B={B}: pix uses {float(used.max()):.3g} of its bound')
    assert used.shape == (B, M) and float(used.max()) <= 1.0

    # gsynth: every element
    gp = (2 * gpix.double() / n).abs()                                  # [B, M]
    gp = gp.expand(B, C) if C == 3 else gp                              # per source channel
    gabs = gdet.double().abs().view(M, B, 3, Hd, Hd).transpose(0, 1)    # [B, M, 3, Hd, Hd]
    gabs = gabs[:, 0] if C == 3 else gabs.sum(2)                        # [B, C, Hd, Hd]: the channels that read (b, c)
    gabs = torch.nn.functional.interpolate(gabs, scale_factor=f, mode='nearest') / (f * f) if f > 1 else gabs
    A = 127.5 * (gabs + gp[:, :, None, None] * d)
    bound = EPS * (4 * A + 127.5 * gp[:, :, None, None] * s64.abs())
    used = (x.grad.cpu().double() - ref['gsynth']).abs() / bound
    print(f'prep C={C} H={H} B={B}: gsynth uses {float(used.max()):.3g} of its bound')
    assert float(used.max()) <= 1.0

    # a second run and a sample alone give the same bits
    again = proj_loss.prep(synth.to(DEV), target.to(DEV))
    assert torch.equal(again[0], det_in) and torch.equal(again[1], pix)
    if B == 3:
        for b in range(B):
            alone_det, alone_pix = proj_loss.prep(synth[b:b + 1].to(DEV), target[b:b + 1].to(DEV))
            assert torch.equal(alone_pix, pix[b:b + 1]), f'sample {b}: pix alone against the batch'
            assert torch.equal(alone_det, det_in.view(M, B, 3, Hd, Hd)[:, b]), f'sample {b}: det_in rows m B + b'


def test_prep_refuses_what_it_cannot_take():
    from torch_utils.ops import proj_loss
    x = torch.zeros([2, 1, 8, 8], device=DEV)
    with pytest.raises(RuntimeError, match='ROCm'):
        proj_loss.prep(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match='one shape'):
        proj_loss.prep(x, x[:1])
    with pytest.raises(RuntimeError, match='power of two'):
        proj_loss.prep(torch.zeros([1, 1, 12, 12], device=DEV), torch.zeros([1, 1, 12, 12], device=DEV))
    y = x.clone().requires_grad_(True)
    det_in, pix = proj_loss.prep(y, x)
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(pix.sum() + det_in.sum(), y, create_graph=True)


def _rows(R, F, seed):
    g = torch.Generator().manual_seed(seed)
    tf = torch.randn([6, F], generator=g)
    f = torch.where(torch.arange(6).view(6, 1) % 2 == 0, tf * (1 + 1e-3 * torch.rand([6, F], generator=g)),
                    torch.randn([6, F], generator=g))                   # near rows and unrelated rows
    return f[:R].contiguous(), tf[:R].contiguous(), torch.randn([6], generator=g)[:R].contiguous()


@pytest.mark.parametrize('R', [1, 6])
@pytest.mark.parametrize('F', [1, 7, 8192, 8193, 20000])
def test_sqdist_rows(F, R):
    from torch_utils.ops import proj_loss
    f, tf, g = _rows(R, F, seed=F)
    serial, depth = proj_loss.sqdist_tree(F)
    bound = (serial + depth + 3) * U
    x = f.to(DEV).requires_grad_(True)
    dist = proj_loss.sqdist_rows(x, tf.to(DEV))
    assert dist.shape == (R,) and dist.dtype == torch.float32
    (dist * g.to(DEV)).sum().backward()
    want = (f.double() - tf.double()).square().sum(1)
    err = float(((dist.detach().cpu().double() - want).abs() / want).max())
    print(f'sqdist_rows F={F} R={R}: rel error {err / U:.2f} x 2^-24 (bound {bound / U:.0f} x 2^-24)')
    assert err <= bound

    gwant = 2 * g.double().view(R, 1) * (f.double() - tf.double())
    assert x.grad.shape == x.shape and torch.isfinite(x.grad).all(), 'every element of the gradient is assigned'
    gerr = (x.grad.cpu().double() - gwant).abs()
    assert bool((gerr <= 2.001 * U * gwant.abs()).all()), float((gerr / gwant.abs().clamp_min(1e-300)).max()) / U

    assert torch.equal(proj_loss.sqdist_rows(f.to(DEV), tf.to(DEV)), dist), 'a second run gives the same bits'
    for shift_f, shift_t in ((1, 0), (0, 3), (2, 2)):      # unaligned row pointers: the same tree, element by element
        y = _shifted(f.to(DEV), shift_f).requires_grad_(True)
        d2 = proj_loss.sqdist_rows(y, _shifted(tf.to(DEV), shift_t))
        assert torch.equal(d2, dist), 'the bits do not depend on the alignment'
        (d2 * g.to(DEV)).sum().backward()
        assert torch.equal(y.grad, x.grad)
    if R == 6:
        for r in range(R):
            alone = proj_loss.sqdist_rows(f[r:r + 1].to(DEV), tf[r:r + 1].to(DEV))
            assert torch.equal(alone, dist[r:r + 1]), f'row {r} alone against the batch'


def test_sqdist_rows_refuses_what_it_cannot_take():
    from torch_utils.ops import proj_loss
    a = torch.zeros([2, 8], device=DEV)
    with pytest.raises(RuntimeError, match='ROCm'):
        proj_loss.sqdist_rows(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match='one shape'):
        proj_loss.sqdist_rows(a, a[:, :4])
    with pytest.raises(RuntimeError, match='float32'):
        proj_loss.sqdist_rows(a.double(), a.double())
    assert proj_loss.sqdist_rows(a + 1, a + 1).tolist() == [0.0, 0.0]
    y = a.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(proj_loss.sqdist_rows(y, a + 1).sum(), y, create_graph=True)


def test_launch_counts():
    """prep: 2 kernels forward, 1 backward; sqdist_rows: 2 forward, 1 backward -- whatever the batch is."""
    from torch.profiler import ProfilerActivity, profile
    from torch_utils.ops import proj_loss
    synth, target, gdet, gpix = _images(3, 2, 32)
    f, tf, g = _rows(6, 8193, seed=1)

    def events(fn):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if e.device_type.name == 'CUDA']

    with poison.unpoisoned(['torch_utils.ops.proj_loss']):      # (the poison's fills are launches of the test's own)
        x, t = synth.to(DEV).requires_grad_(True), target.to(DEV)
        y, ty = f.to(DEV).requires_grad_(True), tf.to(DEV)
        proj_loss.prep(x, t)[1].sum().backward()                # warm-up
        proj_loss.sqdist_rows(y, ty).sum().backward()
        out = []
        fwd = events(lambda: out.append(proj_loss.prep(x, t)))
        gd, gp = torch.ones_like(out[0][0]), torch.ones_like(out[0][1])
        bwd = events(lambda: torch.autograd.backward(out[0], [gd, gp]))
        assert sum('proj_' in n for n in fwd) == 2 and len(fwd) == 2, fwd
        assert sum('proj_prep_bwd' in n for n in bwd) == 1, bwd
        out = []
        fwd = events(lambda: out.append(proj_loss.sqdist_rows(y, ty)))
        go = torch.ones_like(out[0])
        bwd = events(lambda: out[0].backward(go))
        assert sum('sqdist_rows' in n for n in fwd) == 2 and len(fwd) == 2, fwd
        assert sum('sqdist_rows_bwd' in n for n in bwd) == 1, bwd
