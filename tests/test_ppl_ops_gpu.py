"""The two perceptual-path-length kernels on the GPU (csrc/ppl.hip through torch_utils/ops/ppl.py).

prep_images: every (C, channel choice, factor) at H = W in {8, 24, 32}, cropped and not, from a 16-byte aligned and
  from a 4-byte shifted buffer.  H = 24 cropped is a 12 x 12 window at offset (9, 6): nothing is 16-byte aligned, and at
  factor 4 the 3 x 3 output planes shift every row's alignment.  factor 1: bitwise the torch composition on the device;
  factor > 1: within 2^-14 absolute of float64 (<= 16 terms of magnitude ~1: sum error <= 15 * 2^-24 * 16, the scaling
  by 1/f^2 exact, two more roundings, times 127.5: < 2^-15.5).
pair_distances: B in {1, 2, 3}, F in {1, 7, 1024, 4099, 2^20 + 5}, rows 1e-4 apart and unrelated rows.  All terms are
  non-negative, so the relative error against float64 is at most (serial runs + tree depth + 3) * 2^-24 with the
  kernel's documented constants (ops.pair_dist_tree: 9 + 18 at these sizes): the subtraction (its rounding doubled by
  the square), the square and the division are the 3 beyond the additions.  Bitwise: a second run, a pair alone against
  the same pair in a batch, and a 4-byte shifted buffer against an aligned one.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24


def _shifted(t, shift):
    """A contiguous copy of t that starts `shift` floats into a 16-byte aligned buffer."""
    buf = torch.empty([t.numel() + 8], dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[shift:shift + t.numel()].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize('crop', [False, True], ids=['full', 'crop'])
@pytest.mark.parametrize('res', [8, 24, 32])
def test_prep_images(res, crop):
    from torch_utils.ops import ppl as ops
    g = torch.Generator().manual_seed(res + crop)
    worst, count = 0.0, 0
    for C in (1, 2, 3):
        x = (torch.rand([4, C, res, res], generator=g) * 2.4 - 1.2).to(DEV)
        for shift in (0, 1):
            xs = _shifted(x, shift)
            for channel in ([None] if C in (1, 3) else []) + list(range(C)):
                for factor in (1, 2, 4):
                    got = ops.prep_images(xs, channel=channel, crop=crop, factor=factor)
                    side = (res // 2 if crop else res) // factor
                    assert got.shape == (4, 3, side, side) and got.dtype == torch.float32
                    what = f'C={C} channel={channel} factor={factor} shift={shift}'
                    if factor == 1:
                        want = ops.prep_images_ref(x, channel=channel, crop=crop, factor=1)
                        assert torch.equal(got, want), what
                        assert torch.equal(ops.prep_images(xs, channel=channel, crop=crop, factor=0), want), what
                    else:
                        want = ops.prep_images_ref(x.double(), channel=channel, crop=crop, factor=factor)
                        err = float((got.double() - want).abs().max())
                        worst = max(worst, err)
                        assert err <= 2.0 ** -14, (what, err)
                    count += 1
    print(f'prep_images res {res} crop {crop}: {count} cases, worst |error| at factor > 1 {worst:.3g} (bound {2.0 ** -14:.3g})')


def test_prep_images_argument_errors():
    from torch_utils.ops import ppl as ops
    x = torch.zeros([2, 2, 16, 16], device=DEV)
    with pytest.raises(RuntimeError, match='C = 1 or C = 3'):
        ops.prep_images(x)
    with pytest.raises(RuntimeError, match='divide'):
        ops.prep_images(x, channel=0, factor=3)
    with pytest.raises(RuntimeError, match='float32'):
        ops.prep_images(x.half(), channel=0)
    # a channels_last image is read as the NCHW tensor it is
    y = torch.randn([2, 3, 16, 16], device=DEV)
    assert torch.equal(ops.prep_images(y.contiguous(memory_format=torch.channels_last)), ops.prep_images_ref(y))


def _rows(B, F, kind, seed):
    g = torch.Generator().manual_seed(seed)
    t0 = torch.randn([B, F], generator=g)
    if kind == 'near':
        t1 = t0 * (1 + 1e-4 * (torch.rand([B, F], generator=g) * 2 - 1))
    else:
        t1 = torch.randn([B, F], generator=g)
    return torch.cat([t0, t1]).to(DEV)


@pytest.mark.parametrize('kind', ['near', 'unrelated'])
@pytest.mark.parametrize('F', [1, 7, 1024, 4099, 2 ** 20 + 5])
def test_pair_distances(F, kind):
    from torch_utils.ops import ppl as ops
    serial, depth = ops.pair_dist_tree(F)
    bound = (serial + depth + 3) * U
    assert bound <= 64 * U
    for B in (1, 2, 3):
        eps = 1e-2 if B == 2 else 1e-4
        feats = _rows(B, F, kind, seed=F + B)
        got = ops.pair_distances(feats, eps)
        assert got.shape == (B,) and got.dtype == torch.float32
        f64 = feats.double()
        want = (f64[:B] - f64[B:]).square().sum(1) / float(np.float32(eps * eps))
        err = float(((got.double() - want).abs() / want).max())
        print(f'pair_distances F={F} B={B} {kind}: rel error {err:.3g} = {err / U:.2f} x 2^-24 (bound {bound / U:.0f} x 2^-24)')
        assert err <= bound
        assert torch.equal(ops.pair_distances(feats, eps), got), 'a second run gives the same bits'
        assert torch.equal(ops.pair_distances(_shifted(feats, 1), eps), got), 'the bits do not depend on the alignment'
        if B == 3:
            for b in range(B):
                alone = ops.pair_distances(feats[[b, B + b]].contiguous(), eps)
                assert torch.equal(alone, got[b:b + 1]), f'pair {b} alone against the batch'


def test_pair_distances_argument_errors():
    from torch_utils.ops import ppl as ops
    with pytest.raises(RuntimeError, match='2B'):
        ops.pair_distances(torch.zeros([3, 8], device=DEV), 1e-4)
    with pytest.raises(RuntimeError, match='eps'):
        ops.pair_distances(torch.zeros([2, 8], device=DEV), 0.0)
    with pytest.raises(RuntimeError, match='float32'):
        ops.pair_distances(torch.zeros([2, 8], device=DEV, dtype=torch.float64), 1e-4)
    same = torch.ones([4, 100], device=DEV)
    assert ops.pair_distances(same, 1e-4).tolist() == [0.0, 0.0]
