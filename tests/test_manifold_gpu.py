"""The fused k-NN manifold kernels (sg2_knn_radii, sg2_manifold_member; torch_utils/ops/manifold.py) and compute_pr on
the GPU against the float64 numpy oracle of pr_oracle.py, which test_pr_metric.py pins to the reference's numbers.

Shapes (pr_oracle.SHAPES): rows and columns that are no multiple of either tile (256 x 256, or 256 x 128 with
SG2_KNN_WIDE=0), a K tail of 8 after whole 32-steps (d = 40, 72, 136), more than one row tile and several column
tiles; SG2_KNN_SPLITS forces the split merge.
Tolerance: pr_oracle.TAU = 2^-14 relative on a distance (see there); everything rounded to fp16 must be bit-exact
wherever a distance error of TAU cannot change it."""
import numpy as np
import pytest
import torch

import pr_oracle
from pr_oracle import TAU, K

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.asarray(a, dtype=np.float16).view(np.uint16).astype(np.int64)      # non-negative: ordered like values


def _judge_radii(got, exact, lo, hi, cap=0.30):
    """got: float32 from the kernel (fp16 values).  Within one fp16 ulp of the oracle everywhere, bitwise equal where
    the lenient and strict radii coincide; at most `cap` of the radii may fall outside the bitwise comparison."""
    got16 = got.astype(np.float16)
    assert np.array_equal(got16.astype(np.float32), got), 'round16 radii must be fp16 values'
    assert np.abs(_bits(got16) - _bits(exact)).max() <= 1
    decidable = _bits(lo) == _bits(hi)
    share = 1.0 - decidable.mean()
    print(f'radii outside the bitwise comparison: {share:.4f}')
    assert share <= cap
    assert np.array_equal(got16[decidable], exact[decidable])


def _judge_member(got, lenient, strict, exact, cap=0.01):
    decidable = lenient == strict
    share = 1.0 - decidable.mean()
    print(f'undecidable probes: {share:.4f}')
    assert share <= cap
    assert np.array_equal(got[decidable], exact[decidable])
    return share


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_radii_error_without_rounding(case):
    """round16 = 0 against float64: the kernels' only inexact step (d2 in f32) stays within TAU on the distance."""
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(case)
    D_rr, D_gg, _ = pr_oracle.distances(case)
    for x, D in ((real, D_rr), (gen, D_gg)):
        got = manifold.knn_radii(_dev(x), K, round16=False).cpu().numpy().astype(np.float64)
        want = pr_oracle.kth_smallest(D, K)
        err = np.abs(got - want) / want
        print(f'max relative error of the unrounded radii: {err.max():.3e} (tau {TAU:.3e})')
        assert err.max() <= TAU


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_radii_match_the_oracle(case):
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(case)
    o = pr_oracle.oracle(case)
    for name, x in (('real', real), ('gen', gen)):
        got = manifold.knn_radii(_dev(x), K)
        assert got.dtype == torch.float32 and got.shape == (x.shape[0],)
        _judge_radii(got.cpu().numpy(), o[f'radii_{name}'], o[f'radii_{name}_lo'], o[f'radii_{name}_hi'])


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_membership_matches_the_oracle(case):
    """Fed the oracle's radii, the decision equals the oracle's on every probe that TAU cannot change."""
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(case)
    o = pr_oracle.oracle(case)
    for name, mani, probes in (('real', real, gen), ('gen', gen, real)):
        radii = _dev(o[f'radii_{name}'].astype(np.float32))
        got = manifold.manifold_member(_dev(probes), _dev(mani), radii)
        assert got.dtype == torch.bool and got.shape == (probes.shape[0],)
        _judge_member(got.cpu().numpy(), o[f'pred_{name}_fed_lenient'], o[f'pred_{name}_fed_strict'], o[f'pred_{name}'])


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_compute_pr_end_to_end(case, monkeypatch):
    """compute_pr over stub features: within (undecidable share + 1 / probes) of the reference's precision / recall."""
    from metrics import metric_utils, precision_recall
    real, gen = pr_oracle.features(case)
    z = np.load(pr_oracle_fixture())
    cid = pr_oracle.case_id(case)

    class Stats:
        def __init__(self, feats):
            self.feats = feats

        def get_all_torch(self):
            return torch.from_numpy(self.feats.astype(np.float32))

    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_dataset', lambda **kw: Stats(real))
    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_generator', lambda **kw: Stats(gen))
    opts = metric_utils.MetricOptions(device=torch.device(DEV, 0))
    precision, recall = precision_recall.compute_pr(opts, max_real=real.shape[0], num_gen=gen.shape[0], nhood_size=K,
                                                    row_batch_size=10000, col_batch_size=10000)
    o = pr_oracle.oracle(case)
    for got, key, name, probes in ((precision, 'precision', 'real', gen), (recall, 'recall', 'gen', real)):
        undecidable = float((o[f'pred_{name}_lenient'] != o[f'pred_{name}_strict']).mean())
        want = float(z[f'{cid}/{key}'])
        print(f'{key}: {got:.6f}, reference {want:.6f}, undecidable share {undecidable:.4f}')
        assert abs(got - want) <= undecidable + 1.0 / probes.shape[0]


def pr_oracle_fixture():
    import os
    from conftest import GOLDEN
    return os.path.join(GOLDEN, 'pr_ref.npz')


@pytest.mark.parametrize('k', [1, 7])
def test_other_neighbourhood_sizes(k):
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(pr_oracle.SMALL)
    D_rr, _, D_gr = pr_oracle.distances(pr_oracle.SMALL)
    exact = pr_oracle.radii16(D_rr, k)
    got = manifold.knn_radii(_dev(real), k)
    _judge_radii(got.cpu().numpy(), exact, pr_oracle.radii16(D_rr, k, -TAU), pr_oracle.radii16(D_rr, k, +TAU))
    unrounded = manifold.knn_radii(_dev(real), k, round16=False).cpu().numpy().astype(np.float64)
    want = pr_oracle.kth_smallest(D_rr, k)
    assert (np.abs(unrounded - want) / want).max() <= TAU
    hit = manifold.manifold_member(_dev(gen), _dev(real), _dev(exact.astype(np.float32))).cpu().numpy()
    _judge_member(hit, pr_oracle.member16(D_gr, exact, -TAU), pr_oracle.member16(D_gr, exact, +TAU),
                  pr_oracle.member16(D_gr, exact))


def test_splits_tiles_and_reruns_are_bitwise_equal(monkeypatch):
    """The column split (forced: 1 walks every column tile in one workgroup, 2 and 3 walk fewer per split and merge),
    the tile width (SG2_KNN_WIDE: 256 x 256 or 256 x 128, the same K order per dot product) and a second run never
    change a bit: selection and OR do not depend on the order."""
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(pr_oracle.SMALL)
    x, g = _dev(real), _dev(gen)
    base_r = manifold.knn_radii(x, K)
    base_r0 = manifold.knn_radii(x, K, round16=False)
    base_h = manifold.manifold_member(g, x, base_r)
    assert 0 < int(base_h.sum()) < base_h.numel()
    for wide in ('1', '0'):
        monkeypatch.setenv('SG2_KNN_WIDE', wide)
        for splits in ('1', '3', '2', None):
            if splits is None:
                monkeypatch.delenv('SG2_KNN_SPLITS')
            else:
                monkeypatch.setenv('SG2_KNN_SPLITS', splits)
            for _ in range(2):
                assert torch.equal(manifold.knn_radii(x, K), base_r), (wide, splits)
                assert torch.equal(manifold.knn_radii(x, K, round16=False), base_r0), (wide, splits)
                assert torch.equal(manifold.manifold_member(g, x, base_r), base_h), (wide, splits)


@pytest.mark.parametrize('wide', ['0', '1'])
def test_both_tile_widths_match_the_oracle(wide, monkeypatch):
    """The largest case (several row and column tiles of either width) under each tile width, k = 3 and k = 7."""
    from torch_utils.ops import manifold
    monkeypatch.setenv('SG2_KNN_WIDE', wide)
    case = pr_oracle.CASES[-1]
    real, gen = pr_oracle.features(case)
    o = pr_oracle.oracle(case)
    D_rr, _, _ = pr_oracle.distances(case)
    got = manifold.knn_radii(_dev(real), K).cpu().numpy()
    _judge_radii(got, o['radii_real'], o['radii_real_lo'], o['radii_real_hi'])
    got7 = manifold.knn_radii(_dev(real), 7).cpu().numpy()
    _judge_radii(got7, pr_oracle.radii16(D_rr, 7), pr_oracle.radii16(D_rr, 7, -TAU), pr_oracle.radii16(D_rr, 7, +TAU))
    hit = manifold.manifold_member(_dev(gen), _dev(real), _dev(o['radii_real'].astype(np.float32))).cpu().numpy()
    _judge_member(hit, o['pred_real_fed_lenient'], o['pred_real_fed_strict'], o['pred_real'])


def test_round16_is_the_rounding_of_the_unrounded_result():
    """fp16(radii without rounding) == radii with rounding wherever that is decidable; the same for membership with
    unrounded radii and comparison against the rounded ones."""
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(pr_oracle.SMALL)
    o = pr_oracle.oracle(pr_oracle.SMALL)
    x, g = _dev(real), _dev(gen)
    r0 = manifold.knn_radii(x, K, round16=False)
    r1 = manifold.knn_radii(x, K, round16=True)
    decidable = torch.from_numpy(_bits(o['radii_real_lo']) == _bits(o['radii_real_hi'])).to(DEV)
    assert float(decidable.float().mean()) >= 0.70
    assert torch.equal(r0.to(torch.float16).float()[decidable], r1[decidable])
    assert float((r0.to(torch.float16).float() - r1).abs().max()) <= float(np.spacing(np.float16(r1.max().item())))
    # unrounded membership against the unrounded radii: the float64 decision wherever TAU cannot change it
    D_rr, _, D_gr = pr_oracle.distances(pr_oracle.SMALL)
    kth = pr_oracle.kth_smallest(D_rr, K)
    h0 = manifold.manifold_member(g, x, _dev(kth.astype(np.float32)), round16=False).cpu().numpy()
    lenient = (D_gr * (1 - TAU) <= kth[None, :] * (1 + TAU)).any(axis=1)
    strict = (D_gr * (1 + TAU) <= kth[None, :] * (1 - TAU)).any(axis=1)
    _judge_member(h0, lenient, strict, (D_gr <= kth[None, :]).any(axis=1))
