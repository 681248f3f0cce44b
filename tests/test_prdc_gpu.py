"""The fused ball-count kernel (sg2_manifold_count; torch_utils/ops/manifold.py manifold_count) and compute_prdc on the
GPU against the float64 numpy oracle of dc_oracle.py.

Shapes: pr_oracle.CASES -- rows and columns that are no multiple of either tile (256 x 256, or 256 x 128 with
SG2_KNN_WIDE=0), a K tail of 8 after whole 32-steps (d = 40, 72, 136), several row and column tiles; SG2_KNN_SPLITS
forces the split merge.  Tolerance: pr_oracle.TAU = 2^-14 relative on a distance; every count and flag must lie between
the strict and the lenient evaluation and equal the oracle's wherever the two coincide (dc_oracle.judge; at most 2 %
of the probes and 1 % of the reals may fall outside that comparison)."""
import ctypes

import numpy as np
import pytest
import torch

import dc_oracle
import pr_oracle
from dc_oracle import K

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _count(probes, mani, radii, **kw):
    from torch_utils.ops import manifold
    count, covered = manifold.manifold_count(_dev(probes), _dev(mani), _dev(np.asarray(radii, dtype=np.float32)), **kw)
    assert count.dtype == torch.int32 and count.shape == (probes.shape[0],) and count.device.type == 'cuda'
    assert covered.dtype == torch.bool and covered.shape == (mani.shape[0],) and covered.device.type == 'cuda'
    return count, covered


@pytest.mark.parametrize('k', [K, 3])
@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_counts_and_flags_match_the_oracle(case, k):
    """Fed the oracle's radii: every probe's count and every real's flag, exact wherever TAU cannot change them."""
    real, gen = pr_oracle.features(case)
    o = dc_oracle.fed(case, k)
    count, covered = _count(gen, real, o.radii)
    count, covered = count.cpu().numpy(), covered.cpu().numpy()
    print(f'undecidable probes {o.undecidable_probes:.4f}, reals {o.undecidable_reals:.4f}; density '
          f'{count.sum() / (k * o.p):.4f} in [{o.density_strict:.4f}, {o.density_lenient:.4f}], coverage '
          f'{covered.mean():.4f} in [{o.coverage_strict:.4f}, {o.coverage_lenient:.4f}]')
    dc_oracle.judge(count, covered, o, probe_cap=0.02, real_cap=0.01)


@pytest.mark.parametrize('wide', ['0', '1'])
def test_both_tile_widths_match_the_oracle(wide, monkeypatch):
    monkeypatch.setenv('SG2_KNN_WIDE', wide)
    case = pr_oracle.CASES[-1]
    real, gen = pr_oracle.features(case)
    for splits in ('1', '2'):
        monkeypatch.setenv('SG2_KNN_SPLITS', splits)
        o = dc_oracle.fed(case, K)
        count, covered = _count(gen, real, o.radii)
        dc_oracle.judge(count.cpu().numpy(), covered.cpu().numpy(), o)


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_positive_count_is_membership_bit_for_bit(case):
    """count > 0 and manifold_member read the same balls: zero tolerance, both directions of the metric, k = 5 and 3,
    with and without the fp16 rounding of the distances."""
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(case)
    for mani, probes in ((real, gen), (gen, real)):
        m, p = _dev(mani), _dev(probes)
        for k in (K, 3):
            radii = manifold.knn_radii(m, k)
            for round16 in (True, False):
                count, _ = manifold.manifold_count(p, m, radii, round16=round16)
                assert torch.equal(count > 0, manifold.manifold_member(p, m, radii, round16=round16)), (k, round16)


def test_splits_tiles_and_reruns_are_bitwise_equal(monkeypatch):
    """Integer sums and ORs do not depend on the order: the column split, the tile width and a second run never change
    a bit of either output."""
    from torch_utils.ops import manifold
    real, gen = pr_oracle.features(pr_oracle.SMALL)
    x, g = _dev(real), _dev(gen)
    radii = manifold.knn_radii(x, K)
    base_c, base_f = manifold.manifold_count(g, x, radii)
    assert 1 < int(base_c.max()) and 0 < int(base_f.sum()) < base_f.numel() and 0 < int((base_c > 0).sum()) < base_c.numel()
    for wide in ('1', '0'):
        monkeypatch.setenv('SG2_KNN_WIDE', wide)
        for splits in ('1', '3', '2', None):
            if splits is None:
                monkeypatch.delenv('SG2_KNN_SPLITS')
            else:
                monkeypatch.setenv('SG2_KNN_SPLITS', splits)
            for _ in range(2):
                count, covered = manifold.manifold_count(g, x, radii)
                assert torch.equal(count, base_c), (wide, splits)
                assert torch.equal(covered, base_f), (wide, splits)


@pytest.mark.parametrize('wide', ['1', '0'])
@pytest.mark.parametrize('mirrored', [False, True])
def test_padded_probe_rows_take_no_part(mirrored, wide, monkeypatch):
    """260 probes are padded to two 256-row tiles with rows that read as zeros.  Two planted real features lie within
    their radius of the origin: no genuine probe reaches them, so neither may be covered or counted -- unless the
    last probe is a genuine all-zero row (mirrored), which must count and cover both."""
    monkeypatch.setenv('SG2_KNN_WIDE', wide)
    probes, mani, radii, o = dc_oracle.padding_fixture(mirrored)
    planted = [dc_oracle.PAD_J0, dc_oracle.PAD_J1]
    count, covered = _count(probes, mani, radii)
    count, covered = count.cpu().numpy(), covered.cpu().numpy()
    dc_oracle.judge(count, covered, o)
    if mirrored:
        assert covered[planted].all() and count[-1] == o.count[-1] >= 2
        assert int(count.sum()) == int(o.count.sum())
    else:
        assert not covered[planted].any()
        assert int(count.sum()) == int(o.count.sum())         # no probe counts them (the fixture is fully decidable)


@pytest.mark.parametrize('p', [256, 1])
def test_whole_tile_and_single_probe(p):
    """p = 256 exactly (no padded row) and p = 1 (255 padded rows) on the padding fixture's manifold."""
    probes, mani, radii, o = dc_oracle.padding_fixture(False, p=p)
    count, covered = _count(probes, mani, radii)
    dc_oracle.judge(count.cpu().numpy(), covered.cpu().numpy(), o)
    assert not covered[[dc_oracle.PAD_J0, dc_oracle.PAD_J1]].any()


def test_one_probe_one_real():
    """p = n = 1: the ball contains the probe or it does not; a zero probe against a zero feature is distance 0."""
    real, gen = pr_oracle.features(pr_oracle.CASES[0])
    x, y = real[:1], gen[:1]
    dist = float(pr_oracle.dist64(y, x)[0, 0])
    for radius, inside in ((np.float16(dist * 1.01), True), (np.float16(dist * 0.99), False)):
        count, covered = _count(y, x, np.array([radius]))
        assert count.tolist() == [int(inside)] and covered.tolist() == [inside]
    zero = np.zeros_like(x)
    count, covered = _count(zero, zero, np.array([0.0]))
    assert count.tolist() == [1] and covered.tolist() == [True]
    count, covered = _count(zero, zero, np.array([-1.0]))          # a negative radius never matches
    assert count.tolist() == [0] and covered.tolist() == [False]


@pytest.mark.parametrize('case', [pr_oracle.CASES[0], pr_oracle.CASES[-1]], ids=pr_oracle.case_id)
def test_every_output_is_written_and_nothing_beyond(case, monkeypatch):
    """The C entry point on pre-filled buffers: count holds -7, covered 0xAB and the scratch 0xFF bytes (an int partial
    of -1, a set column flag, NaN norms and thresholds) before the call; the outputs carry 64 guard elements.  The
    results equal the wrapper's, every element is overwritten and the guards are untouched."""
    import sg2hip
    from torch_utils.ops import manifold
    lib = sg2hip.lib()
    real, gen = pr_oracle.features(case)
    x, g = _dev(real), _dev(gen)
    (p, d), n = g.shape, x.shape[0]
    radii = manifold.knn_radii(x, K)
    for splits in ('1', '3'):
        monkeypatch.setenv('SG2_KNN_SPLITS', splits)
        want_c, want_f = manifold.manifold_count(g, x, radii)
        nbytes = ctypes.c_int64(0)
        assert lib.sg2_manifold_count_scratch_bytes(ctypes.byref(nbytes), p, n) == 0
        count = torch.full([p + 64], -7, dtype=torch.int32, device=DEV)
        covered = torch.full([n + 64], 0xAB, dtype=torch.uint8, device=DEV)
        scratch = torch.full([nbytes.value], 0xFF, dtype=torch.uint8, device=DEV)
        assert scratch.data_ptr() % 16 == 0
        rc = lib.sg2_manifold_count(sg2hip.ptr(count), sg2hip.ptr(covered), sg2hip.ptr(g), p, sg2hip.ptr(x), n,
                                    sg2hip.ptr(radii), sg2hip.F16, d, 1, sg2hip.ptr(scratch), nbytes.value,
                                    sg2hip.stream_ptr(g.device))
        assert rc == 0, lib.sg2_last_error()
        torch.cuda.synchronize()
        assert torch.equal(count[:p], want_c) and bool((count[:p] >= 0).all())
        assert torch.equal(covered[:n], want_f.to(torch.uint8)) and bool((covered[:n] <= 1).all())
        assert bool((count[p:] == -7).all()) and bool((covered[n:] == 0xAB).all())


class _Stats:
    def __init__(self, feats):
        self.feats = feats

    def get_all_torch(self):
        return torch.from_numpy(self.feats.astype(np.float32))


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_compute_prdc_end_to_end(case, monkeypatch):
    """compute_prdc over stub features, the radii from the kernels too: density and coverage inside the oracle's
    end-to-end interval widened by 1 / p resp. 1 / n, precision and recall within (undecidable share + 1 / probes) of
    the oracle's, as test_manifold_gpu.py bounds them; the composition on the device lands in the same intervals."""
    from metrics import metric_utils, density_coverage
    real, gen = pr_oracle.features(case)
    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_dataset', lambda **kw: _Stats(real))
    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_generator', lambda **kw: _Stats(gen))
    monkeypatch.delenv('SG2_PRDC_FUSED', raising=False)
    opts = metric_utils.MetricOptions(device=torch.device(DEV, 0))
    e = dc_oracle.end_to_end(case, K)
    o = pr_oracle.oracle(case, K)
    n, p = real.shape[0], gen.shape[0]
    for fused in (None, False):
        res = density_coverage.compute_prdc(opts, max_real=n, num_gen=p, nhood_size=K, fused=fused)
        assert sorted(res) == ['coverage', 'density', 'precision', 'recall']
        print(f'fused {fused}: {res}; density [{e.density_strict:.6f}, {e.density_lenient:.6f}], coverage '
              f'[{e.coverage_strict:.6f}, {e.coverage_lenient:.6f}]')
        assert e.density_strict - 1.0 / p <= res['density'] <= e.density_lenient + 1.0 / p
        assert e.coverage_strict - 1.0 / n <= res['coverage'] <= e.coverage_lenient + 1.0 / n
        for key, name, probes in (('precision', 'real', gen), ('recall', 'gen', real)):
            undecidable = float((o[f'pred_{name}_lenient'] != o[f'pred_{name}_strict']).mean())
            assert abs(res[key] - o[key]) <= undecidable + 1.0 / probes.shape[0], key


def test_prdc_from_features_matches_the_ops():
    """The four numbers are the integers of the ops: precision is pr50k's at the same k."""
    from metrics import density_coverage, precision_recall
    from torch_utils.ops import manifold
    real, gen = (_dev(x) for x in pr_oracle.features(pr_oracle.SMALL))
    res = density_coverage.prdc_from_features(real, gen, K, fused=True)
    count, covered = manifold.manifold_count(gen, real, manifold.knn_radii(real, K))
    assert res['density'] == int(count.sum()) / (K * gen.shape[0]) and res['coverage'] == int(covered.sum()) / real.shape[0]
    precision, recall = precision_recall.pr_from_features(real, gen, K)
    assert abs(res['precision'] - precision) < 1e-6 and abs(res['recall'] - recall) < 1e-6
