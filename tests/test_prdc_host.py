"""Density / coverage (prdc50k5), the parts that need no GPU: the two entry points' argument errors, the op's refusal of
CPU tensors, the registry and the offline CLI, the composition path (fused=False, CPU tensors) against the float64
oracle of dc_oracle.py on every pr_oracle case, the oracle's own health, and planted faults that its judge must
reject."""
import ctypes
import json

import numpy as np
import pytest
import torch

import dc_oracle
import pr_oracle
from dc_oracle import K

FAKE = ctypes.c_void_p(4096)      # a non-null, aligned pointer: argument checks come before any device work
VGG_URL = 'https://api.ngc.nvidia.com/v2/models/nvidia/research/stylegan3/versions/1/files/metrics/vgg16.pkl'
KEYS = ('precision', 'recall', 'density', 'coverage')


def _lib():
    import sg2hip
    return sg2hip, sg2hip.lib()


def _scratch_bytes(lib, p, n):
    b = ctypes.c_int64(0)
    assert lib.sg2_manifold_count_scratch_bytes(ctypes.byref(b), p, n) == 0
    return b.value


def test_count_scratch_bytes_and_its_argument_errors():
    hip, lib = _lib()
    assert 'sg2_manifold_count_scratch_bytes' in hip.SIGNATURES and 'sg2_manifold_count' in hip.SIGNATURES
    assert lib.sg2_abi_version() == 11
    small, large = _scratch_bytes(lib, 50, 100), _scratch_bytes(lib, 1000, 900)
    assert 0 < small < large
    # at least the norms and thresholds of whole tiles, one int per row and one flag per (row tile, column)
    assert small >= (256 + 2 * 256) * 4 + 256 * 4 + 256
    b = ctypes.c_int64(0)
    assert lib.sg2_manifold_count_scratch_bytes(None, 10, 10) < 0 and b'non-null' in lib.sg2_last_error()
    assert lib.sg2_manifold_count_scratch_bytes(ctypes.byref(b), 0, 10) < 0 and b'>= 1' in lib.sg2_last_error()
    assert lib.sg2_manifold_count_scratch_bytes(ctypes.byref(b), 10, 0) < 0 and b'>= 1' in lib.sg2_last_error()


def test_manifold_count_argument_errors():
    hip, lib = _lib()
    big = 1 << 30

    def call(count=FAKE, covered=FAKE, probes=FAKE, p=50, manifold=FAKE, n=100, radii=FAKE, dtype=hip.F16, d=64,
             scratch=FAKE, nbytes=big):
        return lib.sg2_manifold_count(count, covered, probes, p, manifold, n, radii, dtype, d, 1, scratch, nbytes, None)

    for name in ('count', 'covered', 'probes', 'manifold', 'radii', 'scratch'):
        assert call(**{name: None}) < 0 and b'non-null' in lib.sg2_last_error(), name
    for dt in (hip.F32, hip.BF16, hip.F32S3):
        assert call(dtype=dt) < 0 and b'dtype' in lib.sg2_last_error()
    for d in (12, 0, -8):
        assert call(d=d) < 0 and b'multiple of 8' in lib.sg2_last_error()
    assert call(p=0) < 0 and b'>= 1' in lib.sg2_last_error()
    assert call(n=0) < 0 and b'>= 1' in lib.sg2_last_error()
    assert call(n=300000, d=4096) < 0 and b'2 GiB' in lib.sg2_last_error()
    assert call(p=300000, d=4096) < 0 and b'2 GiB' in lib.sg2_last_error()
    assert call(probes=ctypes.c_void_p(4104)) < 0 and b'16-byte aligned' in lib.sg2_last_error()
    assert call(manifold=ctypes.c_void_p(4100)) < 0 and b'16-byte aligned' in lib.sg2_last_error()
    assert call(scratch=ctypes.c_void_p(4104)) < 0 and b'16-byte aligned' in lib.sg2_last_error()
    need = _scratch_bytes(lib, 50, 100)
    assert call(nbytes=need - 1) < 0 and b'scratch too small' in lib.sg2_last_error()


def test_manifold_count_refuses_cpu_tensors_and_misfit_shapes():
    from torch_utils.ops import manifold
    x = torch.zeros([16, 8], dtype=torch.float16)
    with pytest.raises(RuntimeError, match='ROCm device tensors'):
        manifold.manifold_count(x, x, torch.zeros([16]))
    from metrics import density_coverage
    with pytest.raises(RuntimeError, match='ROCm device tensors'):
        density_coverage.prdc_from_features(x, x, 5, fused=True)


def test_prdc_metrics_are_registered_with_their_arguments(monkeypatch):
    from metrics import metric_main_mi_multimodal as mm, density_coverage
    assert mm.is_valid_metric('prdc50k5_full') and mm.is_valid_metric('prdc50k5')
    assert {'prdc50k5_full', 'prdc50k5'} <= set(mm.list_valid_metrics())
    assert mm.is_valid_metric('pr50k3_full') and not mm.is_valid_metric('kid50k_full')
    seen = []

    def fake_compute_prdc(opts, max_real, num_gen, nhood_size):
        seen.append((dict(opts.dataset_kwargs), max_real, num_gen, nhood_size))
        return dict(precision=0.25, recall=0.75, density=1.5, coverage=0.5)

    monkeypatch.setattr(density_coverage, 'compute_prdc', fake_compute_prdc)
    kw = dict(dataset_kwargs=dict(path='x', max_size=7, xflip=True), device=torch.device('cpu'))
    full = mm.calc_metric('prdc50k5_full', **kw)
    assert dict(full.results) == dict(prdc50k5_full_precision=0.25, prdc50k5_full_recall=0.75,
                                      prdc50k5_full_density=1.5, prdc50k5_full_coverage=0.5)
    assert seen[-1] == (dict(path='x', max_size=None, xflip=False), 200000, 50000, 5)
    part = mm.calc_metric('prdc50k5', **kw)
    assert dict(part.results) == dict(prdc50k5_precision=0.25, prdc50k5_recall=0.75, prdc50k5_density=1.5,
                                      prdc50k5_coverage=0.5)
    assert seen[-1] == (dict(path='x', max_size=None, xflip=True), 50000, 50000, 5)


def test_compute_prdc_passes_compute_pr_arguments(monkeypatch):
    """Both feature passes get compute_pr's arguments; the distance passes are stubbed."""
    from metrics import metric_utils, density_coverage, precision_recall
    assert density_coverage.DETECTOR_URL == precision_recall.DETECTOR_URL == VGG_URL
    calls = {}

    class Stats:
        def get_all_torch(self):
            return torch.zeros([4, 8])

    def stub(which):
        def f(**kw):
            calls[which] = kw
            return Stats()
        return f

    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_dataset', stub('real'))
    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_generator', stub('gen'))
    got = {}
    want = dict(precision=0.5, recall=0.25, density=1.25, coverage=0.75)

    def fake_prdc(real, gen, k, fused=None):
        got.update(real=real, gen=gen, k=k, fused=fused)
        return want

    monkeypatch.setattr(density_coverage, 'prdc_from_features', fake_prdc)
    opts = metric_utils.MetricOptions(device=torch.device('cpu'), mode_dict=dict(mode_idx=1, mode_name='MR'))
    assert density_coverage.compute_prdc(opts, 123, 45, 5) == want
    common = dict(opts=opts, detector_url=VGG_URL, detector_kwargs=dict(return_features=True), mode_dict=opts.mode_dict,
                  capture_all=True, rel_lo=0)
    assert calls['real'] == dict(common, rel_hi=0, max_items=123)
    assert calls['gen'] == dict(common, rel_hi=1, max_items=45)
    assert got['real'].dtype == torch.float16 and got['gen'].dtype == torch.float16
    assert got['k'] == 5 and got['fused'] is None


def test_fused_switch(monkeypatch):
    from metrics import density_coverage
    monkeypatch.delenv('SG2_PRDC_FUSED', raising=False)
    assert density_coverage.fused_default()
    monkeypatch.setenv('SG2_PRDC_FUSED', '0')
    assert not density_coverage.fused_default()
    monkeypatch.setenv('SG2_PRDC_FUSED', '1')
    assert density_coverage.fused_default()


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_oracle_is_not_degenerate(case):
    """Measured at k = 5, radii fed, over the six cases: density 0.54 .. 1.47, coverage 0.83 .. 0.99, largest count
    12 .. 19, lenient and strict counts differ on at most 0.89 % of the probes and flags on none of the reals (k = 3:
    0.77 % and 0.19 %); end to end the density interval is at most 0.0031 wide.  The caps the GPU tests put on the
    undecidable shares (2 % of the probes, 1 % of the reals) are conditions: the oracle stays under half of each."""
    for k in (K, 3):
        o = dc_oracle.fed(case, k)
        print(f'k {k}: density {o.density:.4f} [{o.density_strict:.4f}, {o.density_lenient:.4f}], coverage '
              f'{o.coverage:.4f} [{o.coverage_strict:.4f}, {o.coverage_lenient:.4f}], largest count {o.count.max()}, '
              f'undecidable probes {o.undecidable_probes:.4f}, reals {o.undecidable_reals:.4f}')
        assert o.undecidable_probes <= 0.01 and o.undecidable_reals <= 0.005
        assert o.density_strict <= o.density <= o.density_lenient
        assert o.coverage_strict <= o.coverage <= o.coverage_lenient
        assert 0.5 < o.density < 1.5 and 0.6 < o.coverage < 0.995
        assert 0 < (o.count > 0).mean() < 1, 'precision must be neither 0 nor 1'
        # a count is not a flag on these inputs: most probes lie in several balls
        assert o.count.max() >= 9 and (o.count > 1).mean() > 0.4
    o, e = dc_oracle.fed(case, K), dc_oracle.end_to_end(case, K)
    assert 12 <= o.count.max() <= 19 and 0.8 < o.coverage
    assert e.density_strict <= o.density_strict and o.density_lenient <= e.density_lenient
    assert 0 <= e.density_lenient - e.density_strict <= 0.0035
    assert e.recall_strict <= e.recall <= e.recall_lenient


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_composition_matches_the_oracle(case):
    """fused=False on CPU tensors: counts and flags with the oracle's radii fed in, then the four numbers end to end
    inside the oracle's own lenient / strict interval."""
    from metrics import density_coverage
    real, gen = pr_oracle.features(case)
    o = dc_oracle.fed(case, K)
    count, covered = density_coverage.composed_count(torch.from_numpy(gen), torch.from_numpy(real),
                                                     torch.from_numpy(o.radii.astype(np.float32)))
    assert count.dtype == torch.int32 and covered.dtype == torch.bool
    dc_oracle.judge(count.numpy(), covered.numpy(), o)
    density = int(count.sum()) / (K * o.p)
    coverage = int(covered.sum()) / o.n
    assert o.density_strict <= density <= o.density_lenient and o.coverage_strict <= coverage <= o.coverage_lenient
    # the composed radii are the oracle's wherever TAU cannot change them
    D_rr = pr_oracle.distances(case)[0]
    radii = density_coverage.composed_radii(torch.from_numpy(real), K).numpy()
    lo, hi = pr_oracle.radii16(D_rr, K, -dc_oracle.TAU), pr_oracle.radii16(D_rr, K, +dc_oracle.TAU)
    assert (lo <= radii).all() and (radii <= hi).all()
    e = dc_oracle.end_to_end(case, K)
    res = density_coverage.prdc_from_features(torch.from_numpy(real), torch.from_numpy(gen), K, fused=False)
    assert sorted(res) == sorted(KEYS)
    print({key: (getattr(e, key + '_strict'), res[key], getattr(e, key + '_lenient')) for key in KEYS})
    for key in KEYS:
        assert getattr(e, key + '_strict') <= res[key] <= getattr(e, key + '_lenient'), key


def test_composition_row_blocks(monkeypatch):
    """Several row blocks, the last one short: the same counts, flags and radii as one block."""
    from metrics import density_coverage
    real, gen = (torch.from_numpy(x) for x in pr_oracle.features(pr_oracle.SMALL))
    radii = density_coverage.composed_radii(real, K)
    count, covered = density_coverage.composed_count(gen, real, radii)
    monkeypatch.setattr(density_coverage, 'ROW_BLOCK', 100)
    # (a block's GEMM may round a distance differently: compare through the oracle, not bit for bit)
    o = dc_oracle.fed(pr_oracle.SMALL, K)
    c2, f2 = density_coverage.composed_count(gen, real, torch.from_numpy(o.radii.astype(np.float32)))
    dc_oracle.judge(c2.numpy(), f2.numpy(), o)
    assert c2.shape == count.shape and f2.shape == covered.shape
    assert density_coverage.composed_radii(real, K).shape == radii.shape


# ---- planted faults: the judge must reject each ----

def _rejects(count, covered, o):
    with pytest.raises(AssertionError):
        dc_oracle.judge(count, covered, o)


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_judge_rejects_planted_faults(case):
    o = dc_oracle.fed(case, K)
    _, D_gg, D_gr = pr_oracle.distances(case)
    dc_oracle.judge(o.count, o.covered, o)                                  # the oracle itself passes
    dc_oracle.judge(o.count_lenient, o.covered_lenient, o)
    dc_oracle.judge(o.count_strict, o.covered_strict, o)
    # counts collapsed to flags: precision would still be right
    _rejects((o.count > 0).astype(np.int32), o.covered, o)
    # radii taken per probe (the generated set's own) instead of per manifold row
    M = D_gr.astype(np.float16) <= pr_oracle.radii16(D_gg, K)[:, None]
    _rejects(dc_oracle.count(M), dc_oracle.covered(M), o)
    _rejects(o.count, dc_oracle.covered(M), o)
    # one count off by one, one flag flipped, on decidable elements
    i = int(np.flatnonzero(o.count_lenient == o.count_strict)[0])
    bad = o.count.copy()
    bad[i] += 1
    _rejects(bad, o.covered, o)
    j = int(np.flatnonzero(o.covered_lenient == o.covered_strict)[0])
    flipped = o.covered.copy()
    flipped[j] = ~flipped[j]
    _rejects(o.count, flipped, o)
    # dtypes and shapes
    _rejects(o.count.astype(np.int64), o.covered, o)
    _rejects(o.count, o.covered.astype(np.uint8), o)
    _rejects(o.count[:-1], o.covered, o)


@pytest.mark.parametrize('mirrored', [False, True])
def test_judge_rejects_the_padding_fault(mirrored):
    """252 all-zero probe rows appended (260 probes padded to two 256-row tiles) and allowed to take part: they cover
    the two planted features, and the judge sees it; without them the fixture's answer is clean."""
    probes, mani, radii, o = dc_oracle.padding_fixture(mirrored)
    planted = [dc_oracle.PAD_J0, dc_oracle.PAD_J1]
    assert probes.shape == (260, 40) and mani.shape == (300, 40) and o.undecidable_probes == 0
    if mirrored:
        assert o.covered[planted].all() and o.count[-1] >= 2 and not probes[-1].any()
    else:
        assert not o.covered[planted].any()
    padded = np.concatenate([probes, np.zeros([252, 40], dtype=np.float16)])
    M = dc_oracle.pairs(pr_oracle.dist64(padded, mani), radii)
    assert M[260:, planted].all()
    if not mirrored:
        _rejects(o.count, dc_oracle.covered(M), o)
    # the composition on the genuine probes passes
    from metrics import density_coverage
    count, covered = density_coverage.composed_count(torch.from_numpy(probes), torch.from_numpy(mani),
                                                     torch.from_numpy(radii.astype(np.float32)))
    dc_oracle.judge(count.numpy(), covered.numpy(), o)


# ---- the offline CLI ----

def test_cli_help_lists_the_metrics():
    from click.testing import CliRunner
    import calc_metrics_mi_multimodal as cli
    res = CliRunner().invoke(cli.calc_metrics, ['--help'])
    assert res.exit_code == 0 and 'prdc50k5_full' in res.output and 'prdc50k5 ' in res.output
    assert 'density and coverage' in res.output


def test_offline_cli_writes_four_numbers_per_modality(tmp_path, monkeypatch):
    """calc_metrics_mi_multimodal.py --metrics prdc50k5_full on a snapshot, the feature passes stubbed and the distance
    passes composed on the CPU (SG2_PRDC_FUSED=0): metric-<modality>-prdc50k5_full.jsonl holds four numbers."""
    from click.testing import CliRunner
    import calc_metrics_mi_multimodal as cli
    import legacy
    from metrics import metric_utils
    from training import networks_stylegan2 as net
    kw = dict(c_dim=0, img_resolution=16, img_channels=2, channel_base=64, channel_max=8)
    G = net.Generator(z_dim=16, w_dim=16, num_fp16_res=0, mapping_kwargs=dict(num_layers=2), **kw)
    D = net.Discriminator(num_fp16_res=0, **kw)
    run = tmp_path / 'run'
    run.mkdir()
    (run / 'training_options.json').write_text('{}')
    snapshot = str(run / 'network-snapshot-000004.pkl')
    legacy.save_network_pkl(snapshot, G, D, G, None,
                            dict(class_name='training.dataset_mi_multimodal.CustomImageFolderDataset',
                                 path='/data/from_pickle.zip', modalities=['a', 'b'], xflip=True, use_labels=False,
                                 split='train', dtype='float32', max_size=7))
    case = pr_oracle.CASES[0]
    real, gen = pr_oracle.features(case)
    seen = []

    class Stats:
        def __init__(self, feats):
            self.feats = feats

        def get_all_torch(self):
            return torch.from_numpy(self.feats.astype(np.float32))

    def dataset_pass(**kw):
        seen.append((kw['opts'].mode_dict['mode_name'], dict(kw['opts'].dataset_kwargs)['max_size'],
                     dict(kw['opts'].dataset_kwargs)['xflip'], kw['max_items']))
        return Stats(real)

    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_dataset', dataset_pass)
    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_generator', lambda **kw: Stats(gen))
    monkeypatch.setattr(cli, '_device', lambda rank: torch.device('cpu'))
    monkeypatch.setenv('SG2_PRDC_FUSED', '0')
    res = CliRunner().invoke(cli.calc_metrics, ['--network', snapshot, '--metrics', 'prdc50k5_full', '--verbose',
                                                'False'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert seen == [('a', None, False, 200000), ('b', None, False, 200000)]
    e = dc_oracle.end_to_end(case, K)
    for name in 'ab':
        with open(run / f'metric-{name}-prdc50k5_full.jsonl') as f:
            lines = [json.loads(line) for line in f]
        assert len(lines) == 1 and lines[0]['metric'] == 'prdc50k5_full' and lines[0]['mode'] == name
        results = lines[0]['results']
        assert sorted(results) == sorted(f'prdc50k5_full_{key}' for key in KEYS)
        for key in KEYS:
            assert getattr(e, key + '_strict') <= results[f'prdc50k5_full_{key}'] <= getattr(e, key + '_lenient'), key
