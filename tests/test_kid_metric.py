"""Kernel inception distance, the parts that need no GPU: the fixture check that pins the tests' numpy oracle
(kid_oracle.py) to the reference's own numbers (tests/golden/kid_ref.npz, written by tests/golden/make_kid_golden.py),
compute_kid's plumbing with the feature passes and the kernel stubbed, the registry, the two entry points' argument
errors and the op's checks of what it is given."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kid_oracle
from conftest import GOLDEN

FAKE = ctypes.c_void_p(4096)      # a non-null, aligned pointer: argument checks come before any device work
INCEPTION_URL = ('https://api.ngc.nvidia.com/v2/models/nvidia/research/stylegan3/versions/1/files/metrics/'
                 'inception-2015-12-05.pkl')


@pytest.mark.parametrize('index', range(len(kid_oracle.CASES)), ids=[kid_oracle.case_id(c) for c in kid_oracle.CASES])
def test_numpy_oracle_reproduces_the_reference_fixture(index):
    """kid_ref.npz holds what the reference's own compute_kid produced: its draws are the oracle's exactly, its
    float32 KID lies within the KID bound of the oracle's float64 value, and the features are the same."""
    case = kid_oracle.CASES[index]
    z = np.load(os.path.join(GOLDEN, 'kid_ref.npz'))
    cid = kid_oracle.case_id(case)
    real, gen = kid_oracle.features(case)
    assert real.dtype == np.float32 and gen.dtype == np.float32
    assert float(z[f'{cid}/sum_real']) == kid_oracle.checksum(real)
    assert float(z[f'{cid}/sum_gen']) == kid_oracle.checksum(gen)
    ig, ir = kid_oracle.draws(case)
    m = kid_oracle.subset_size(case)
    assert ig.shape == ir.shape == (case[3], m)
    np.testing.assert_array_equal(z[f'{cid}/idx_gen'], ig)
    np.testing.assert_array_equal(z[f'{cid}/idx_real'], ir)
    o = kid_oracle.oracle(case)
    print(f'{cid}: float64 KID {o["kid"]:.6f}, reference {float(z[f"{cid}/kid"]):.6f}, bound {kid_oracle.kid_bound(case):.3g}')
    assert abs(o['kid'] - float(z[f'{cid}/kid'])) <= kid_oracle.kid_bound(case)
    assert abs(o['kid'] - kid_oracle.KID_MEASURED[index]) < 1e-4


def test_tolerance_comes_from_the_reference_precision():
    """E_REF is a float32 rounding level (not 0, not a 16-bit one) and REL stays below every case's worst-case cap."""
    assert 2.0 ** -26 < kid_oracle.E_REF < 2.0 ** -20
    assert kid_oracle.REL == 16 * kid_oracle.E_REF
    for case in kid_oracle.CASES:
        assert kid_oracle.REL < kid_oracle.cap(case[2])
        assert kid_oracle.kid_bound(case) < 1e-4 < 50 * abs(kid_oracle.oracle(case)['kid'])


class _Stats:
    def __init__(self, feats):
        self.feats = feats

    def get_all_torch(self):
        return torch.from_numpy(np.array(self.feats))


def _stub_passes(monkeypatch, real, gen):
    from metrics import metric_utils
    calls = {}

    def stub(which, feats):
        def f(**kw):
            calls[which] = kw
            return _Stats(feats)
        return f

    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_dataset', stub('real', real))
    monkeypatch.setattr(metric_utils, 'compute_feature_stats_for_generator', stub('gen', gen))
    return calls


def _stub_kernel(monkeypatch, seen):
    from torch_utils.ops import poly_mmd

    def fake_subset_sums(gen, real, idx_gen, idx_real):
        seen.append((np.array(idx_gen), np.array(idx_real)))
        return torch.from_numpy(kid_oracle.sums64(gen.numpy(), real.numpy(), idx_gen, idx_real))

    monkeypatch.setattr(poly_mmd, 'subset_sums', fake_subset_sums)


@pytest.mark.parametrize('index', [0, 2], ids=['gen_smaller', 'capped'])
def test_compute_kid_plumbing(monkeypatch, index):
    """Both feature passes get the reference's arguments plus mode_dict; the draws come from the global np.random in
    the reference's order; m = min(n_real, n_gen, max_subset_size); the result is the oracle's KID."""
    from metrics import metric_utils, kernel_inception_distance as kid
    case = kid_oracle.CASES[index]
    n_real, n_gen, d, S, msub, _, _ = case
    real, gen = kid_oracle.features(case)
    calls = _stub_passes(monkeypatch, real, gen)
    seen = []
    _stub_kernel(monkeypatch, seen)
    monkeypatch.setattr(kid, 'composed_subset_sums', lambda *a: pytest.fail('the composition ran'))
    monkeypatch.delenv('SG2_KID_FUSED', raising=False)
    opts = metric_utils.MetricOptions(device=torch.device('cpu'), mode_dict=dict(mode_idx=1, mode_name='MR'))
    np.random.seed(kid_oracle.SEED)
    got = kid.compute_kid(opts, max_real=123, num_gen=45, num_subsets=S, max_subset_size=msub)
    common = dict(opts=opts, detector_url=INCEPTION_URL, detector_kwargs=dict(return_features=True),
                  mode_dict=opts.mode_dict, capture_all=True, rel_lo=0)
    assert calls['real'] == dict(common, rel_hi=0, max_items=123)
    assert calls['gen'] == dict(common, rel_hi=1, max_items=45)
    (ig, ir), = seen
    want_g, want_r = kid_oracle.draws(case)
    assert ig.shape == (S, min(n_real, n_gen, msub))
    np.testing.assert_array_equal(ig, want_g)
    np.testing.assert_array_equal(ir, want_r)
    assert isinstance(got, float) and got == kid_oracle.oracle(case)['kid']
    # a subset size above both sets: m = the smaller set, every row of it drawn once
    seen.clear()
    kid.compute_kid(opts, max_real=123, num_gen=45, num_subsets=2, max_subset_size=10 ** 6)
    (ig, ir), = seen
    assert ig.shape == ir.shape == (2, min(n_real, n_gen))


def test_compute_kid_other_ranks_return_nan_and_draw_nothing(monkeypatch):
    from metrics import metric_utils, kernel_inception_distance as kid
    real, gen = kid_oracle.features(kid_oracle.CASES[0])
    calls = _stub_passes(monkeypatch, real, gen)
    seen = []
    _stub_kernel(monkeypatch, seen)
    opts = metric_utils.MetricOptions(device=torch.device('cpu'), num_gpus=2, rank=1)
    np.random.seed(5)
    before = np.random.get_state()
    got = kid.compute_kid(opts, 50000, 50000, 100, 1000)
    after = np.random.get_state()
    assert np.isnan(got) and not seen and set(calls) == {'real', 'gen'}      # the passes are collective: both ran
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_kid_fused_0_selects_the_composition(monkeypatch):
    """SG2_KID_FUSED=0 runs the reference's float32 composition in torch (here on the CPU), not the kernel; its KID
    lies within the KID bound of the oracle's."""
    from metrics import metric_utils, kernel_inception_distance as kid
    from torch_utils.ops import poly_mmd
    case = kid_oracle.CASES[0]
    real, gen = kid_oracle.features(case)
    _stub_passes(monkeypatch, real, gen)
    monkeypatch.setattr(poly_mmd, 'subset_sums', lambda *a: pytest.fail('the fused kernel ran'))
    monkeypatch.setenv('SG2_KID_FUSED', '0')
    assert not kid.fused_default()
    opts = metric_utils.MetricOptions(device=torch.device('cpu'))
    np.random.seed(kid_oracle.SEED)
    got = kid.compute_kid(opts, case[0], case[1], case[3], case[4])
    assert abs(got - kid_oracle.oracle(case)['kid']) <= kid_oracle.kid_bound(case)
    ig, ir = (np.array(t) for t in kid_oracle.draws(case))
    sums = kid.composed_subset_sums(torch.from_numpy(np.array(gen)), torch.from_numpy(np.array(real)), ig, ir)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (case[3], 3)
    want = kid_oracle.oracle(case)['sums']
    assert float(np.max(np.abs(sums.numpy() - want) / want)) <= kid_oracle.REL
    monkeypatch.setenv('SG2_KID_FUSED', '1')
    assert kid.fused_default()


def test_kid_from_sums_is_the_estimator():
    from torch_utils.ops import poly_mmd
    case = kid_oracle.CASES[1]
    o = kid_oracle.oracle(case)
    assert poly_mmd.kid_from_sums(torch.from_numpy(np.array(o['sums'])), o['m']) == o['kid']
    assert poly_mmd.kid_from_sums(o['sums'], o['m']) == o['kid']
    # by hand: one subset, m = 3
    assert poly_mmd.kid_from_sums(np.array([[6.0, 12.0, 9.0]]), 3) == ((6.0 + 12.0) / 2 - 2 * 9.0 / 3) / 3


def test_kid50k_is_registered_with_the_reference_arguments(monkeypatch):
    from metrics import metric_main_mi_multimodal as mm, kernel_inception_distance as kid
    assert mm.is_valid_metric('kid50k') and 'kid50k' in mm.list_valid_metrics()
    seen = []

    def fake_compute_kid(opts, max_real, num_gen, num_subsets, max_subset_size):
        seen.append((dict(opts.dataset_kwargs), max_real, num_gen, num_subsets, max_subset_size))
        return 0.125

    monkeypatch.setattr(kid, 'compute_kid', fake_compute_kid)
    res = mm.calc_metric('kid50k', dataset_kwargs=dict(path='x', max_size=7, xflip=True), device=torch.device('cpu'))
    assert dict(res.results) == dict(kid50k=0.125) and res.metric == 'kid50k'
    assert seen == [(dict(path='x', max_size=None, xflip=True), 50000, 50000, 100, 1000)]


def _lib():
    import sg2hip
    return sg2hip, sg2hip.lib()


def test_entry_points_exist_and_refuse_bad_arguments():
    """Argument checks only: every call returns before any launch."""
    hip, lib = _lib()
    assert 'sg2_poly_mmd_scratch_bytes' in hip.SIGNATURES and 'sg2_poly_mmd_sums' in hip.SIGNATURES
    assert lib.sg2_poly_mmd_scratch_bytes and lib.sg2_poly_mmd_sums and lib.sg2_abi_version() == 11
    b = ctypes.c_int64(0)
    assert lib.sg2_poly_mmd_scratch_bytes(ctypes.byref(b), 100, 1000) == 0
    assert b.value == 100 * 3 * 8 * 8 * 8                   # one f64 per 128 x 128 tile slot
    assert lib.sg2_poly_mmd_scratch_bytes(ctypes.byref(b), 1, 128) == 0 and b.value == 24
    assert lib.sg2_poly_mmd_scratch_bytes(ctypes.byref(b), 1, 129) == 0 and b.value == 96
    assert lib.sg2_poly_mmd_scratch_bytes(None, 1, 8) == -1 and b'non-null' in lib.sg2_last_error()
    assert lib.sg2_poly_mmd_scratch_bytes(ctypes.byref(b), 1, 1) == -1 and b'm must be >= 2' in lib.sg2_last_error()
    assert lib.sg2_poly_mmd_scratch_bytes(ctypes.byref(b), 0, 8) == -1 and b'S must be >= 1' in lib.sg2_last_error()
    big = 1 << 30

    def call(sums=FAKE, gen=FAKE, n_gen=50, real=FAKE, n_real=60, idx_gen=FAKE, idx_real=FAKE, S=2, m=16, d=8,
             scratch=FAKE, nbytes=big):
        return lib.sg2_poly_mmd_sums(sums, gen, n_gen, real, n_real, idx_gen, idx_real, S, m, d, scratch, nbytes, None)

    for name in ('sums', 'gen', 'real', 'idx_gen', 'idx_real', 'scratch'):
        assert call(**{name: None}) == -1 and b'non-null' in lib.sg2_last_error(), name
    assert call(m=1) == -1 and b'm must be >= 2' in lib.sg2_last_error()
    for d in (6, 0, 2, -4):
        assert call(d=d) == -1 and b'multiple of 4' in lib.sg2_last_error(), d
    assert call(S=0) == -1 and b'S must be >= 1' in lib.sg2_last_error()
    assert call(n_gen=0) == -1 and b'n_gen and n_real' in lib.sg2_last_error()
    assert call(n_real=0) == -1 and b'n_gen and n_real' in lib.sg2_last_error()
    assert call(gen=ctypes.c_void_p(4100)) == -1 and b'16-byte aligned' in lib.sg2_last_error()
    assert call(real=ctypes.c_void_p(4104)) == -1 and b'16-byte aligned' in lib.sg2_last_error()
    assert call(nbytes=2 * 3 * 8 - 1) == -1 and b'scratch too small' in lib.sg2_last_error()


def test_subset_sums_refuses_cpu_features():
    from torch_utils.ops import poly_mmd
    x = torch.zeros([16, 8])
    idx = np.zeros([2, 4], dtype=np.int64)
    with pytest.raises(RuntimeError, match='ROCm device tensors'):
        poly_mmd.subset_sums(x, x, idx, idx)


def test_index_tables_are_checked_on_the_host():
    """What subset_sums checks before it uploads a table: the kernel trusts its indices."""
    from torch_utils.ops import poly_mmd
    good = np.arange(12).reshape(3, 4)
    ig, ir = poly_mmd.check_tables(good, torch.from_numpy(good), 12, 20)
    assert ig.dtype == ir.dtype == np.int32 and ig.flags.c_contiguous
    np.testing.assert_array_equal(ig, good)
    np.testing.assert_array_equal(ir, good)
    ig, _ = poly_mmd.check_tables(good.T[:, ::-1], good.T, 12, 12)      # a strided view is taken as its values
    np.testing.assert_array_equal(ig, good.T[:, ::-1])
    with pytest.raises(RuntimeError, match=r'idx_gen \[3, 4\].*outside the 11 rows'):
        poly_mmd.check_tables(good, good, 11, 20)
    with pytest.raises(RuntimeError, match=r'idx_real \[3, 4\].*outside the 11 rows'):
        poly_mmd.check_tables(good, good, 12, 11)
    with pytest.raises(RuntimeError, match=r'\[-1, 10\]'):
        poly_mmd.check_tables(good - 1, good, 12, 12)
    with pytest.raises(RuntimeError, match=r'idx_gen \[3, 4\] and idx_real \[4, 3\]'):
        poly_mmd.check_tables(good, good.reshape(4, 3), 12, 12)
    with pytest.raises(RuntimeError, match=r'idx_gen must be \[S, m\]; got \[12\]'):
        poly_mmd.check_tables(good.reshape(-1), good, 12, 12)
    with pytest.raises(RuntimeError, match=r'idx_real must be \[S, m\]; got \[3, 2, 2\]'):
        poly_mmd.check_tables(good, good.reshape(3, 2, 2), 12, 12)
    with pytest.raises(RuntimeError, match='integers'):
        poly_mmd.check_tables(good.astype(np.float32), good, 12, 12)


def test_offline_cli_evaluates_kid50k_per_modality(tmp_path, monkeypatch):
    """calc_metrics_mi_multimodal.py --metrics kid50k: the registry's kid50k runs once per modality of the snapshot's
    dataset options (compute_kid itself stubbed) and metric-<modality>-kid50k.jsonl is appended in the run directory."""
    import json
    from click.testing import CliRunner
    import calc_metrics_mi_multimodal as cli
    import legacy
    from metrics import kernel_inception_distance as kid
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
    seen = []

    def fake_compute_kid(opts, max_real, num_gen, num_subsets, max_subset_size):
        seen.append((opts.mode_dict, opts.dataset_kwargs.max_size, max_real, num_gen, num_subsets, max_subset_size))
        return 0.25 * len(seen)

    monkeypatch.setattr(kid, 'compute_kid', fake_compute_kid)
    monkeypatch.setattr(cli, '_device', lambda rank: torch.device('cpu'))
    res = CliRunner().invoke(cli.calc_metrics, ['--network', snapshot, '--metrics', 'kid50k', '--verbose', 'False'],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert seen == [({'mode_name': n, 'mode_idx': i}, None, 50000, 50000, 100, 1000) for i, n in enumerate('ab')]
    for i, n in enumerate('ab'):
        with open(run / f'metric-{n}-kid50k.jsonl') as f:
            lines = [json.loads(line) for line in f]
        assert len(lines) == 1 and lines[0]['metric'] == 'kid50k' and lines[0]['mode'] == n
        assert lines[0]['results'] == {'kid50k': 0.25 * (i + 1)}
