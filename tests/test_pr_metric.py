"""Precision / recall metric, the parts that need no GPU: the ABI-10 entry points' argument errors, the op's refusal of
CPU tensors, the metric registry, FeatureStats with capture_all (get_all_torch, save / load, the world-size-2 gather),
the per-detector offline lookup, and the fixture check that pins the tests' numpy oracle (pr_oracle.py) to the
reference's own numbers (tests/golden/pr_ref.npz, written by tests/golden/make_pr_golden.py)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pr_oracle
from conftest import GOLDEN

FAKE = ctypes.c_void_p(4096)      # a non-null, aligned pointer: argument checks come before any device work
VGG_URL = 'https://api.ngc.nvidia.com/v2/models/nvidia/research/stylegan3/versions/1/files/metrics/vgg16.pkl'


def _lib():
    import sg2hip
    return sg2hip, sg2hip.lib()


def _scratch_bytes(lib, rows, cols, k):
    b = ctypes.c_int64(0)
    assert lib.sg2_knn_scratch_bytes(ctypes.byref(b), rows, cols, k) == 0
    return b.value


def test_scratch_bytes_and_its_argument_errors():
    hip, lib = _lib()
    assert _scratch_bytes(lib, 1000, 1000, 3) > 0
    assert _scratch_bytes(lib, 1000, 1000, 7) >= _scratch_bytes(lib, 1000, 1000, 3)
    b = ctypes.c_int64(0)
    assert lib.sg2_knn_scratch_bytes(None, 10, 10, 3) < 0 and b'non-null' in lib.sg2_last_error()
    assert lib.sg2_knn_scratch_bytes(ctypes.byref(b), 10, 10, 0) < 0 and b'k must be' in lib.sg2_last_error()
    assert lib.sg2_knn_scratch_bytes(ctypes.byref(b), 10, 10, 8) < 0 and b'k must be' in lib.sg2_last_error()
    assert lib.sg2_knn_scratch_bytes(ctypes.byref(b), 0, 10, 3) < 0


def test_knn_radii_argument_errors():
    hip, lib = _lib()
    big = 1 << 30

    def call(radii=FAKE, x=FAKE, dtype=hip.F16, n=100, d=64, k=3, scratch=FAKE, nbytes=big):
        return lib.sg2_knn_radii(radii, x, dtype, n, d, k, 1, scratch, nbytes, None)

    assert call(radii=None) < 0 and b'non-null' in lib.sg2_last_error()
    assert call(x=None) < 0 and b'non-null' in lib.sg2_last_error()
    assert call(scratch=None) < 0 and b'non-null' in lib.sg2_last_error()
    for dt in (hip.F32, hip.BF16, hip.F32S3):
        assert call(dtype=dt) < 0 and b'dtype' in lib.sg2_last_error()
    assert call(d=60) < 0 and b'multiple of 8' in lib.sg2_last_error()
    assert call(k=0) < 0 and b'k must be' in lib.sg2_last_error()
    assert call(k=8) < 0 and b'k must be' in lib.sg2_last_error()
    assert call(n=3, k=3) < 0 and b'k + 1' in lib.sg2_last_error()
    assert call(n=300000, d=4096) < 0 and b'2 GiB' in lib.sg2_last_error()
    need = _scratch_bytes(lib, 100, 100, 3)
    assert call(nbytes=need - 1) < 0 and b'scratch too small' in lib.sg2_last_error()


def test_manifold_member_argument_errors():
    hip, lib = _lib()
    big = 1 << 30

    def call(hit=FAKE, probes=FAKE, p=50, manifold=FAKE, n=100, radii=FAKE, dtype=hip.F16, d=64, scratch=FAKE,
             nbytes=big):
        return lib.sg2_manifold_member(hit, probes, p, manifold, n, radii, dtype, d, 1, scratch, nbytes, None)

    for name in ('hit', 'probes', 'manifold', 'radii', 'scratch'):
        assert call(**{name: None}) < 0 and b'non-null' in lib.sg2_last_error(), name
    assert call(dtype=hip.F32) < 0 and b'dtype' in lib.sg2_last_error()
    assert call(d=12) < 0 and b'multiple of 8' in lib.sg2_last_error()
    assert call(p=0) < 0
    assert call(n=300000, d=4096) < 0 and b'2 GiB' in lib.sg2_last_error()
    need = _scratch_bytes(lib, 50, 100, 1)
    assert call(nbytes=need - 1) < 0 and b'scratch too small' in lib.sg2_last_error()


def test_manifold_ops_refuse_cpu_tensors():
    from torch_utils.ops import manifold
    x = torch.zeros([16, 8], dtype=torch.float16)
    with pytest.raises(RuntimeError):
        manifold.knn_radii(x, 3)
    with pytest.raises(RuntimeError):
        manifold.manifold_member(x, x, torch.zeros([16]))


def test_metrics_are_registered_with_the_reference_result_names(monkeypatch):
    from metrics import metric_main_mi_multimodal as mm, precision_recall
    assert mm.is_valid_metric('pr50k3_full') and mm.is_valid_metric('pr50k3')
    assert mm.is_valid_metric('fid50k_full') and not mm.is_valid_metric('kid50k_full')
    seen = []

    def fake_compute_pr(opts, max_real, num_gen, nhood_size, row_batch_size, col_batch_size):
        seen.append((dict(opts.dataset_kwargs), max_real, num_gen, nhood_size, row_batch_size, col_batch_size))
        return 0.25, 0.75

    monkeypatch.setattr(precision_recall, 'compute_pr', fake_compute_pr)
    kw = dict(dataset_kwargs=dict(path='x', max_size=7, xflip=True), device=torch.device('cpu'))
    full = mm.calc_metric('pr50k3_full', **kw)
    assert dict(full.results) == dict(pr50k3_full_precision=0.25, pr50k3_full_recall=0.75)
    assert seen[-1] == (dict(path='x', max_size=None, xflip=False), 200000, 50000, 3, 10000, 10000)
    part = mm.calc_metric('pr50k3', **kw)
    assert dict(part.results) == dict(pr50k3_precision=0.25, pr50k3_recall=0.75)
    assert seen[-1] == (dict(path='x', max_size=None, xflip=True), 50000, 50000, 3, 10000, 10000)


def test_compute_pr_passes_the_reference_arguments(monkeypatch):
    """Both feature passes get the reference's arguments (precision_recall.py:41-47); the kernels are stubbed."""
    from metrics import metric_utils, precision_recall
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

    def fake_pr(real, gen, k):
        got.update(real=real, gen=gen, k=k)
        return 0.5, 0.5

    monkeypatch.setattr(precision_recall, 'pr_from_features', fake_pr)
    opts = metric_utils.MetricOptions(device=torch.device('cpu'), mode_dict=dict(mode_idx=1, mode_name='MR'))
    assert precision_recall.compute_pr(opts, 123, 45, 3, 10000, 10000) == (0.5, 0.5)
    common = dict(opts=opts, detector_url=VGG_URL, detector_kwargs=dict(return_features=True), mode_dict=opts.mode_dict,
                  capture_all=True, rel_lo=0)
    assert calls['real'] == dict(common, rel_hi=0, max_items=123)
    assert calls['gen'] == dict(common, rel_hi=1, max_items=45)
    assert got['real'].dtype == torch.float16 and got['gen'].dtype == torch.float16 and got['k'] == 3


def test_feature_stats_capture_all_roundtrip(tmp_path):
    from metrics import metric_utils
    g = torch.Generator().manual_seed(3)
    batches = [torch.randn([5, 6], generator=g) for _ in range(4)]
    s = metric_utils.FeatureStats(capture_all=True, max_items=17)
    for b in batches:
        s.append_torch(b)
    want = torch.cat(batches)[:17]
    got = s.get_all_torch()
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and torch.equal(got, want)
    path = str(tmp_path / 'stats.npz')
    s.save(path)
    back = metric_utils.FeatureStats.load(path)
    assert back.capture_all and not back.capture_mean_cov
    assert back.num_items == 17 and back.num_features == 6 and back.max_items == 17
    assert torch.equal(back.get_all_torch(), want)
    # moments and features together; a moments-only file loads as before
    both = metric_utils.FeatureStats(capture_all=True, capture_mean_cov=True)
    both.append_torch(batches[0])
    both.save(path)
    back = metric_utils.FeatureStats.load(path)
    assert back.capture_all and back.capture_mean_cov and torch.equal(back.get_all_torch(), batches[0])
    np.testing.assert_array_equal(back.get_mean_cov()[1], both.get_mean_cov()[1])
    fid = metric_utils.FeatureStats(capture_mean_cov=True)
    fid.append_torch(batches[0])
    fid.save(path)
    assert sorted(np.load(path).files) == ['max_items', 'num_features', 'num_items', 'raw_cov', 'raw_mean']
    back = metric_utils.FeatureStats.load(path)
    assert not back.capture_all and back.capture_mean_cov
    np.testing.assert_array_equal(back.get_mean_cov()[0], fid.get_mean_cov()[0])


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, paths, result_q):
    import sys
    sys.path[:0] = paths
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    try:
        from metrics import metric_utils
        g = torch.Generator().manual_seed(11)
        stream = torch.randn([4, 6, 5], generator=g)       # 4 global batches of 6 items: rank r holds rows r::2
        out = {}
        for max_items in (24, 21, 20, 7, 1):               # 21: the last batch is cut 2 : 1; 7, 1: early cuts
            s = metric_utils.FeatureStats(capture_all=True, max_items=max_items)
            for b in stream:
                s.append_torch(b[rank::world], num_gpus=world, rank=rank)
            s.reduce(world)
            out[max_items] = (s.num_items, s.get_all_torch().clone())
        result_q.put((rank, {k: (n, v.numpy()) for k, (n, v) in out.items()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_capture_all_gathers_the_global_set_gloo():
    """After reduce() both ranks hold the multiset of rows a single process keeps with the same max_items."""
    from metrics import metric_utils
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, 'gan-track_amd'), root]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, paths, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(60)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    g = torch.Generator().manual_seed(11)
    stream = torch.randn([4, 6, 5], generator=g)
    canon = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    for max_items in (24, 21, 20, 7, 1):
        single = metric_utils.FeatureStats(capture_all=True, max_items=max_items)
        for b in stream:
            single.append_torch(b)
        want = single.get_all_torch().numpy()
        assert want.shape[0] == max_items
        np.testing.assert_array_equal(want, stream.reshape(-1, 5).numpy()[:max_items])
        for rank in (0, 1):
            n, got = res[rank][max_items]
            assert n == max_items and got.shape == want.shape, (rank, max_items, got.shape)
            np.testing.assert_array_equal(canon(got), canon(want))


def test_detector_lookup_is_per_detector(monkeypatch, tmp_path):
    from metrics import metric_utils, frechet_inception_distance, precision_recall
    assert precision_recall.DETECTOR_URL == VGG_URL

    class Det(torch.nn.Module):
        def __init__(self, scale):
            super().__init__()
            self.scale = scale

        def forward(self, x):
            return x.float().mean([2, 3]) * self.scale

    paths = {}
    for name, scale in (('inception', 1.0), ('vgg', 2.0)):
        paths[name] = str(tmp_path / f'{name}.pt')
        torch.jit.script(Det(scale)).save(paths[name])
    monkeypatch.setattr(metric_utils, '_detectors', {})
    monkeypatch.delenv('SG2_PR_DETECTOR', raising=False)
    monkeypatch.setenv('SG2_FID_DETECTOR', paths['inception'])
    x = torch.ones([1, 3, 2, 2])
    # the Inception file alone no longer answers a VGG request, and the error names the right variable
    with pytest.raises(RuntimeError, match='SG2_PR_DETECTOR'):
        metric_utils.get_feature_detector(VGG_URL)
    assert float(metric_utils.get_feature_detector(frechet_inception_distance.DETECTOR_URL)(x)[0, 0]) == 1.0
    monkeypatch.setenv('SG2_PR_DETECTOR', paths['vgg'])
    assert float(metric_utils.get_feature_detector(VGG_URL)(x)[0, 0]) == 2.0
    # another detector has no variable; register_detector serves any url
    with pytest.raises(RuntimeError, match='register_detector'):
        metric_utils.get_feature_detector('https://example.invalid/other.pkl')
    monkeypatch.setattr(metric_utils, '_detectors', {})
    monkeypatch.delenv('SG2_FID_DETECTOR')
    with pytest.raises(RuntimeError, match='SG2_FID_DETECTOR'):
        metric_utils.get_feature_detector(frechet_inception_distance.DETECTOR_URL)
    marker = object()
    metric_utils.register_detector(VGG_URL, marker)
    metric_utils.register_detector(frechet_inception_distance.DETECTOR_URL, marker)
    assert metric_utils.get_feature_detector(VGG_URL) is marker
    assert metric_utils.get_feature_detector(frechet_inception_distance.DETECTOR_URL) is marker


@pytest.mark.parametrize('case', pr_oracle.CASES, ids=pr_oracle.case_id)
def test_numpy_oracle_reproduces_the_reference_fixture(case):
    """pr_ref.npz holds what the reference's own compute_pr control flow produced; the numpy restatement the GPU tests
    judge against gives the same radii, predictions, precision and recall, exactly."""
    z = np.load(os.path.join(GOLDEN, 'pr_ref.npz'))
    cid, sid = pr_oracle.case_id(case), pr_oracle.shape_id(case)
    real, gen = pr_oracle.features(case)
    assert z[f'{sid}/real'].dtype == np.float16 and z[f'{cid}/radii_real'].dtype == np.float16
    np.testing.assert_array_equal(z[f'{sid}/real'], real)
    np.testing.assert_array_equal(z[f'{cid}/gen'], gen)
    o = pr_oracle.oracle(case)
    for key in ('radii_real', 'radii_gen', 'pred_real', 'pred_gen'):
        np.testing.assert_array_equal(z[f'{cid}/{key}'], o[key], err_msg=key)
    assert float(z[f'{cid}/precision']) == o['precision'] and float(z[f'{cid}/recall']) == o['recall']
    # neither pass is trivially all-hit or all-miss
    assert 0.6 < o['precision'] < 0.99 and 0.7 < o['recall'] < 0.99
