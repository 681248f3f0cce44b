"""The perceptual path length metric's host side (no GPU): the CPU oracle pinned to the reference-made fixture
(tests/golden/ppl_ref.npz, make_ppl_golden.py), the percentile cut, the registration, compute_ppl's plumbing, the rank
gather, the offline CLI and the argument checks of the new C entry points.

Oracle pin: ppl_oracle.sample() on the CPU oracle generator with the fixture's tape replayed; every per-sample
distance within max(1e-4, 4 x the reference's own f32 spread) of the reference run (the spread: the reference
re-evaluated with one thread and at parameters nudged by 2^-24; floor and margin are projector_oracle's).  Measured
spreads: up to 3.1e-2 per sample at epsilon = 1e-4 in W (5.6e-2 in Z), 2.7e-4 at epsilon = 1e-2."""
import copy
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch

import ppl_oracle as pp
import projector_oracle as po
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'ppl_ref.npz')


@pytest.fixture(scope='module')
def fix():
    f = pp.load_fixture(FIXTURE)
    f['G'] = po.load_fixture(os.path.join(GOLDEN, 'projector_ref.npz'))['G']
    return f


@pytest.fixture(scope='module')
def oracle_G(fix):
    from oracle import sg2_oracle as O
    return po.build_generator(O, fix['G'])


# ---- the fixture and the oracle ----

def test_fixture_bounds_judge_something(fix):
    for case, ref in fix['cases'].items():
        (bd, sd), (bp, sp) = pp.bounds(ref)
        print(f'{case}: per-sample bound {bd:.3g} (spread {sd:.3g}), ppl bound {bp:.3g} (spread {sp:.3g})')
        assert ref['dist'].shape == (pp.CASES[case]['num_samples'],) and np.isfinite(ref['dist']).all()
        assert (ref['dist'] > 0).all()
        assert bd <= pp.MAX_BOUND, case
        if pp.CASES[case]['epsilon'] == 1e-2:
            assert bd <= pp.MAX_BOUND_E2, case


@pytest.mark.parametrize('case', list(pp.CASES))
def test_oracle_reproduces_the_reference(fix, oracle_G, case):
    ref = fix['cases'][case]
    got = pp.run_case(copy.deepcopy(oracle_G), po.stand_in(fix['det']), case, tape=ref['tape'])
    assert ref['tape'].pos == len(ref['tape'].entries), 'the oracle consumed a different number of random draws'
    pp.judge(got, ref, f'oracle {case}', with_ppl=pp.CASES[case]['num_samples'] >= 100)


# ---- the percentile cut ----

def test_ppl_from_distances(fix):
    from metrics import perceptual_path_length as ppl
    for case, ref in fix['cases'].items():
        assert ppl.ppl_from_distances(ref['dist']) == ref['ppl'], case
        n = len(ref['dist'])
        kept = np.sort(ref['dist'])[1:-1] if n >= 102 else ref['dist']     # 128 samples: one value cut at each end
        assert ppl.ppl_from_distances(ref['dist']) == pytest.approx(float(kept.mean()), rel=1e-6)
    small = np.array([3.0, 1.0, 2.0, 10.0], dtype=np.float32)
    assert ppl.ppl_from_distances(small) == 4.0, 'n < 100: nothing is cut'
    ties = np.array([1.0] * 3 + [2.0] * 194 + [9.0] * 3, dtype=np.float32)      # n = 200: ranks 1 and 198 are the cuts
    assert ppl.ppl_from_distances(ties) == pytest.approx(float(ties.mean())), 'ties with a cut value all stay'
    ramp = np.arange(200, dtype=np.float32)
    assert ppl.ppl_from_distances(ramp) == pytest.approx(float(ramp[1:199].mean()))
    assert ppl.ppl_from_distances(ramp[::-1].copy()) == ppl.ppl_from_distances(ramp)
    assert pp.ppl_from_distances(ramp) == ppl.ppl_from_distances(ramp)


# ---- registration and compute_ppl ----

def test_ppl2_wend_is_registered_with_the_reference_arguments(monkeypatch):
    from metrics import metric_main_mi_multimodal as mm
    from metrics import metric_utils, perceptual_path_length
    calls = []

    def recorder(opts, **kw):
        calls.append((opts, kw))
        return 12.5

    monkeypatch.setattr(perceptual_path_length, 'compute_ppl', recorder)
    assert mm.is_valid_metric('ppl2_wend') and 'ppl2_wend' in mm.list_valid_metrics()
    res = mm.calc_metric('ppl2_wend', G=None, num_gpus=1, rank=0, device=torch.device('cpu'),
                         mode_dict={'mode_name': 'CT', 'mode_idx': 1})
    assert res.results == {'ppl2_wend': 12.5} and res.metric == 'ppl2_wend'
    (opts, kw), = calls
    assert kw == dict(num_samples=50000, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2)
    assert isinstance(opts, metric_utils.MetricOptions) and opts.mode_dict == {'mode_name': 'CT', 'mode_idx': 1}


def test_compute_ppl_plumbing(fix, oracle_G, monkeypatch):
    """compute_ppl on the CPU (the composition, on the oracle generator): detector URL, mode_dict, the number of
    sampler calls, the cut to num_samples, and the distances against ppl_oracle.sample on the draws it used."""
    from metrics import metric_utils, precision_recall
    from metrics import perceptual_path_length as ppl
    asked = []
    det = po.stand_in(fix['det'])

    def get_detector(url, **kw):
        asked.append((url, kw))
        return det

    monkeypatch.setattr(metric_utils, 'get_feature_detector', get_detector)
    opts = metric_utils.MetricOptions(G=oracle_G, num_gpus=1, rank=0, device=torch.device('cpu'),
                                      mode_dict={'mode_name': po.MODALITIES[1], 'mode_idx': 1})
    draws = []
    torch.manual_seed(5)
    value = ppl.compute_ppl(opts, num_samples=5, epsilon=1e-2, space='w', sampling='full', crop=True, batch_size=2,
                            draws_out=draws)
    (url, kw), = asked
    assert url == precision_recall.DETECTOR_URL == ppl.DETECTOR_URL and url.endswith('/metrics/vgg16.pkl')
    assert kw['device'] == torch.device('cpu') and kw['num_gpus'] == 1 and kw['rank'] == 0
    assert len(draws) == 3, 'ceil(5 / 2) sampler calls'
    dist = torch.cat([d for _, _, d in draws])
    assert value == ppl.ppl_from_distances(dist[:5].numpy())
    G = po.build_generator(__import__('oracle.sg2_oracle', fromlist=['x']), fix['G'])
    for c, (t, z, noise), d in draws:
        assert t.shape == (2,) and z.shape == (4, G.z_dim) and len(noise) == len(pp.noise_buffers(G))
        want = pp.sample(G, det, c, 1e-2, 'w', 'full', True, mode_idx=1, draws=(t, z, noise))
        assert np.allclose(d.numpy(), want.numpy(), rtol=1e-6, atol=0)
    # the generator handed in keeps its noise; the same seed gives the same value
    assert all(torch.equal(a, torch.from_numpy(fix['G'][n])) for n, a in oracle_G.named_buffers() if 'noise_const' in n)
    torch.manual_seed(5)
    assert ppl.compute_ppl(opts, num_samples=5, epsilon=1e-2, space='w', sampling='full', crop=True, batch_size=2) == value
    # other ranks report nan
    opts.rank, opts.num_gpus = 1, 1
    assert np.isnan(ppl.compute_ppl(opts, num_samples=2, epsilon=1e-2, space='w', sampling='end', crop=False, batch_size=2))


def test_sampler_errors(fix, oracle_G):
    from metrics import perceptual_path_length as ppl
    c = torch.zeros([2, 0])
    s = ppl.PPLSampler(oracle_G, {}, 1e-2, 'w', 'end', False, po.stand_in(fix['det']))
    with pytest.raises(RuntimeError, match='mode_dict'):
        s(c)

    class NoLpips(torch.nn.Module):
        def forward(self, img, return_features: bool = False):
            return img.mean(dim=[2, 3])

    s = ppl.PPLSampler(oracle_G, {}, 1e-2, 'w', 'end', False, NoLpips(), mode_dict={'mode_name': 'a', 'mode_idx': 0})
    with pytest.raises(RuntimeError, match='SG2_PR_DETECTOR'):
        s(c)
    with pytest.raises(AssertionError):
        ppl.PPLSampler(oracle_G, {}, 1e-2, 'x', 'end', False, None)


def test_slerp():
    from metrics import perceptual_path_length as ppl
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn([5, 16], generator=g, dtype=torch.float64), torch.randn([5, 16], generator=g, dtype=torch.float64)
    t = torch.rand([5, 1], generator=g, dtype=torch.float64)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)  # noqa: E731
    assert torch.allclose(ppl.slerp(a, b, torch.zeros(5, 1, dtype=torch.float64)), unit(a), atol=1e-12)
    assert torch.allclose(ppl.slerp(a, b, torch.ones(5, 1, dtype=torch.float64)), unit(b), atol=1e-12)
    out = ppl.slerp(a, b, t)
    assert torch.allclose(out.norm(dim=-1), torch.ones(5, dtype=torch.float64), atol=1e-12)
    omega = torch.acos((unit(a) * unit(b)).sum(-1, keepdim=True))
    want = (torch.sin((1 - t) * omega) * unit(a) + torch.sin(t * omega) * unit(b)) / torch.sin(omega)
    assert torch.allclose(out, want, atol=1e-12)
    assert torch.allclose(out, pp.slerp(a, b, t), atol=1e-15)


# ---- the rank gather ----

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, paths, q):
    import sys
    sys.path[:0] = paths
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from metrics import perceptual_path_length as ppl
        local = (torch.arange(6, dtype=torch.float32).view(3, 2) + 100 * rank)       # [iters 3, B 2]
        q.put((rank, ppl.gather_distances(local, 9, world).tolist()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_gather_distances_gloo():
    from metrics import perceptual_path_length as ppl
    local = torch.arange(6, dtype=torch.float32).view(3, 2)
    assert ppl.gather_distances(local, 5, 1).tolist() == [0, 1, 2, 3, 4]
    import torch.multiprocessing as mp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, 'gan-track_amd'), root]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, paths, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=100) for _ in range(2))
    for p in procs:
        p.join(60)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    # call-major, rank-minor, then the batch; 9 of 12 kept (an uneven cut: the last call's rank 1 is dropped whole)
    want = [0, 1, 100, 101, 2, 3, 102, 103, 4]
    assert res[0] == want and res[1] == want


# ---- the CLI ----

@pytest.fixture()
def snapshot(tmp_path):
    """A run directory with training_options.json and a snapshot of a small product generator (never moved to a GPU)."""
    import legacy
    from training import networks_stylegan2 as net
    kw = dict(c_dim=0, img_resolution=16, img_channels=2, channel_base=64, channel_max=8)
    G = net.Generator(z_dim=16, w_dim=16, num_fp16_res=0, mapping_kwargs=dict(num_layers=2), **kw)
    D = net.Discriminator(num_fp16_res=0, **kw)
    run = tmp_path / 'run'
    run.mkdir()
    (run / 'training_options.json').write_text('{}')
    path = str(run / 'network-snapshot-000004.pkl')
    legacy.save_network_pkl(path, G, D, G, None, dict(class_name='training.dataset_mi_multimodal.CustomImageFolderDataset',
                                                      path='/data/from_pickle.zip', modalities=['a', 'b', 'c'], xflip=True,
                                                      use_labels=True, split='val', dtype='float32', max_size=7))
    return path


def _cli(monkeypatch):
    import calc_metrics_mi_multimodal as cli
    from metrics import metric_main_mi_multimodal as mm
    calls = []

    def calc_metric(metric, **kw):
        calls.append(dict(metric=metric, **kw))
        import dnnlib
        return dnnlib.EasyDict(results=dnnlib.EasyDict({metric: 1.5 + len(calls)}), metric=metric, total_time=0.0,
                               total_time_str='0s', num_gpus=kw['num_gpus'])

    monkeypatch.setattr(mm, 'calc_metric', calc_metric)
    monkeypatch.setattr(cli, '_device', lambda rank: torch.device('cpu'))
    return cli, calls


def test_cli_options_from_the_pickle(snapshot, monkeypatch):
    from click.testing import CliRunner
    cli, calls = _cli(monkeypatch)
    res = CliRunner().invoke(cli.calc_metrics, ['--network', snapshot, '--metrics', 'ppl2_wend,fid50k_full',
                                                '--verbose', 'False'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert [(k['metric'], k['mode_dict']) for k in calls] == [
        (m, {'mode_name': n, 'mode_idx': i}) for m in ('ppl2_wend', 'fid50k_full') for i, n in enumerate('abc')]
    for k in calls:
        d = k['dataset_kwargs']
        assert d.path == '/data/from_pickle.zip' and d.split == 'val' and d.xflip is True and d.max_size == 7
        assert d.resolution == 16 and d.use_labels is False, 'resolution and use_labels come from G'
        assert k['num_gpus'] == 1 and k['rank'] == 0 and k['device'] == torch.device('cpu') and k['cache'] is False
        assert isinstance(k['G'], torch.nn.Module) and k['G'].img_resolution == 16
        assert not any(p.requires_grad for p in k['G'].parameters()) and not k['G'].training
    run = os.path.dirname(snapshot)
    for metric in ('ppl2_wend', 'fid50k_full'):
        for n in 'abc':
            with open(os.path.join(run, f'metric-{n}-{metric}.jsonl')) as f:
                lines = [json.loads(line) for line in f]
            assert len(lines) == 1 and lines[0]['metric'] == metric and lines[0]['mode'] == n
            assert lines[0]['snapshot_pkl'] == 'network-snapshot-000004.pkl' and np.isfinite(lines[0]['results'][metric])
    assert res.output.count('"metric": "ppl2_wend"') == 3


def test_cli_options_from_the_command_line(snapshot, tmp_path, monkeypatch):
    from click.testing import CliRunner
    cli, calls = _cli(monkeypatch)
    moved = str(tmp_path / 'elsewhere.pkl')       # no training_options.json next to it: nothing is appended
    os.replace(snapshot, moved)
    res = CliRunner().invoke(cli.calc_metrics, ['--network', moved, '--metrics', 'pr50k3_full', '--data', '/data/cli.zip',
                                                '--modalities', 'x, y', '--split', 'test', '--mirror', '1',
                                                '--metrics_cache', 'True'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert [k['mode_dict'] for k in calls] == [{'mode_name': 'x', 'mode_idx': 0}, {'mode_name': 'y', 'mode_idx': 1}]
    d = calls[0]['dataset_kwargs']
    assert (d.path, d.split, d.xflip, d.modalities, d.max_size, d.dtype) == ('/data/cli.zip', 'test', True, ['x', 'y'],
                                                                             None, 'float32')
    assert d.class_name == 'training.dataset_mi_multimodal.CustomImageFolderDataset' and d.resolution == 16
    assert calls[0]['cache'] is True
    assert not [f for f in os.listdir(tmp_path) if f.endswith('.jsonl')]
    assert 'Dataset options:' in res.output and '"metric": "pr50k3_full"' in res.output


def test_cli_failures(snapshot, tmp_path, monkeypatch):
    from click.testing import CliRunner
    from metrics import metric_main_mi_multimodal as mm
    cli, calls = _cli(monkeypatch)
    res = CliRunner().invoke(cli.calc_metrics, ['--network', snapshot, '--metrics', 'ppl2_wend,kid50k_full'])
    assert res.exit_code != 0 and 'kid50k_full' in res.output and not calls
    assert all(name in res.output for name in mm.list_valid_metrics())
    res = CliRunner().invoke(cli.calc_metrics, ['--network', str(tmp_path / 'absent.pkl')])
    assert res.exit_code != 0 and '--network' in res.output
    res = CliRunner().invoke(cli.calc_metrics, ['--network', snapshot, '--gpus', '0'])
    assert res.exit_code != 0 and '--gpus' in res.output
    import legacy
    with open(snapshot, 'rb') as f:
        data = legacy.load_network_pkl(f)
    bare = str(tmp_path / 'bare.pkl')
    legacy.save_network_pkl(bare, data['G'], data['D'], data['G_ema'], None, None)
    res = CliRunner().invoke(cli.calc_metrics, ['--network', bare])
    assert res.exit_code != 0 and '--data' in res.output and not calls


# ---- the new C entry points: argument checks only, no device work ----

def test_ppl_symbols_and_argument_errors():
    import sg2hip
    L = sg2hip.lib()
    assert L.sg2_abi_version() == 11 == sg2hip.ABI_VERSION
    for name in ('sg2_ppl_prep', 'sg2_lpips_pair_dist', 'sg2_lpips_pair_dist_scratch_bytes'):
        assert hasattr(L, name) and name in sg2hip.SIGNATURES
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below fails its argument checks first
    err = lambda: L.sg2_last_error()  # noqa: E731
    # sg2_ppl_prep(out, img, N, C, H, W, channel, crop, factor, stream)
    bad = [((None, p, 1, 1, 8, 8, -1, 0, 1), b'non-null'), ((p, None, 1, 1, 8, 8, -1, 0, 1), b'non-null'),
           ((p, p, 0, 1, 8, 8, -1, 0, 1), b'at least 1'), ((p, p, 1, 1, 8, 8, -1, 0, 0), b'factor'),
           ((p, p, 1, 1, 8, 8, -1, 0, 3), b'divide'), ((p, p, 1, 1, 24, 24, -1, 1, 8), b'divide'),
           ((p, p, 1, 2, 8, 8, -1, 0, 1), b'C = 1 or C = 3'), ((p, p, 1, 4, 8, 8, -1, 0, 1), b'C = 1 or C = 3'),
           ((p, p, 1, 2, 8, 8, 2, 0, 1), b'channel'), ((p, p, 1, 2, 8, 8, -2, 0, 1), b'channel'),
           ((p, p, 1, 1, 8, 16, -1, 1, 1), b'square'), ((p, p, 1, 1, 12, 12, -1, 1, 1), b'H % 8'),
           ((p, p, 1, 1, 8, 8, -1, 2, 1), b'crop')]
    for args, msg in bad:
        assert L.sg2_ppl_prep(*args, None) != 0 and msg in err(), (args, err())
    # sg2_lpips_pair_dist(dist, feats, B, F, eps, scratch, scratch_bytes, stream)
    nbytes = ctypes.c_int64(-1)
    assert L.sg2_lpips_pair_dist_scratch_bytes(ctypes.byref(nbytes), 2, 7995392) == 0
    assert nbytes.value == 4 * 2 * 976 and 976 == 7995392 // 8192, 'one partial per 8192-element chunk and pair'
    assert L.sg2_lpips_pair_dist_scratch_bytes(ctypes.byref(nbytes), 3, 8193) == 0 and nbytes.value == 4 * 3 * 2
    assert L.sg2_lpips_pair_dist_scratch_bytes(None, 1, 1) != 0 and b'non-null' in err()
    assert L.sg2_lpips_pair_dist_scratch_bytes(ctypes.byref(nbytes), 0, 1) != 0 and b'B must' in err()
    assert L.sg2_lpips_pair_dist_scratch_bytes(ctypes.byref(nbytes), 1, 0) != 0 and b'F must' in err()
    bad = [((None, p, 1, 8, 1e-4, p, 4), b'non-null'), ((p, None, 1, 8, 1e-4, p, 4), b'non-null'),
           ((p, p, 1, 8, 1e-4, None, 4), b'non-null'), ((p, p, 0, 8, 1e-4, p, 4), b'B must'),
           ((p, p, 1, 0, 1e-4, p, 4), b'F must'), ((p, p, 1, 8, 0.0, p, 4), b'eps'), ((p, p, 1, 8, -1.0, p, 4), b'eps'),
           ((p, p, 2, 8193, 1e-4, p, 15), b'scratch too small')]
    for args, msg in bad:
        assert L.sg2_lpips_pair_dist(*args, None) != 0 and msg in err(), (args, err())


def test_ops_refuse_cpu_tensors_and_document_the_tree():
    from torch_utils.ops import ppl as ops
    with pytest.raises(RuntimeError, match='ROCm'):
        ops.prep_images(torch.zeros(2, 1, 8, 8))
    with pytest.raises(RuntimeError, match='ROCm'):
        ops.pair_distances(torch.zeros(2, 16), 1e-4)
    assert ops.pair_dist_tree(1) == (9, 18) and ops.pair_dist_tree(8192 * 256) == (9, 18)
    assert ops.pair_dist_tree(8192 * 256 + 1) == (10, 18) and ops.pair_dist_tree(7995392) == (12, 18)
    # the compositions are the reference's arithmetic on any device
    x = torch.linspace(-1, 1, 2 * 2 * 16 * 16).view(2, 2, 16, 16)
    y = ops.prep_images_ref(x, channel=1, crop=True, factor=2)
    want = ((x[:, 1:2, 6:14, 4:12].reshape(2, 1, 4, 2, 4, 2).mean([3, 5]) + 1) * 127.5).repeat(1, 3, 1, 1)
    assert y.shape == (2, 3, 4, 4) and torch.equal(y, want)
    f = torch.arange(12.).view(4, 3)
    assert torch.allclose(ops.pair_distances_ref(f, 0.5), torch.tensor([108.0 * 4, 108.0 * 4]))
