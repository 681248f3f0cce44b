"""SSIM / MSE scoring without a GPU: the oracle against itself and against a planted float32 fault, the torch
composition against the oracle, the C entry points' argument checks (no device work), the op's refusals, and the
score_projections plumbing on a CPU generator with ssim_mse stubbed by the oracle.  Bounds: tests/ssim_oracle.py."""
import collections
import csv
import ctypes
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

import ssim_oracle as so

# the GPU tests' shapes: every tile edge per axis, both at 2 TILE + 1, and the two whole images
SHAPES = [(3, 2, oh + 10, ow + 10) for oh, ow in
          [(1, 32), (15, 32), (16, 32), (17, 32), (16, 1), (16, 31), (16, 33), (33, 65)]] + \
         [(1, 1, 256, 256), (1, 1, 1024, 1024)]


# ---- the oracle ----

def test_oracle_direct_and_separable_agree():
    for shape in [(3, 2, 26, 42), (1, 1, 11, 11), (1, 1, 256, 256)]:
        x, y = so.smooth_pair(shape)
        out, smap = so.reference('smooth', shape)
        out_d, smap_d = so.ssim_mse(x, y, form='direct')
        assert np.abs(smap - smap_d).max() <= so.SSIM_TOL and np.abs(out - out_d)[..., 0].max() <= so.SSIM_TOL
        assert np.array_equal(out[..., 1], out_d[..., 1])
    x, y = so.flat_pair()
    assert np.abs(so.ssim_map(x, y) - so.ssim_map(x, y, form='direct')).max() <= so.SSIM_TOL


def test_oracle_closed_forms():
    g = so.gaussian_window()
    assert g.shape == (11,) and g.dtype == np.float64 and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    assert g[5] / g[4] == pytest.approx(math.exp(1 / 4.5), rel=1e-14)
    for a, b, L in [(200.0, 180.0, 255.0), (0.0, 255.0, 255.0), (0.25, 0.75, 1.0)]:
        x, y = np.full((1, 1, 20, 23), a, np.float32), np.full((1, 1, 20, 23), b, np.float32)
        out, smap = so.ssim_mse(x, y, L)
        c1 = (0.01 * L) ** 2
        assert smap.shape == (1, 1, 10, 13)
        assert np.abs(smap - (2 * a * b + c1) / (a * a + b * b + c1)).max() <= so.SSIM_TOL
        assert out[0, 0, 1] == (a - b) ** 2
    for x in (so.smooth_pair((2, 2, 30, 45))[0], so.flat_pair()[0], so.integer_pair()[0]):
        out, smap = so.ssim_mse(x, x.copy())
        assert (smap == 1.0).all() and (out[..., 0] == 1.0).all() and (out[..., 1] == 0.0).all()


@pytest.mark.parametrize('name,shape', [('flat', (1, 1, 64, 64)), ('smooth', (1, 1, 256, 256))])
def test_float32_moments_violate_the_bound(name, shape):
    """The planted fault: the same code with the moments in float32 misses by far more than SSIM_TOL."""
    x, y = (so.flat_pair if name == 'flat' else so.smooth_pair)(shape)
    out, smap = so.reference(name, shape)
    out32, smap32 = so.ssim_mse(x, y, dtype=np.float32)
    e_mean, e_map = abs(out32[0, 0, 0] - out[0, 0, 0]), np.abs(smap32 - smap).max()
    print(f'{name} {shape}: float32 moments miss the mean by {e_mean:.3g}, the map by {e_map:.3g} '
          f'(bound {so.SSIM_TOL:.3g})')
    assert e_mean > 10 * so.SSIM_TOL and e_map > 10 * so.SSIM_TOL


# ---- the composition ----

def _judge(out, smap, want_out, want_map, what):
    e_ssim = np.abs(out[..., 0] - want_out[..., 0]).max()
    e_map = np.abs(smap.astype(np.float64) - want_map).max()
    e_mse = (np.abs(out[..., 1] - want_out[..., 1]) / want_out[..., 1]).max()
    print(f'{what}: mean SSIM {e_ssim:.3g}, map {e_map:.3g}, MSE rel {e_mse:.3g}')
    assert e_ssim <= so.SSIM_TOL and e_map <= so.MAP_TOL and e_mse <= so.MSE_REL, what


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_composition_on_cpu_tensors(shape):
    from torch_utils.ops import ssim
    x, y = so.smooth_pair(shape)
    want_out, want_map = so.reference('smooth', shape)
    out, smap = ssim.ssim_mse_ref(torch.tensor(x), torch.tensor(y), want_map=True)
    assert out.dtype == torch.float64 and smap.dtype == torch.float32 and tuple(out.shape) == shape[:2] + (2,)
    _judge(out.numpy(), smap.numpy(), want_out, want_map, f'{shape}')
    assert torch.equal(ssim.ssim_mse_ref(torch.tensor(x), torch.tensor(y)), out)


def test_composition_other_fixtures():
    from torch_utils.ops import ssim
    for name, pair, L in (('flat', so.flat_pair(), 255.0), ('integer', so.integer_pair(), 255.0),
                          ('unit', so.unit_pair(), 1.0)):
        x, y = pair
        want_out, want_map = so.reference(name, x.shape, L)
        out, smap = ssim.ssim_mse_ref(torch.tensor(x), torch.tensor(y), data_range=L, want_map=True)
        _judge(out.numpy(), smap.numpy(), want_out, want_map, name)


def test_window_and_psnr():
    from torch_utils.ops import ssim
    assert np.array_equal(ssim.gaussian_window(), so.gaussian_window()) and ssim.gaussian_window().dtype == np.float64
    assert ssim.psnr(0.0) == math.inf and ssim.psnr(0.0, 1.0) == math.inf
    assert ssim.psnr(255.0 ** 2) == 0.0 and ssim.psnr(65.025) == pytest.approx(30.0, abs=1e-12)
    assert ssim.psnr(0.01, 1.0) == pytest.approx(20.0, abs=1e-12)


# ---- the C entry points: symbols and argument checks only, no device work ----

def test_ssim_symbols_and_argument_errors():
    import sg2hip
    L = sg2hip.lib()
    assert L.sg2_abi_version() == 11, 'additive entry points: the ABI version stays'
    for name in ('sg2_ssim_scratch_bytes', 'sg2_ssim_mse'):
        assert hasattr(L, name) and name in sg2hip.SIGNATURES
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below fails its argument checks first
    win = (ctypes.c_double * 11)(*so.gaussian_window().tolist())
    nbytes = ctypes.c_int64(-1)

    def call(out=p, x=p, y=p, N=1, C=1, H=32, W=32, window=win, L_=255.0, scratch=p, sb=1 << 20):
        return L.sg2_ssim_mse(out, p, x, y, N, C, H, W, window, L_, scratch, sb, None)

    bad = [(dict(out=None), b'non-null'), (dict(x=None), b'non-null'), (dict(y=None), b'non-null'),
           (dict(window=None), b'non-null'), (dict(scratch=None), b'non-null'),
           (dict(N=0), b'N and C must be >= 1'), (dict(C=0), b'N and C must be >= 1'), (dict(N=-3), b'N and C'),
           (dict(H=10), b'11..1024'), (dict(H=1025), b'11..1024'), (dict(W=10), b'11..1024'), (dict(W=1025), b'11..1024'),
           (dict(L_=0.0), b'data_range'), (dict(L_=-1.0), b'data_range'), (dict(L_=float('nan')), b'data_range'),
           (dict(sb=15), b'scratch too small'), (dict(N=3, C=2, H=43, W=75, sb=3 * 2 * 9 * 16 - 1), b'scratch too small')]
    for kw, msg in bad:
        rc = call(**kw)
        assert rc == -1 and msg in L.sg2_last_error(), (kw, rc, L.sg2_last_error())
    for (N, C, H, W), msg in {(0, 1, 32, 32): b'N and C', (1, 1, 10, 32): b'11..1024', (1, 1, 32, 2000): b'11..1024'}.items():
        assert L.sg2_ssim_scratch_bytes(ctypes.byref(nbytes), N, C, H, W) == -1 and msg in L.sg2_last_error()
    assert L.sg2_ssim_scratch_bytes(None, 1, 1, 32, 32) == -1 and b'non-null' in L.sg2_last_error()


def test_scratch_bytes_formula():
    import sg2hip
    from torch_utils.ops import ssim
    L = sg2hip.lib()
    nbytes = ctypes.c_int64(-1)
    th, tw = ssim.TILE_H, ssim.TILE_W
    # two float64 partial sums per output tile and pair
    for (N, C, H, W), tiles in {(1, 1, 11, 11): 1, (3, 2, 43, 75): 3 * 3, (8, 2, 1024, 1024): 64 * 32}.items():
        assert tiles == -(-(H - 10) // th) * -(-(W - 10) // tw)
        assert L.sg2_ssim_scratch_bytes(ctypes.byref(nbytes), N, C, H, W) == 0
        assert nbytes.value == N * C * tiles * 16, (N, C, H, W)


def test_op_refusals():
    from torch_utils.ops import ssim
    x = torch.zeros([1, 2, 16, 16])
    with pytest.raises(RuntimeError, match='ROCm'):
        ssim.ssim_mse(x, x)
    with pytest.raises(RuntimeError, match='one shape'):
        ssim.ssim_mse(x, torch.zeros([1, 2, 16, 17]))
    with pytest.raises(RuntimeError, match='float32'):
        ssim.ssim_mse(x, x.double())
    with pytest.raises(RuntimeError, match='float32'):
        ssim.ssim_mse_ref(x.to(torch.uint8), x)
    with pytest.raises(RuntimeError, match='11..1024'):
        ssim.ssim_mse_ref(torch.zeros([1, 1, 10, 16]), torch.zeros([1, 1, 10, 16]))
    with pytest.raises(RuntimeError, match='data_range'):
        ssim.ssim_mse_ref(x, x, data_range=0.0)


# ---- score_projections on a CPU generator, ssim_mse stubbed by the oracle ----

def _oracle_stub(calls):
    def stub(x, y, data_range=255.0, want_map=False):
        calls.append((tuple(x.shape), float(data_range), bool(want_map)))
        assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape
        out, smap = so.ssim_mse(x.numpy(), y.numpy(), data_range)
        out = torch.from_numpy(out)
        return (out, torch.from_numpy(smap.astype(np.float32))) if want_map else out
    return stub


@pytest.fixture()
def projection_run(tmp_path, monkeypatch):
    """A fabricated projection run: a synthetic two-modality zip at 32^2, the oracle generator on the CPU, and w of
    mapped seeds for every second slice."""
    import projector_oracle as po
    import synth_zip
    from oracle import sg2_oracle as O
    from genlib import run_projector_mi_multimodal as pcli
    from genlib.projector import score
    from metrics import metric_utils
    monkeypatch.setattr(score, '_device', lambda: torch.device('cpu'))
    monkeypatch.setattr(metric_utils, '_detectors', {})
    for var in ('SG2_LPIPS_DETECTOR', 'SG2_PR_DETECTOR'):
        monkeypatch.delenv(var, raising=False)
    calls = []
    monkeypatch.setattr(score.ssim_op, 'ssim_mse', _oracle_stub(calls))
    data = str(tmp_path / 'data.zip')
    names = synth_zip.make_zip(data, modalities=tuple(po.MODALITIES), res=32, patients=2, slices=3)
    c, _, _, _ = pcli.build_config(data=data, outdir=str(tmp_path / 'reports'), gpus=1, experiment='00002',
                                   network_pkl='network-snapshot-000004.pkl', modalities=','.join(po.MODALITIES))
    G = po.build_generator(O)
    keys = [(n.split('/')[0], n.split('/')[1][-12:-7]) for n in names[::2]]
    with torch.no_grad():
        ws = G.mapping(torch.from_numpy(np.random.RandomState(5).randn(len(keys), G.z_dim)), None).float().numpy()
    run = tmp_path / 'run'
    run.mkdir()
    with open(run / 'training_options.json', 'wt') as f:
        json.dump(c, f, indent=2)
    return dict(run=run, data=data, names=names, keys=keys, ws=ws, G=G, calls=calls, modalities=list(po.MODALITIES))


def _dump(run, projected):
    with open(run / 'projected_w', 'wb') as f:
        pickle.dump(projected, f, protocol=pickle.HIGHEST_PROTOCOL)


def _plain(keys, ws):
    projected = {}
    for (p, s), w in zip(keys, ws):
        projected.setdefault(p, {})[s] = w
    return projected


def test_score_run_rows_and_summary(projection_run):
    import io
    import zipfile
    from genlib.projector import score
    from training.dataset_mi_multimodal import safe_load_pickle
    r = projection_run
    # stored out of dataset order: the rows follow the dataset, not the pickle
    _dump(r['run'], _plain(r['keys'][::-1], r['ws'][::-1]))
    rows, summary = score.score_run(str(r['run']), batch=2, maps=True, G=r['G'])
    assert r['calls'] == [((2, 2, 32, 32), 255.0, True), ((1, 2, 32, 32), 255.0, True)], 'one call per batch'
    with zipfile.ZipFile(r['data']) as z:
        targets = np.stack([np.stack([safe_load_pickle(io.BytesIO(z.read(f'train/{n}')))[m] for m in r['modalities']])
                            for n in r['names'][::2]]).astype(np.float32)
    ws = torch.from_numpy(r['ws'])          # (rendered in the tool's own batches: a batch changes the last bits)
    images = torch.cat([score.render(r['G'], ws[:2]), score.render(r['G'], ws[2:])]).numpy()
    assert images.dtype == np.float32 and images.min() >= 0 and images.max() <= 255
    want, want_map = so.ssim_mse(images, targets)
    with open(r['run'] / 'reconstruction.csv') as f:
        got = list(csv.DictReader(f))
    assert list(got[0]) == ['patient', 'slice', 'modality', 'mse', 'psnr', 'ssim']
    assert [(g['patient'], g['slice'], g['modality']) for g in got] == \
        [(p, s, m) for p, s in r['keys'] for m in r['modalities']], 'dataset order'
    for i, g in enumerate(got):
        b, ch = divmod(i, 2)
        assert float(g['ssim']) == want[b, ch, 0] and float(g['mse']) == want[b, ch, 1], 'full precision in the CSV'
        assert float(g['psnr']) == 10 * math.log10(255.0 ** 2 / want[b, ch, 1])
        assert rows[i]['ssim'] == want[b, ch, 0]
    with open(r['run'] / 'reconstruction.json') as f:
        saved = json.load(f)
    assert saved['modalities'] == summary and saved['slices'] == 3 and list(summary) == r['modalities']
    for ch, m in enumerate(r['modalities']):
        e = summary[m]
        assert e['count'] == 3 and e['psnr']['count_infinite'] == 0
        for k, col in (('ssim', 0), ('mse', 1)):
            v = want[:, ch, col]
            assert e[k] == {'mean': float(v.mean()), 'std': float(v.std()), 'min': float(v.min()), 'max': float(v.max())}
        assert e['psnr']['mean_finite'] == pytest.approx(np.mean(10 * np.log10(255.0 ** 2 / want[:, ch, 1])), rel=1e-12)
    import PIL.Image
    p, s = r['keys'][2]
    png = np.array(PIL.Image.open(r['run'] / p / r['modalities'][0] / 'ssim_map' / f'map_{s}.png'))
    assert png.shape == (22, 22) and png.dtype == np.uint8
    grey = np.round(np.clip(want_map[2, 0].astype(np.float32), 0, 1) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(png, grey)


def test_score_run_reads_a_reference_style_pickle(projection_run):
    from genlib.projector import score
    from genlib.utils import util_general
    r = projection_run
    nested = util_general.nested_dict()
    for (p, s), w in zip(r['keys'], r['ws']):
        nested[p][s] = w
    _dump(r['run'], nested)         # a defaultdict whose factory is genlib.utils.util_general.nested_dict
    assert b'nested_dict' in (r['run'] / 'projected_w').read_bytes()
    loaded = score.load_projected_w(str(r['run'] / 'projected_w'))
    assert type(loaded) is dict and all(type(v) is dict for v in loaded.values())
    assert [(p, s) for p, v in loaded.items() for s in v] == r['keys']
    assert all(np.array_equal(loaded[p][s], w) for (p, s), w in zip(r['keys'], r['ws']))
    rows, _ = score.score_run(str(r['run']), batch=16, G=r['G'])
    assert len(rows) == 6 and r['calls'] == [((3, 2, 32, 32), 255.0, False)]


def test_projected_w_refuses_other_globals(projection_run):
    from genlib.projector import score
    r = projection_run
    _dump(r['run'], {'p000': {'00000': os.system}})
    with pytest.raises(pickle.UnpicklingError, match=r'(posix|os|nt)\.system'):
        score.load_projected_w(str(r['run'] / 'projected_w'))
    _dump(r['run'], collections.OrderedDict(p000={'00000': collections.Counter()}))
    with pytest.raises(pickle.UnpicklingError, match=r'collections\.Counter'):
        score.score_run(str(r['run']), G=r['G'])


def test_unknown_slice_key_is_an_error(projection_run):
    from genlib.projector import score
    r = projection_run
    projected = _plain(r['keys'], r['ws'])
    projected['p001']['00077'] = r['ws'][0]
    _dump(r['run'], projected)
    with pytest.raises(RuntimeError, match=r"no item in the dataset.*'p001', '00077'"):
        score.score_run(str(r['run']), G=r['G'])
    assert not r['calls'] and not os.path.exists(r['run'] / 'reconstruction.csv')


def test_cli_lpips_without_detector_and_moved_files(projection_run):
    from click.testing import CliRunner
    from genlib import score_projections as cli
    r = projection_run
    _dump(r['run'], _plain(r['keys'], r['ws']))
    res = CliRunner().invoke(cli.main, ['--run', str(r['run']), '--lpips', '--network', 'unused.pkl'])
    assert res.exit_code != 0 and 'SG2_LPIPS_DETECTOR or SG2_PR_DETECTOR' in res.output, res.output
    # without G the snapshot must be named: training_options.json holds none here
    res = CliRunner().invoke(cli.main, ['--run', str(r['run'])])
    assert res.exit_code != 0 and '--network' in res.output, res.output
    res = CliRunner().invoke(cli.main, ['--run', str(r['run']), '--data', str(r['run'] / 'moved.zip')])
    assert res.exit_code != 0
    assert not r['calls']


def test_psnr_is_infinite_at_zero_mse_and_counted(projection_run, monkeypatch):
    from genlib.projector import score
    r = projection_run
    _dump(r['run'], _plain(r['keys'], r['ws']))
    inner = score.ssim_op.ssim_mse

    def exact_first(x, y, data_range=255.0, want_map=False):
        out = inner(x, y, data_range, want_map).clone()
        out[0, 1] = torch.tensor([1.0, 0.0], dtype=torch.float64)     # the first slice's second modality: a perfect hit
        return out

    monkeypatch.setattr(score.ssim_op, 'ssim_mse', exact_first)
    rows, summary = score.score_run(str(r['run']), batch=16, G=r['G'])
    assert rows[1]['psnr'] == math.inf and all(math.isfinite(x['psnr']) for i, x in enumerate(rows) if i != 1)
    with open(r['run'] / 'reconstruction.csv') as f:
        got = list(csv.DictReader(f))
    assert got[1]['psnr'] == 'inf' and float(got[1]['mse']) == 0.0
    m0, m1 = r['modalities']
    assert summary[m1]['psnr']['count_infinite'] == 1 and summary[m0]['psnr']['count_infinite'] == 0
    assert summary[m1]['psnr']['mean_finite'] == pytest.approx(np.mean([rows[3]['psnr'], rows[5]['psnr']]), rel=1e-12)
    with open(r['run'] / 'reconstruction.json') as f:
        json.load(f)        # strict JSON: no Infinity token
