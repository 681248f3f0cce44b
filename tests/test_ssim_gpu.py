"""The fused SSIM / MSE kernel (sg2_ssim_mse, torch_utils/ops/ssim.py) on the GPU against the float64 oracle
(tests/ssim_oracle.py, whose docstring derives SSIM_TOL, MAP_TOL and MSE_REL), and score_projections end to end.
Outputs, map and scratch are NaN-poisoned: an element the kernel does not write fails every judge."""
import csv
import json
import os
import pickle

import numpy as np
import pytest
import torch

import poison
import ssim_oracle as so

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(autouse=True)
def _poisoned(monkeypatch):
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.ssim'])
    monkeypatch.delenv('SG2_SSIM_FUSED', raising=False)


def _tiles():
    from torch_utils.ops import ssim
    assert (ssim.TILE_H, ssim.TILE_W) == (16, 32), 'the extents below are written for this tile'
    return ssim.TILE_H, ssim.TILE_W


def _dev(*arrays):
    return [torch.tensor(a, device=DEV) for a in arrays]        # (a copy: the fixtures are read-only)


def _judge(out, smap, want_out, want_map, what):
    out, smap = out.cpu().numpy(), smap.cpu().numpy().astype(np.float64)
    assert out.dtype == np.float64 and out.shape == want_out.shape and smap.shape == want_map.shape
    assert not np.isnan(out).any() and not np.isnan(smap).any(), f'{what}: an element was never written'
    e_ssim = np.abs(out[..., 0] - want_out[..., 0]).max()
    e_map = np.abs(smap - want_map).max()
    e_mse = (np.abs(out[..., 1] - want_out[..., 1]) / np.maximum(want_out[..., 1], 1e-300)).max()
    print(f'{what}: mean SSIM {e_ssim:.3g} (bound {so.SSIM_TOL:.3g}), map {e_map:.3g} (bound {so.MAP_TOL:.3g}), '
          f'MSE rel {e_mse:.3g} (bound {so.MSE_REL:.3g})')
    assert e_ssim <= so.SSIM_TOL and e_map <= so.MAP_TOL and e_mse <= so.MSE_REL, what


# one case per tile edge per axis (1, TILE - 1, TILE, TILE + 1 valid positions), both axes at 2 TILE + 1
EXTENTS = [(1, 32), (15, 32), (16, 32), (17, 32), (16, 1), (16, 31), (16, 33), (33, 65)]


@pytest.mark.parametrize('oh,ow', EXTENTS)
def test_extents(oh, ow):
    from torch_utils.ops import ssim
    th, tw = _tiles()
    assert oh in (1, th - 1, th, th + 1, 2 * th + 1) and ow in (1, tw - 1, tw, tw + 1, 2 * tw + 1)
    shape = (3, 2, oh + 10, ow + 10)
    x, y = so.smooth_pair(shape)
    want_out, want_map = so.reference('smooth', shape)
    out, smap = ssim.ssim_mse(*_dev(x, y), want_map=True)
    assert smap.dtype == torch.float32 and tuple(out.shape) == (3, 2, 2)
    _judge(out, smap, want_out, want_map, f'{shape}')
    assert len({float(v) for v in out[..., 0].flatten()}) == 6, 'distinct content per (n, c)'


@pytest.mark.parametrize('size', [256, 1024])
def test_whole_images(size):
    from torch_utils.ops import ssim
    shape = (1, 1, size, size)
    x, y = so.smooth_pair(shape)
    want_out, want_map = so.reference('smooth', shape)
    out, smap = ssim.ssim_mse(*_dev(x, y), want_map=True)
    _judge(out, smap, want_out, want_map, f'{shape}')


def test_more_pairs_than_grid_planes():
    """N C above 65535: a workgroup takes a second (n, c) in its loop, the only size at which it does."""
    from torch_utils.ops import ssim
    base = (251, 1, 11, 12)             # 251 distinct pairs, repeated: 65535 mod 251 != 0, so a pair off by a grid's
    idx = np.arange(65535 + 2) % 251    # worth of planes would be another pair's values
    x, y = [a[idx] for a in so.smooth_pair(base)]
    want_out, want_map = [a[idx] for a in so.reference('smooth', base)]
    out, smap = ssim.ssim_mse(*_dev(x, y), want_map=True)
    _judge(out, smap, want_out, want_map, f'{x.shape}')
    assert torch.equal(ssim.ssim_mse(*_dev(x[-2:], y[-2:])), out[-2:]), 'the looped pairs alone as in the batch'


def test_exact_cases():
    from torch_utils.ops import ssim
    x, y = so.integer_pair()
    out = ssim.ssim_mse(*_dev(x, y)).cpu().numpy()
    d = x.astype(np.float64) - y.astype(np.float64)
    want = (d * d).mean(axis=(2, 3))
    assert (d * d).sum() < 2.0 ** 53 and np.array_equal(out[..., 1], want), 'sums of integers are exact in any order'
    want_out, _ = so.reference('integer', x.shape)
    assert np.abs(out[..., 0] - want_out[..., 0]).max() <= so.SSIM_TOL
    # x against itself: numerator and denominator are the same bits
    xs, _ = so.smooth_pair((2, 2, 45, 77))
    xd, = _dev(xs)
    out, smap = ssim.ssim_mse(xd, xd.clone(), want_map=True)
    assert torch.equal(out, torch.tensor([1.0, 0.0], dtype=torch.float64, device=DEV).expand(2, 2, 2))
    assert torch.equal(smap, torch.ones_like(smap))


def test_determinism():
    from torch_utils.ops import ssim
    shape = (3, 2, 43, 75)
    x, y = _dev(*so.smooth_pair(shape))
    out, smap = ssim.ssim_mse(x, y, want_map=True)
    out2, smap2 = ssim.ssim_mse(x, y, want_map=True)
    assert torch.equal(out, out2) and torch.equal(smap, smap2), 'two calls give the same bits'
    for n in range(shape[0]):
        o1, m1 = ssim.ssim_mse(x[n:n + 1, 1:2].contiguous(), y[n:n + 1, 1:2].contiguous(), want_map=True)
        assert torch.equal(o1[0, 0], out[n, 1]) and torch.equal(m1[0, 0], smap[n, 1]), 'alone as in the batch'
    nomap = ssim.ssim_mse(x, y, want_map=False)
    assert isinstance(nomap, torch.Tensor) and torch.equal(nomap, out), 'the map does not change out'


def test_data_range_one():
    from torch_utils.ops import ssim
    x, y = so.unit_pair()
    want_out, want_map = so.reference('unit', x.shape, 1.0)
    out, smap = ssim.ssim_mse(*_dev(x, y), data_range=1.0, want_map=True)
    _judge(out, smap, want_out, want_map, 'data_range = 1')
    assert np.abs(want_out[..., 0] - so.reference('unit', x.shape, 255.0)[0][..., 0]).min() > 1e-3, \
        'the fixture tells the two ranges apart'


def test_composition_on_the_device():
    """ssim_mse_ref on ROCm tensors (what SG2_SSIM_FUSED=0 runs) is within the same bounds."""
    from torch_utils.ops import ssim
    shape = (3, 2, 27, 75)
    x, y = so.smooth_pair(shape)
    want_out, want_map = so.reference('smooth', shape)
    with poison.unpoisoned(['torch_utils.ops.ssim']):
        out, smap = ssim.ssim_mse_ref(*_dev(x, y), want_map=True)
    _judge(out, smap, want_out, want_map, f'composition {shape}')


# ---- end to end ----

MODALITIES = ['MR_nonrigid_CT', 'MR_MR_T2']


def _read_rows(run):
    with open(os.path.join(run, 'reconstruction.csv')) as f:
        return list(csv.DictReader(f))


def _fabricate(tmp_path):
    """A 16^2 two-modality generator saved as a snapshot, a synthetic zip, the run's options and a projected_w of mapped
    seeds for every second slice, as a run with --step_patient_slice 2 would leave them."""
    import synth_zip
    import legacy
    from genlib import run_projector_mi_multimodal as pcli
    from training import networks_stylegan2 as net
    data = str(tmp_path / 'data.zip')
    names = synth_zip.make_zip(data, modalities=tuple(MODALITIES), res=16, patients=2, slices=3)
    kw = dict(c_dim=0, img_resolution=16, img_channels=2, channel_base=64, channel_max=8)
    torch.manual_seed(3)
    G = net.Generator(z_dim=16, w_dim=16, num_fp16_res=0, mapping_kwargs=dict(num_layers=2), **kw)
    D = net.Discriminator(num_fp16_res=0, **kw)
    snapshot = str(tmp_path / 'network-snapshot-000004.pkl')
    legacy.save_network_pkl(snapshot, G, D, G, None, dict(path=data, modalities=MODALITIES))
    c, _, _, _ = pcli.build_config(data=data, outdir=str(tmp_path / 'reports'), gpus=1, experiment='00002',
                                   network_pkl='network-snapshot-000004.pkl', modalities=','.join(MODALITIES))
    c.projector_kwargs.outdir_model = snapshot
    keys = [(n.split('/')[0], n.split('/')[1][-12:-7]) for n in names[::2]]     # every second slice, as a run would
    with torch.no_grad():
        ws = G.to(DEV).mapping(torch.from_numpy(np.random.RandomState(5).randn(len(keys), 16)).to(DEV), None).cpu().numpy()
    projected = {}
    for (p, s), w in zip(keys, ws):
        projected.setdefault(p, {})[s] = w.astype(np.float32)

    def make_run(name):
        run = tmp_path / name
        run.mkdir()
        with open(run / 'training_options.json', 'wt') as f:
            json.dump(c, f, indent=2)
        with open(run / 'projected_w', 'wb') as f:
            pickle.dump(projected, f, protocol=pickle.HIGHEST_PROTOCOL)
        return run

    return data, names, keys, make_run


def test_score_projections_end_to_end(tmp_path, monkeypatch):
    """score_projections with the kernel and with SG2_SSIM_FUSED=0 on the same rendered images (the second run is
    handed the first run's images, so the rows compare the two SSIM paths and nothing else), and the kernel's rows
    against the oracle on those images."""
    from click.testing import CliRunner
    from genlib import score_projections as cli
    from genlib.projector import score
    data, names, keys, make_run = _fabricate(tmp_path)
    rendered = []
    real_render = score.render
    rows = {}
    for fused in (True, False):
        run = make_run('fused' if fused else 'composition')
        if fused:
            def render(G_, ws_):
                rendered.append(real_render(G_, ws_))
                return rendered[-1]
        else:
            monkeypatch.setenv('SG2_SSIM_FUSED', '0')
            replay = iter(rendered)

            def render(G_, ws_):
                return next(replay)
        monkeypatch.setattr(score, 'render', render)
        res = CliRunner().invoke(cli.main, ['--run', str(run), '--batch', '2'] + (['--maps'] if fused else []),
                                 catch_exceptions=False)
        assert res.exit_code == 0, res.output
        assert MODALITIES[0] in res.output and MODALITIES[1] in res.output, 'the per-modality table is printed'
        rows[fused] = _read_rows(run)
        with open(run / 'reconstruction.json') as f:
            summary = json.load(f)['modalities']
        assert all(summary[m]['count'] == len(keys) for m in MODALITIES)

    assert [(r['patient'], r['slice'], r['modality']) for r in rows[True]] == \
        [(p, s, m) for p, s in keys for m in MODALITIES], 'dataset order'
    assert len(rendered) == 2 and [len(r) for r in rendered] == [2, 1]
    images = torch.cat(rendered).cpu().numpy()
    assert images.min() >= 0 and images.max() <= 255 and images.std() > 1
    from training.dataset_mi_multimodal import safe_load_pickle
    import io
    import zipfile
    with zipfile.ZipFile(data) as z:
        targets = np.stack([np.stack([safe_load_pickle(io.BytesIO(z.read(f'train/{n}')))[m] for m in MODALITIES])
                            for n in names[::2]]).astype(np.float32)
    want, want_map = so.ssim_mse(images, targets)
    for i, (k, f) in enumerate(zip(rows[True], rows[False])):
        b, ch = divmod(i, 2)
        for got in (k, f):
            assert abs(float(got['ssim']) - want[b, ch, 0]) <= so.SSIM_TOL
            assert abs(float(got['mse']) - want[b, ch, 1]) <= so.MSE_REL * want[b, ch, 1]
        assert abs(float(k['ssim']) - float(f['ssim'])) <= so.SSIM_TOL
        assert abs(float(k['mse']) - float(f['mse'])) <= so.MSE_REL * float(f['mse'])
        assert float(k['psnr']) == pytest.approx(10 * np.log10(255.0 ** 2 / want[b, ch, 1]), rel=1e-12)
    import PIL.Image
    p, s = keys[1]
    png = np.array(PIL.Image.open(tmp_path / 'fused' / p / MODALITIES[1] / 'ssim_map' / f'map_{s}.png'))
    assert png.shape == (6, 6) and png.dtype == np.uint8
    grey = np.round(np.clip(want_map[1, 1], 0, 1) * 255).astype(np.int64)
    assert np.abs(png.astype(np.int64) - grey).max() <= 1, 'the map as 8-bit grey (a rounding tie may fall either way)'


def test_score_projections_lpips_column(tmp_path, monkeypatch):
    """--lpips with a registered stand-in detector: the column is the squared feature distance of the rendered slice
    to its target per modality, against the float64 composition on the same images.  Bound: an f32 sum of F
    non-negative terms on a fixed tree plus the f32 features' own rounding -- the project's f32 floor, 1e-4."""
    import projector_oracle as po
    from genlib.projector import projector as pj
    from genlib.projector import score
    from metrics import metric_utils
    det = po.stand_in().to(DEV)
    monkeypatch.setattr(metric_utils, '_detectors', {pj.LPIPS_URL: det})
    data, names, keys, make_run = _fabricate(tmp_path)
    rendered, targets = [], []
    real_render, real_ssim = score.render, score.ssim_op.ssim_mse

    def render(G_, ws_):
        rendered.append(real_render(G_, ws_))
        return rendered[-1]

    def ssim_mse(x, y, **kw):
        targets.append(y)
        return real_ssim(x, y, **kw)

    monkeypatch.setattr(score, 'render', render)
    monkeypatch.setattr(score.ssim_op, 'ssim_mse', ssim_mse)
    rows, summary = score.score_run(str(make_run('lpips')), batch=16, lpips=True)
    assert len(rows) == 6 and len(rendered) == 1 and list(_read_rows(tmp_path / 'lpips')[0])[-1] == 'lpips'
    with torch.no_grad():
        s_mod, t_mod = pj.split_modalities(rendered[0], MODALITIES), pj.split_modalities(targets[0], MODALITIES)
        want = {m: (det(s_mod[m].clone(), resize_images=False, return_lpips=True).double() -
                    det(t_mod[m].clone(), resize_images=False, return_lpips=True).double()).square().sum(1).cpu().numpy()
                for m in MODALITIES}
    for i, row in enumerate(rows):
        b, ch = divmod(i, 2)
        w = want[MODALITIES[ch]][b]
        print(f'{row["patient"]} {row["slice"]} {row["modality"]}: lpips {row["lpips"]:.6g}, float64 {w:.6g}')
        assert w > 0 and abs(row['lpips'] - w) <= po.FLOOR * w
    assert summary[MODALITIES[0]]['lpips']['mean'] == pytest.approx(want[MODALITIES[0]].mean(), rel=po.FLOOR)
