"""The latent projector on the GPU against the reference-made fixture (tests/golden/projector_ref.npz) and the CPU
oracle (tests/projector_oracle.py, pinned to the fixture by test_projector_host.py).

  * frozen-weight synthesis gradients -- N = 1, noise_mode='const', weights frozen, d/dws and every d/dnoise_const
    wanted (the projector's configuration of the fused conv kernels; sg2_layer_bwd's dnoise output): against the
    oracle generator on CPU, f32 to the project's f32 parity floor 1e-4 relative L2, one num_fp16_res > 0 case to
    the fp16 parity bound of parity_train.py (3e-2);
  * StyleGAN2Projector.forward end to end on the fixture's generator, target, stand-in detector and replayed draws,
    cold and warm: step-0 gradients to 1e-4; per-step loss terms and w_out[K-1] within max(1e-4, 4 x the reference's
    own f32 spread) (config_parity.judge_f32's margin on the fixture's re-evaluations); w_avg, w_std and the
    schedules tightly; best_step only if the reference's re-evaluations agree on it; then the same run with
    SG2_PROJ_FUSED=0 (the reference's composition) under the same bounds;
  * the CLI on a synthetic zip and a snapshot written by this build's saver.
"""
import glob
import json
import os
import pickle

import numpy as np
import pytest
import torch

import projector_oracle as po
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FIXTURE = os.path.join(GOLDEN, 'projector_ref.npz')
FP16_TOL = 3e-2         # parity_train.py: mixed precision against the f32 reference


@pytest.fixture(scope='module')
def fix():
    return po.load_fixture(FIXTURE)


@pytest.fixture(scope='module')
def oracle_grads(fix):
    """d/dws and d/dnoise_const of a fixed random projection of the image, oracle generator, CPU f32: computed once."""
    from oracle import sg2_oracle as O
    G = po.build_generator(O, fix['G'])
    ws, proj = _grad_inputs(G)
    return _grads(G, ws, proj), ws, proj


def _grad_inputs(G):
    g = torch.Generator().manual_seed(11)
    ws = torch.randn([1, G.mapping.num_ws, G.w_dim], generator=g)
    proj = torch.randn([1, G.img_channels, G.img_resolution, G.img_resolution], generator=g)
    return ws, proj


def _grads(G, ws, proj):
    G = G.requires_grad_(False)
    names = po.noise_names(G)
    bufs = [G.synthesis.get_buffer(n) for n in names]
    for b in bufs:
        b.requires_grad = True
    ws = ws.clone().requires_grad_(True)
    img = G.synthesis(ws, noise_mode='const')
    (img.float() * proj).sum().backward()
    assert all(p.grad is None for p in G.parameters()), 'frozen weights take no gradient'
    out = {'ws': ws.grad.detach().cpu().double().numpy()}
    out.update({n: b.grad.detach().cpu().double().numpy() for n, b in zip(names, bufs)})
    return out


@pytest.mark.parametrize('num_fp16_res', [0, 2], ids=['f32', 'fp16'])
def test_frozen_weight_synthesis_gradients(fix, oracle_grads, num_fp16_res):
    from training import networks_stylegan2 as net
    want, ws, proj = oracle_grads
    G = po.build_generator(net, fix['G'], num_fp16_res=num_fp16_res).to(DEV)
    got = _grads(G, ws.to(DEV), proj.to(DEV))
    tol = FP16_TOL if num_fp16_res else po.FLOOR
    errs = {k: po.rel(got[k], want[k]) for k in want}
    for k, e in errs.items():
        print(f'frozen-weight gradient {k} (num_fp16_res={num_fp16_res}): rel L2 {e:.3g} (bound {tol:.3g})')
    assert all(np.isfinite(v).all() for v in got.values())
    assert max(errs.values()) <= tol, {k: e for k, e in errs.items() if e > tol}


def _product_run(fix, run, tmp_path, fused, monkeypatch):
    from genlib.projector import projector as pj
    from metrics import metric_utils
    from training import networks_stylegan2 as net
    monkeypatch.setenv('SG2_PROJ_FUSED', '1' if fused else '0')
    monkeypatch.setattr(metric_utils, '_detectors', {pj.LPIPS_URL: po.stand_in(fix['det'])})
    ref = fix[run]
    G = po.build_generator(net, fix['G'])
    before = {n: b.clone() for n, b in G.synthesis.named_buffers() if 'noise_const' in n}
    p = pj.StyleGAN2Projector(outdir=str(tmp_path), device=torch.device(DEV), modalities=po.MODALITIES, dtype='float32',
                              outdir_model=None, w_avg_samples=po.W_AVG_SAMPLES, G=G)
    w_init = torch.from_numpy(ref['w_init']) if run == 'warm' else None
    with ref['tape'].replay():
        w_steps, best_step = p.forward('p000', 7, torch.from_numpy(fix['target']), num_steps=po.K_STEPS,
                                       early_stopping=100000, w_init=w_init, verbose_logger=False)
    assert ref['tape'].pos == len(ref['tape'].entries), 'the projection consumed a different number of random draws'
    last = p.last
    assert last['fused'] == fused
    assert w_steps.shape == (po.K_STEPS, G.mapping.num_ws, G.w_dim) and torch.equal(w_steps[:, 0], w_steps[:, -1])
    got = {k: np.asarray(v, np.float64) for k, v in last['history'].items()}
    got['w_out'] = w_steps[:, 0].cpu().double().numpy()
    got['grad0/w'] = last['first_grads']['w'].cpu().double().numpy()
    for i, g in enumerate(last['first_grads']['noise']):
        got[f'grad0/noise/{i}'] = g.cpu().double().numpy()
    got['best_step'] = best_step
    # the generator handed in is untouched; the private copy holds the optimised, renormalised noise
    for n, b in p.G.synthesis.named_buffers():
        if 'noise_const' in n:
            assert torch.equal(b.cpu(), before[n]) and not b.requires_grad
    for i, n in enumerate(po.noise_names(last['G'])):
        b = last['G'].synthesis.get_buffer(n).cpu().double()
        assert not torch.equal(b.float(), before[n]) and abs(float(b.square().mean()) - 1) < 1e-5 and abs(float(b.mean())) < 1e-5
        print(f'{run} fused={fused} final noise {i}: rel L2 {po.rel(b.numpy(), ref[f"noise/{i}"]):.3g} (not asserted)')
    # outputs
    assert os.path.isfile(tmp_path / 'p000' / 'projections' / f'w_00007-best_step_{best_step}.npz')
    w = np.load(tmp_path / 'p000' / 'projections' / f'w_00007-best_step_{best_step}.npz')['w']
    assert w.shape == (1, G.mapping.num_ws, G.w_dim) and np.array_equal(w[0], w_steps[best_step].cpu().numpy())
    for m in po.MODALITIES:
        import PIL.Image
        img = PIL.Image.open(tmp_path / 'p000' / m / 'image_log' / f'img_00007-best_step_{best_step}.png')
        assert img.size == (64, 32) and img.mode == 'L'
    return got, last


@pytest.mark.parametrize('run', po.RUNS)
def test_projector_end_to_end(fix, run, tmp_path, monkeypatch):
    ref = fix[run]
    agree = len({int(s['best_step']) for s in ref['spread'].values()} | {int(ref['best_step'])}) == 1
    results = {}
    for fused in (True, False):
        out = tmp_path / ('fused' if fused else 'composition')
        out.mkdir()
        got, last = _product_run(fix, run, out, fused, monkeypatch)
        what = f'{run} {"fused" if fused else "composition"}'
        e_avg, e_std = po.rel(last['w_avg'], ref['w_avg']), abs(float(last['w_std']) - float(ref['w_std'])) / float(ref['w_std'])
        print(f'{what} w_avg rel L2 {e_avg:.3g}, w_std rel {e_std:.3g}')
        assert e_avg <= 1e-5 and e_std <= 1e-5
        # the schedules: exact given the reference's w_std (test_projector_host), here through this run's own w_std
        lr, scale = np.array(last['schedules'], np.float64).T
        assert lr.tolist() == ref['lr'].tolist()
        assert np.allclose(scale, ref['w_noise_scale'], rtol=1e-5, atol=0)
        results[fused] = po.judge(got, ref, what, grads_tight=True, check=False)
        results[fused]['best_step'] = got['best_step']
    bad = [f'{"fused" if f else "composition"} {k}: {e:.3g} > {b:.3g}' for f, r in results.items()
           for k, v in r.items() if k != 'best_step' for e, b in [v] if not e <= b]
    assert not bad, bad
    if agree:
        assert results[True]['best_step'] == results[False]['best_step'] == int(ref['best_step'])


def test_cli_smoke(fix, tmp_path, monkeypatch):
    """run_projector_mi_multimodal on a synthetic zip: 2 patients x 2 slices at 16^2, every slice projected."""
    import synth_zip
    import legacy
    from click.testing import CliRunner
    from genlib import run_projector_mi_multimodal as cli
    from genlib.projector import projector as pj
    from metrics import metric_utils
    from training import networks_stylegan2 as net
    monkeypatch.setattr(metric_utils, '_detectors', {pj.LPIPS_URL: po.stand_in(fix['det'])})
    data = str(tmp_path / 'data.zip')
    synth_zip.make_zip(data, modalities=tuple(po.MODALITIES), res=16, patients=2, slices=2)
    kw = dict(c_dim=0, img_resolution=16, img_channels=2, channel_base=64, channel_max=8)
    torch.manual_seed(3)
    G = net.Generator(z_dim=16, w_dim=16, num_fp16_res=0, mapping_kwargs=dict(num_layers=2), **kw)
    D = net.Discriminator(num_fp16_res=0, **kw)
    with torch.no_grad():
        for n, p in G.named_parameters():
            if n.endswith('noise_strength'):
                p.fill_(0.1)
    mods = ','.join(po.MODALITIES)
    run = tmp_path / 'reports' / 'Pelvis_2.1' / 'training-runs' / 'data' / mods / '00002-some-training-run'
    run.mkdir(parents=True)
    legacy.save_network_pkl(str(run / 'network-snapshot-000004.pkl'), G, D, G, None, dict(path=data, modalities=po.MODALITIES))
    res = CliRunner().invoke(cli.main, [
        '--data', data, '--outdir', str(tmp_path / 'reports'), '--gpus', '1', '--experiment', '00002',
        '--network_pkl', 'network-snapshot-000004.pkl', '--step_patient_slice', '1', '--num-steps', '3',
        '--first_num_steps', '4', '--early_stopping', '2', '--modalities', mods], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    runs = glob.glob(str(tmp_path / 'reports' / 'Pelvis_2.1' / 'projection-runs' / 'data' / mods / '00000-*'))
    assert len(runs) == 1 and runs[0].endswith('-w_lips_1.0-w_pix_0.0001')
    with open(os.path.join(runs[0], 'training_options.json')) as f:
        opts = json.load(f)
    assert set(opts) == {'projector_kwargs', 'training_set_kwargs', 'num_gpus', 'batch_size', 'image_snapshot_ticks',
                         'network_snapshot_ticks', 'random_seed', 'run_dir'}
    assert opts['projector_kwargs']['num_steps'] == 3 and opts['projector_kwargs']['first_num_steps'] == 4
    assert opts['training_set_kwargs']['modalities'] == po.MODALITIES
    with open(os.path.join(runs[0], 'projected_w'), 'rb') as f:
        saved = pickle.load(f)
    assert {p: sorted(v) for p, v in saved.items()} == {'p000': ['00000', '00001'], 'p001': ['00000', '00001']}
    assert all(w.shape == (G.mapping.num_ws, 16) and w.dtype == np.float32 and np.isfinite(w).all()
               for v in saved.values() for w in v.values())
    for p in ('p000', 'p001'):
        assert len(glob.glob(os.path.join(runs[0], p, 'projections', 'w_0000[01]-best_step_*.npz'))) == 2
        for m in po.MODALITIES:
            assert len(glob.glob(os.path.join(runs[0], p, m, 'image_log', 'img_0000[01]-best_step_*.png'))) == 2
    assert os.path.isfile(os.path.join(runs[0], 'log.txt'))
