"""Batched latent projection on the GPU (StyleGAN2Projector.forward_batch) against the reference-made fixture
(tests/golden/projector_ref.npz) and the CPU oracle (tests/projector_oracle.py).

  * per-sample synthesis gradients at N = 3: noise_const replaced by [3, 1, R, R] leaves; d/dws and every
    d/dnoise_const of sample b against the oracle generator run at batch 1 on that sample's ws and noise -- f32 to the
    f32 parity floor (po.FLOOR), num_fp16_res = 2 to the fp16 parity bound (test_projector_gpu.FP16_TOL);
  * forward_batch at B = 1 under the fixture's own tape, cold and warm, fused and SG2_PROJ_FUSED=0: the tape is
    consumed exactly and every judged quantity passes po.judge (grads_tight) against the reference-made run;
  * forward_batch at B = 3, cold and warm: sample 0 is the fixture's target with the fixture's draws (the batched
    tape holds the sample-major initial draws, then the per-step [3, 1, w_dim] arrays whose row 0 is the fixture's),
    judged against the fixture's reference run -- batch mates do not perturb a sample; samples 1 and 2 are
    po.make_target of two other seeds with fresh numpy draws, judged against po.project on the CPU oracle under their
    own tapes with the fixture run's bound table, max(FLOOR, 4 x the reference's own spread): it applies because the
    generator, the step count and the quantities are the same;
  * the CLI with --batch 2 against --batch 1 on a synthetic zip.
"""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

import projector_oracle as po
from conftest import GOLDEN
from rngtape import Tape

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FIXTURE = os.path.join(GOLDEN, 'projector_ref.npz')
FP16_TOL = 3e-2         # parity_train.py: mixed precision against the f32 reference (test_projector_gpu.FP16_TOL)
SEEDS = (5, 9)          # the targets of samples 1 and 2
IDS = [('p000', 7), ('p001', 3), ('p001', 4)]


@pytest.fixture(scope='module')
def fix():
    return po.load_fixture(FIXTURE)


# ---- per-sample synthesis gradients ----

def _batch_inputs(G, n=3):
    g = torch.Generator().manual_seed(23)
    ws = torch.randn([n, G.mapping.num_ws, G.w_dim], generator=g)
    proj = torch.randn([n, G.img_channels, G.img_resolution, G.img_resolution], generator=g)
    noise = [torch.randn([n, 1, *G.synthesis.get_buffer(name).shape], generator=g) for name in po.noise_names(G)]
    return ws, proj, noise


def _owners(G):
    return [(G.synthesis.get_submodule(name.rsplit('.', 1)[0]), name) for name in po.noise_names(G)]


def _grads(G, ws, proj, noise, squeeze):
    """d/dws and d/dnoise of sum(img * proj) with the noise buffers replaced by leaves (squeeze: [R, R] at batch 1)."""
    G = G.requires_grad_(False)
    leaves = []
    for (owner, _), n in zip(_owners(G), noise):
        leaf = (n[0, 0] if squeeze else n).clone().requires_grad_(True)
        owner._buffers['noise_const'] = leaf
        leaves.append(leaf)
    ws = ws.clone().requires_grad_(True)
    img = G.synthesis(ws, noise_mode='const')
    (img.float() * proj).sum().backward()
    assert all(p.grad is None for p in G.parameters()), 'frozen weights take no gradient'
    return ws.grad.detach().cpu().double().numpy(), [l.grad.detach().cpu().double().numpy() for l in leaves]


@pytest.fixture(scope='module')
def oracle_batch_grads(fix):
    """Per sample, the oracle generator at batch 1 on that sample's ws and noise (CPU f32): computed once."""
    import copy
    from oracle import sg2_oracle as O
    G = po.build_generator(O, fix['G'])
    ws, proj, noise = _batch_inputs(G)
    want = [_grads(copy.deepcopy(G), ws[b:b + 1], proj[b:b + 1], [n[b:b + 1] for n in noise], squeeze=True)
            for b in range(ws.shape[0])]
    return want, ws, proj, noise


@pytest.mark.parametrize('num_fp16_res', [0, 2], ids=['f32', 'fp16'])
def test_per_sample_synthesis_gradients(fix, oracle_batch_grads, num_fp16_res):
    from training import networks_stylegan2 as net
    want, ws, proj, noise = oracle_batch_grads
    G = po.build_generator(net, fix['G'], num_fp16_res=num_fp16_res).to(DEV)
    gws, gnoise = _grads(G, ws.to(DEV), proj.to(DEV), [n.to(DEV) for n in noise], squeeze=False)
    tol = FP16_TOL if num_fp16_res else po.FLOOR
    bad = []
    for b, (wws, wnoise) in enumerate(want):
        errs = {'ws': po.rel(gws[b], wws[0])}
        errs.update({f'noise/{i}': po.rel(g[b, 0], w) for i, (g, w) in enumerate(zip(gnoise, wnoise))})
        for k, e in errs.items():
            print(f'sample {b} gradient {k} (num_fp16_res={num_fp16_res}): rel L2 {e:.3g} (bound {tol:.3g})')
            if not e <= tol:
                bad.append((b, k, e))
    assert np.isfinite(gws).all() and all(np.isfinite(g).all() for g in gnoise)
    assert not bad, bad


# ---- forward_batch ----

def _projector(fix, tmp_path, fused, monkeypatch):
    from genlib.projector import projector as pj
    from metrics import metric_utils
    from training import networks_stylegan2 as net
    monkeypatch.setenv('SG2_PROJ_FUSED', '1' if fused else '0')
    monkeypatch.setattr(metric_utils, '_detectors', {pj.LPIPS_URL: po.stand_in(fix['det'])})
    G = po.build_generator(net, fix['G'])
    before = {n: b.clone() for n, b in G.synthesis.named_buffers() if 'noise_const' in n}
    p = pj.StyleGAN2Projector(outdir=str(tmp_path), device=torch.device(DEV), modalities=po.MODALITIES, dtype='float32',
                              outdir_model=None, w_avg_samples=po.W_AVG_SAMPLES, G=G)
    return p, G, before


def _sample_run(sample, w_steps_b, best_step):
    got = {k: np.asarray(v, np.float64) for k, v in sample['history'].items()}
    got['w_out'] = w_steps_b[:, 0].cpu().double().numpy()
    got['grad0/w'] = sample['first_grads']['w'].cpu().double().numpy()
    for i, g in enumerate(sample['first_grads']['noise']):
        got[f'grad0/noise/{i}'] = g.cpu().double().numpy()
    got['best_step'] = best_step
    return got


def _check_outputs(p, G, before, tmp_path, ids, w_steps, best_steps):
    import PIL.Image
    for n, b in p.G.synthesis.named_buffers():      # the generator handed in is untouched
        if 'noise_const' in n:
            assert torch.equal(b.cpu(), before[n]) and not b.requires_grad
    assert w_steps.shape == (len(ids), po.K_STEPS, G.mapping.num_ws, G.w_dim) and torch.equal(w_steps[:, :, 0], w_steps[:, :, -1])
    for b, (patient, sl) in enumerate(ids):
        sample = p.last['samples'][b]
        assert sample['best_step'] == best_steps[b] and sample['stop_step'] == po.K_STEPS - 1
        for i, nb in enumerate(sample['noise']):    # the final noise: renormalised per sample
            nb = nb.cpu().double()
            assert nb.shape == before[po.noise_names(G)[i]].shape
            assert abs(float(nb.square().mean()) - 1) < 1e-5 and abs(float(nb.mean())) < 1e-5
        path = tmp_path / patient / 'projections' / f'w_{sl:05d}-best_step_{best_steps[b]}.npz'
        assert os.path.isfile(path)
        w = np.load(path)['w']
        assert w.shape == (1, G.mapping.num_ws, G.w_dim) and np.array_equal(w[0], w_steps[b, best_steps[b]].cpu().numpy())
        for m in po.MODALITIES:
            img = PIL.Image.open(tmp_path / patient / m / 'image_log' / f'img_{sl:05d}-best_step_{best_steps[b]}.png')
            assert img.size == (64, 32) and img.mode == 'L'


def _agree(ref):
    return len({int(s['best_step']) for s in ref['spread'].values()} | {int(ref['best_step'])}) == 1


@pytest.mark.parametrize('run', po.RUNS)
def test_forward_batch_of_one_is_the_fixture_run(fix, run, tmp_path, monkeypatch):
    ref = fix[run]
    results = {}
    for fused in (True, False):
        out = tmp_path / ('fused' if fused else 'composition')
        out.mkdir()
        p, G, before = _projector(fix, out, fused, monkeypatch)
        w_init = torch.from_numpy(ref['w_init']) if run == 'warm' else None
        with ref['tape'].replay():
            w_steps, best_steps = p.forward_batch(IDS[:1], torch.from_numpy(fix['target']), num_steps=po.K_STEPS,
                                                  early_stopping=100000, w_init=w_init, verbose_logger=False)
        assert ref['tape'].pos == len(ref['tape'].entries), 'the projection consumed a different number of random draws'
        last = p.last
        assert last['fused'] == fused and last['batch'] == 1 and len(best_steps) == 1
        _check_outputs(p, G, before, out, IDS[:1], w_steps, best_steps)
        sample = last['samples'][0]
        what = f'B=1 {run} {"fused" if fused else "composition"}'
        e_avg = po.rel(sample['w_avg'], ref['w_avg'])
        e_std = abs(float(sample['w_std']) - float(ref['w_std'])) / float(ref['w_std'])
        print(f'{what} w_avg rel L2 {e_avg:.3g}, w_std rel {e_std:.3g}')
        assert e_avg <= 1e-5 and e_std <= 1e-5
        assert [s[0] for s in last['schedules']] == ref['lr'].tolist()
        assert np.allclose([s[1][0] for s in last['schedules']], ref['w_noise_scale'], rtol=1e-5, atol=0)
        results[fused] = po.judge(_sample_run(sample, w_steps[0], best_steps[0]), ref, what, grads_tight=True, check=False)
        results[fused]['best_step'] = best_steps[0]
    bad = [f'{"fused" if f else "composition"} {k}: {e:.3g} > {b:.3g}' for f, r in results.items()
           for k, v in r.items() if k != 'best_step' for e, b in [v] if not e <= b]
    assert not bad, bad
    if _agree(ref):
        assert results[True]['best_step'] == results[False]['best_step'] == int(ref['best_step'])


@pytest.fixture(scope='module')
def batch_of_three(fix):
    """Per run: the batched tape, the targets, the per-sample w_init and, for samples 1 and 2, po.project on the CPU
    oracle under their own tapes: computed once."""
    from oracle import sg2_oracle as O
    G = po.build_generator(O, fix['G'])
    det = po.stand_in(fix['det'])
    nbuf = len(po.noise_names(G))
    targets = torch.from_numpy(np.concatenate([fix['target']] + [po.make_target(s) for s in SEEDS]))
    out = {}
    for run in po.RUNS:
        ref = fix[run]
        entries = ref['tape'].entries
        init0, steps0 = entries[:nbuf], entries[nbuf:]
        assert len(steps0) == po.K_STEPS and all(k == 'randn' and a.shape == (1, 1, G.w_dim) for k, a in steps0)
        rs = np.random.RandomState(100 + len(run))
        init = [[('randn', rs.standard_normal(a.shape).astype(np.float32)) for _, a in init0] for _ in SEEDS]
        steps = [[rs.standard_normal(a.shape).astype(np.float32) for _, a in steps0] for _ in SEEDS]
        tape = Tape(entries=list(init0) + init[0] + init[1] +
                    [('randn', np.concatenate([a] + [s[i] for s in steps])) for i, (_, a) in enumerate(steps0)])
        w_init = None
        if run == 'warm':
            w0 = torch.from_numpy(ref['w_init'])
            g = torch.Generator().manual_seed(3)
            w_init = torch.stack([w0, w0 + 0.1 * torch.randn(w0.shape, generator=g), w0 * 0.9])
        want = []
        for b in range(len(SEEDS)):
            own = Tape(entries=init[b] + [('randn', a) for a in steps[b]])
            with own.replay():
                want.append(po.project(G, det, targets[b + 1:b + 2], po.K_STEPS,
                                       w_init=None if w_init is None else w_init[b + 1]))
            assert own.pos == len(own.entries)
        out[run] = dict(tape=tape, w_init=w_init, want=want)
    return targets, out


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composition'])
@pytest.mark.parametrize('run', po.RUNS)
def test_forward_batch_of_three(fix, batch_of_three, run, fused, tmp_path, monkeypatch):
    ref = fix[run]
    targets, cases = batch_of_three
    case = cases[run]
    p, G, before = _projector(fix, tmp_path, fused, monkeypatch)
    with case['tape'].replay():
        w_steps, best_steps = p.forward_batch(IDS, targets, num_steps=po.K_STEPS, early_stopping=100000,
                                              w_init=case['w_init'], verbose_logger=False)
    assert case['tape'].pos == len(case['tape'].entries), 'the projection consumed a different number of random draws'
    assert p.last['fused'] == fused and p.last['batch'] == 3
    _check_outputs(p, G, before, tmp_path, IDS, w_steps, best_steps)
    what = f'B=3 {run} {"fused" if fused else "composition"}'
    bad = []

    # sample 0: the fixture's run, unperturbed by its batch mates
    got0 = _sample_run(p.last['samples'][0], w_steps[0], best_steps[0])
    res = po.judge(got0, ref, f'{what} sample 0', grads_tight=True, check=False)
    bad += [f'sample 0 {k}: {e:.3g} > {b:.3g}' for k, (e, b) in res.items() if not e <= b]
    if _agree(ref):
        assert best_steps[0] == int(ref['best_step'])

    # samples 1 and 2: the CPU oracle under their own tapes, the fixture run's bound table
    bnd = po.bounds(ref)
    for b, want in enumerate(case['want'], start=1):
        got = po.quantities(_sample_run(p.last['samples'][b], w_steps[b], best_steps[b]))
        wq = po.quantities(want)
        assert set(got) == set(wq)
        for k in sorted(wq):
            bound = po.FLOOR if k.startswith('grad0/') else bnd[k][0]
            e = po.rel(got[k], wq[k])
            print(f'{what} sample {b} {k}: rel L2 {e:.3g} (bound {bound:.3g})')
            if not e <= bound:
                bad.append(f'sample {b} {k}: {e:.3g} > {bound:.3g}')
        if run == 'warm':
            assert abs(float(p.last['samples'][b]['w_std']) - float(want['w_std'])) <= 1e-5 * float(want['w_std'])
    assert not bad, bad


# ---- the CLI ----

def test_cli_batch_2_against_batch_1(fix, tmp_path, monkeypatch):
    """run_projector_mi_multimodal --batch 2 on a synthetic zip (2 patients x 3 slices at 16^2, every slice): exit 0,
    the npz / PNG set and the projected_w key order of a --batch 1 run, all w finite."""
    import synth_zip
    import legacy
    from click.testing import CliRunner
    from genlib import run_projector_mi_multimodal as cli
    from genlib.projector import projector as pj
    from metrics import metric_utils
    from training import networks_stylegan2 as net
    monkeypatch.setattr(metric_utils, '_detectors', {pj.LPIPS_URL: po.stand_in(fix['det'])})
    data = str(tmp_path / 'data.zip')
    synth_zip.make_zip(data, modalities=tuple(po.MODALITIES), res=16, patients=2, slices=3)
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
    found = {}
    for batch in (1, 2):
        res = CliRunner().invoke(cli.main, [
            '--data', data, '--outdir', str(tmp_path / 'reports'), '--gpus', '1', '--experiment', '00002',
            '--network_pkl', 'network-snapshot-000004.pkl', '--step_patient_slice', '1', '--num-steps', '3',
            '--first_num_steps', '4', '--early_stopping', '2', '--modalities', mods, '--batch', str(batch),
            '--desc', f'b{batch}'], catch_exceptions=False)
        assert res.exit_code == 0, res.output
        runs = glob.glob(str(tmp_path / 'reports' / 'Pelvis_2.1' / 'projection-runs' / 'data' / mods / f'*-b{batch}'))
        assert len(runs) == 1
        import json
        with open(os.path.join(runs[0], 'training_options.json')) as f:
            assert json.load(f)['projector_kwargs']['batch'] == batch
        with open(os.path.join(runs[0], 'projected_w'), 'rb') as f:
            saved = pickle.load(f)
        assert all(w.shape == (G.mapping.num_ws, 16) and w.dtype == np.float32 and np.isfinite(w).all()
                   for v in saved.values() for w in v.values())
        # file names without the best step, which the two runs need not share
        files = sorted(os.path.relpath(f, runs[0]).split('-best_step_')[0]
                       for f in glob.glob(os.path.join(runs[0], 'p*', '**', '*-best_step_*'), recursive=True))
        found[batch] = ([(p, list(v)) for p, v in saved.items()], files)
    assert found[1][0] == [('p000', ['00000', '00001', '00002']), ('p001', ['00000', '00001', '00002'])]
    assert found[2] == found[1], 'the same keys in the same order, the same npz / PNG set'
    assert len(found[2][1]) == 6 * (1 + len(po.MODALITIES))
