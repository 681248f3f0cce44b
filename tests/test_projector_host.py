"""The latent projector's host side (no GPU): CLI config, detector lookup, schedules, modality split, early stopping,
the projection loop's control flow on a stub projector, the CPU oracle pinned to the reference-made fixture
(tests/golden/projector_ref.npz, make_projector_golden.py) and the argument checks of the new C entry points.

Oracle pin: projector_oracle.project() on the CPU oracle generator with the fixture's tape replayed; loss terms,
step-0 gradients and w_out[K-1] within max(1e-4, 4 x the reference's own f32 spread) of the reference run (the spread:
the reference re-evaluated with one thread and at states nudged by 2^-24; the margin is config_parity.judge_f32's)."""
import ctypes
import os
import pickle

import click
import numpy as np
import pytest
import torch

import projector_oracle as po
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'projector_ref.npz')


@pytest.fixture(scope='module')
def fix():
    return po.load_fixture(FIXTURE)


@pytest.fixture()
def zip_path(tmp_path):
    import synth_zip
    path = str(tmp_path / 'data.zip')
    synth_zip.make_zip(path, modalities=tuple(po.MODALITIES), res=16, patients=2, slices=3)
    return path


# ---- CLI ----

def _flags(zip_path, tmp_path, **over):
    kw = dict(data=zip_path, outdir=str(tmp_path / 'reports'), gpus=1, experiment='00003',
              network_pkl='network-snapshot-000100.pkl')
    kw.update(over)
    return kw


def test_cli_config_and_description(zip_path, tmp_path):
    from genlib import run_projector_mi_multimodal as cli
    c, desc, outdir, outdir_model = cli.build_config(**_flags(zip_path, tmp_path, desc='x', num_steps=7))
    assert c.batch_size == 1 and c.num_gpus == 1 and c.random_seed == 303 == c.training_set_kwargs.random_seed
    assert c.image_snapshot_ticks == c.network_snapshot_ticks == 50
    assert c.training_set_kwargs.modalities == po.MODALITIES and c.training_set_kwargs.resolution == 16
    assert c.training_set_kwargs.max_size == 6 and c.training_set_kwargs.split == 'train'
    pk = c.projector_kwargs
    assert (pk.num_steps, pk.early_stopping, pk.step_patient_slice, pk.w_lpips, pk.w_pix) == (7, 50, 2, 1.0, 1e-4)
    assert (pk.save_final_projection, pk.snap_video, pk.snap_optimization_history, pk.verbose) == (True, 60, 60, False)
    assert pk.target_fname is None and 'first_num_steps' not in pk
    mods = ','.join(po.MODALITIES)
    assert outdir == os.path.join(str(tmp_path / 'reports'), 'Pelvis_2.1', 'projection-runs', 'data', mods)
    assert outdir_model == os.path.join(str(tmp_path / 'reports'), 'Pelvis_2.1', 'training-runs', 'data', mods)
    assert desc == ('data-split_train-stylegan_exp_00003-network_filename_network-snapshot-000100.pkl'
                    '-w_lips_1.0-w_pix_0.0001-x')


def test_cli_required_flags(zip_path, tmp_path):
    from genlib import run_projector_mi_multimodal as cli
    for missing in cli.REQUIRED:
        kw = _flags(zip_path, tmp_path)
        kw[missing] = None
        with pytest.raises(click.ClickException, match=f'--{missing}'):
            cli.build_config(**kw)
    with pytest.raises(click.ClickException, match='--data'):
        cli.build_config(**_flags(str(tmp_path / 'absent.zip'), tmp_path))
    from click.testing import CliRunner
    res = CliRunner().invoke(cli.main, ['--data', zip_path, '--outdir', str(tmp_path), '--gpus', '1'])
    assert res.exit_code != 0 and 'experiment' in res.output


def test_cli_run_dir_numbering(tmp_path):
    from genlib import run_projector_mi_multimodal as cli
    out = str(tmp_path / 'runs')
    assert cli.next_run_dir(out, 'd') == os.path.join(out, '00000-d')
    os.makedirs(os.path.join(out, '00000-a'))
    os.makedirs(os.path.join(out, '00007-b'))
    os.makedirs(os.path.join(out, 'notes'))
    open(os.path.join(out, '00099-file'), 'w').close()      # files do not count
    assert cli.next_run_dir(out, 'd') == os.path.join(out, '00008-d')


def test_model_path(tmp_path):
    from genlib.metric import metric_utils as gm
    import dnnlib
    root = tmp_path / 'training-runs'
    (root / '00003-run').mkdir(parents=True)
    (root / '00004-run').mkdir()
    pk = dnnlib.EasyDict()
    path = gm.get_outdir_model_path(str(tmp_path), str(root), '00003', metric_name='snap.pkl', projector_kwargs=pk)
    assert path == str(root / '00003-run' / 'snap.pkl') == pk.outdir_model and pk.network_pkl == 'snap.pkl'
    with pytest.raises(RuntimeError, match='exactly one'):
        gm.get_outdir_model_path(str(tmp_path), str(root), '0000', metric_name='snap.pkl')
    real = tmp_path / 'abs.pkl'
    real.write_bytes(b'')
    assert gm.get_outdir_model_path(str(tmp_path), str(root), 'zzz', metric_name=str(real)) == str(real)


# ---- detector lookup ----

class _NoLpips(torch.nn.Module):
    def forward(self, img, return_features: bool = False):
        return img.mean(dim=[2, 3])


@pytest.fixture()
def detectors(tmp_path, monkeypatch):
    from metrics import metric_utils
    monkeypatch.setattr(metric_utils, '_detectors', {})
    for v in ('SG2_LPIPS_DETECTOR', 'SG2_PR_DETECTOR', 'SG2_FID_DETECTOR'):
        monkeypatch.delenv(v, raising=False)
    paths = {'lpips': str(tmp_path / 'lpips.pt'), 'plain': str(tmp_path / 'plain.pt')}
    torch.jit.script(po.stand_in()).save(paths['lpips'])
    torch.jit.script(_NoLpips()).save(paths['plain'])
    return paths


def test_detector_lookup(detectors, monkeypatch):
    from genlib.projector import projector as pj
    from metrics import metric_utils, precision_recall
    img = torch.rand(1, 3, 32, 32) * 255
    with pytest.raises(RuntimeError, match='SG2_LPIPS_DETECTOR or SG2_PR_DETECTOR'):
        metric_utils.get_feature_detector(pj.LPIPS_URL)
    monkeypatch.setenv('SG2_PR_DETECTOR', detectors['lpips'])           # the fallback
    det = metric_utils.get_feature_detector(pj.LPIPS_URL)
    want = po.stand_in()(img, return_lpips=True)
    assert torch.equal(pj.lpips_features(det, img.clone()), want)
    monkeypatch.setattr(metric_utils, '_detectors', {})
    monkeypatch.setenv('SG2_LPIPS_DETECTOR', detectors['plain'])        # the projector's own variable goes first
    det = metric_utils.get_feature_detector(pj.LPIPS_URL)
    with pytest.raises(RuntimeError, match='SG2_LPIPS_DETECTOR'):
        pj.lpips_features(det, img.clone())
    # what pr50k3 and FID get is unchanged: their own variables only
    assert metric_utils.detector_env_vars(precision_recall.DETECTOR_URL) == ('SG2_PR_DETECTOR',)
    assert metric_utils.detector_env_vars('https://x/metrics/inception-2015-12-05.pkl') == ('SG2_FID_DETECTOR',)
    pr = metric_utils.get_feature_detector(precision_recall.DETECTOR_URL)
    assert torch.equal(pr(img, return_lpips=True), want), 'pr50k3 still reads SG2_PR_DETECTOR'


# ---- schedules, split, early stopping ----

def test_schedules_equal_the_fixture(fix):
    from genlib.projector import projector as pj
    for run in po.RUNS:
        ref = fix[run]
        # (w_std keeps the type the reference computes it in -- numpy float32 cold, Python float warm -- and the
        # perturbation scale inherits it through numpy's promotion rules, in the reference and here alike)
        w_std = ref['w_std'][()] if ref['w_std'].dtype == np.float32 else float(ref['w_std'])
        got = [pj.schedule(s, po.K_STEPS, w_std) for s in range(po.K_STEPS)]
        assert [g[0] for g in got] == ref['lr'].tolist()
        assert [g[1] for g in got] == ref['w_noise_scale'].tolist()
    assert pj.schedule(0, 500, 1.0)[0] == 0.0 and pj.schedule(25, 500, 1.0)[0] == pytest.approx(0.1)
    assert pj.schedule(375, 500, 2.0)[1] == 0.0


def test_modality_split():
    from genlib.projector import projector as pj
    one = torch.arange(4.).view(1, 1, 2, 2)
    out = pj.split_modalities(one, ['CT'])
    assert list(out) == ['CT'] and out['CT'].shape == (1, 3, 2, 2) and torch.equal(out['CT'][:, 2], one[:, 0])
    rgb = torch.arange(12.).view(1, 3, 2, 2)
    out = pj.split_modalities(rgb, ['CT', 'unused'])
    assert list(out) == ['CT'] and out['CT'] is rgb
    two = torch.arange(8.).view(1, 2, 2, 2)
    out = pj.split_modalities(two, ['a', 'b'])
    assert list(out) == ['a', 'b']
    for i, m in enumerate(out):
        assert out[m].shape == (1, 3, 2, 2) and all(torch.equal(out[m][:, c], two[:, i]) for c in range(3))
    four = torch.arange(16.).view(1, 4, 2, 2)
    assert list(pj.split_modalities(four, ['a', 'b', 'c', 'd'])) == ['a', 'b', 'c', 'd']


def test_early_stopping_and_best_step():
    from genlib.projector import projector as pj
    losses = [5.0, 4.0, 4.5, 4.0, 4.2, 3.0, 9.0]
    seen = []

    def step(i):
        seen.append(i)
        return losses[i]

    assert pj.optimise(7, 100, step) == (5, 3.0) and seen == list(range(7))
    seen.clear()
    assert pj.optimise(7, 3, step) == (1, 4.0) and seen == [0, 1, 2, 3, 4], 'three steps without improvement (a tie is none)'
    seen.clear()
    assert pj.optimise(7, 1, step) == (1, 4.0) and seen == [0, 1, 2]
    assert pj.optimise(3, 10, lambda i: float('nan')) == (3, np.inf), 'no loss below +inf: best_step stays num_steps'


# ---- projection loop ----

class StubProjector:
    calls = []

    def __init__(self, outdir, device, modalities, dtype, **kwargs):
        self.kwargs = dict(outdir=outdir, modalities=modalities, dtype=dtype, **kwargs)
        StubProjector.calls = []

    def forward(self, id_patient, id_slice, target, num_steps, early_stopping, w_init=None, verbose=False):
        n = len(StubProjector.calls)
        StubProjector.calls.append(dict(patient=id_patient, slice=id_slice, shape=tuple(target.shape), dtype=target.dtype,
                                        num_steps=num_steps, early_stopping=early_stopping, verbose=verbose,
                                        w_init=None if w_init is None else w_init.clone()))
        w = torch.arange(num_steps * 8, dtype=torch.float32).view(num_steps, 2, 4) + 1000 * n
        return w, num_steps - 1


def test_projection_loop_control_flow(zip_path, tmp_path, monkeypatch):
    from genlib.projector import projection_loop as pl
    from genlib import run_projector_mi_multimodal as cli
    monkeypatch.setattr(pl, '_device', lambda rank: torch.device('cpu'))
    c, _, _, _ = cli.build_config(**_flags(zip_path, tmp_path, num_steps=3, early_stopping=2, first_num_steps=5,
                                           first_early_stopping=77, verbose=True))
    c.projector_kwargs.class_name = 'test_projector_host.StubProjector'
    c.projector_kwargs.outdir_model = 'unused'

    def run(step):
        c.projector_kwargs.step_patient_slice = step
        run_dir = tmp_path / f'run{step}'
        run_dir.mkdir()
        pl.projection_loop(run_dir=str(run_dir), rank=0, **c)
        import sys
        calls = sys.modules['test_projector_host'].StubProjector.calls
        with open(run_dir / 'projected_w', 'rb') as f:
            return calls, pickle.load(f)

    calls, saved = run(1)
    assert [(k['patient'], k['slice']) for k in calls] == [(f'p{p:03d}', s) for p in range(2) for s in range(3)]
    assert all(k['shape'] == (1, 2, 16, 16) and k['dtype'] == torch.float32 for k in calls)
    for p in range(2):
        first, later = calls[3 * p], calls[3 * p + 1:3 * p + 3]
        assert (first['num_steps'], first['early_stopping'], first['w_init'], first['verbose']) == (5, 77, None, False)
        best_first = torch.arange(40.).view(5, 2, 4)[4] + 1000 * (3 * p)
        for k in later:     # every later slice starts from the FIRST slice's best w, not from its predecessor's
            assert (k['num_steps'], k['early_stopping'], k['verbose']) == (3, 2, True)
            assert torch.equal(k['w_init'], best_first)
    assert type(saved) is dict and list(saved) == ['p000', 'p001']
    assert all(type(v) is dict and list(v) == ['00000', '00001', '00002'] for v in saved.values())
    assert saved['p001']['00001'].shape == (2, 4) and saved['p001']['00001'].dtype == np.float32
    assert np.array_equal(saved['p001']['00001'], (torch.arange(24.).view(3, 2, 4)[2] + 4000).numpy())

    calls, saved = run(2)   # items 0, 2, 4 of the whole dataset: p000/0, p000/2, p001/1 (the counter is not per patient)
    assert [(k['patient'], k['slice']) for k in calls] == [('p000', 0), ('p000', 2), ('p001', 1)]
    assert [k['w_init'] is None for k in calls] == [True, False, True]
    assert {p: list(v) for p, v in saved.items()} == {'p000': ['00000', '00002'], 'p001': ['00001']}


# ---- the oracle pinned to the reference's fixture ----

@pytest.mark.parametrize('run', po.RUNS)
def test_oracle_reproduces_the_reference(fix, run):
    from oracle import sg2_oracle as O
    ref = fix[run]
    G = po.build_generator(O, fix['G'])
    det = po.stand_in(fix['det'])
    w_init = torch.from_numpy(ref['w_init']) if run == 'warm' else None
    with ref['tape'].replay():
        got = po.project(G, det, torch.from_numpy(fix['target']), po.K_STEPS, w_init=w_init)
    assert ref['tape'].pos == len(ref['tape'].entries)
    assert got['lr'].tolist() == ref['lr'].tolist() and got['w_noise_scale'].tolist() == ref['w_noise_scale'].tolist()
    assert po.rel(got['w_avg'], ref['w_avg']) <= 1e-6 and abs(got['w_std'] - ref['w_std']) <= 1e-6 * ref['w_std']
    po.judge(got, ref, f'oracle {run}')
    if len({int(s['best_step']) for s in ref['spread'].values()} | {int(ref['best_step'])}) == 1:
        assert int(got['best_step']) == int(ref['best_step'])


# ---- the new C entry points: argument checks only, no device work ----

def test_noise_reg_symbols_and_argument_errors():
    import sg2hip
    L = sg2hip.lib()
    assert L.sg2_abi_version() == 11
    for name in ('sg2_noise_reg_scratch_bytes', 'sg2_noise_reg_fwd', 'sg2_noise_reg_bwd', 'sg2_noise_normalize_multi'):
        assert hasattr(L, name) and name in sg2hip.SIGNATURES
    nbytes = ctypes.c_int64(-1)
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below fails its argument checks first
    ok = sg2hip.i64arr([32, 4, 48, 8, 112, 16, 368, 256])
    assert L.sg2_noise_reg_scratch_bytes(ctypes.byref(nbytes), ok, 4) == 0
    # pooled levels: 16 -> 8x8; 256 -> 128^2 + ... + 8^2; partials: 2 floats per 1024-element chunk of every level
    pooled = 64 + sum((256 >> l) ** 2 for l in range(1, 6))
    chunks = 1 + 1 + 2 + sum(max(1, (256 >> l) ** 2 // 1024) for l in range(6))
    assert nbytes.value == 4 * (pooled + 2 * chunks)
    bad = [([0, 6], 1, b'power of two'), ([0, 2], 1, b'power of two'), ([0, 2048], 1, b'power of two'),
           ([0, 4], 0, b'nbuf'), ([2, 4], 1, b'multiples of 4'), ([0, 4] * 33, 33, b'nbuf')]
    for table, n, msg in bad:
        t = sg2hip.i64arr(table)
        for rc in (L.sg2_noise_reg_scratch_bytes(ctypes.byref(nbytes), t, n),
                   L.sg2_noise_reg_fwd(p, p, p, t, n, p, None),
                   L.sg2_noise_reg_bwd(p, p, p, p, t, n, p, 0, None),
                   L.sg2_noise_normalize_multi(p, t, n, None)):
            assert rc != 0 and msg in L.sg2_last_error(), (table, n, L.sg2_last_error())
    assert L.sg2_noise_reg_fwd(p, p, p, ok, 4, None, None) != 0 and b'scratch' in L.sg2_last_error()
    assert L.sg2_noise_reg_bwd(p, p, p, p, ok, 4, None, 0, None) != 0 and b'scratch' in L.sg2_last_error()
    assert L.sg2_noise_reg_scratch_bytes(ctypes.byref(nbytes), None, 1) != 0 and b'table' in L.sg2_last_error()
    assert L.sg2_noise_normalize_multi(None, ok, 4, None) != 0 and b'non-null' in L.sg2_last_error()


def test_noise_reg_python_side_needs_no_gpu_for_its_layout():
    from torch_utils.ops import noise_reg
    table, total = noise_reg.make_table(30, [4, 8, 16])
    assert table == ((32, 4), (48, 8), (112, 16)) and total == 368
    assert noise_reg.supported(table) and not noise_reg.supported(((32, 12),)) and not noise_reg.supported(())
    assert [noise_reg.num_levels(r) for r in (4, 8, 16, 256, 1024)] == [1, 1, 2, 6, 8]
    with pytest.raises(RuntimeError):
        noise_reg.noise_regularizer(torch.zeros(368), table)     # CPU tensors are refused
    bufs = [torch.randn(r, r, dtype=torch.float64) for r in (4, 16)]
    want = sum((lv * lv.roll(1, d)).mean() ** 2 for b in bufs
               for lv in ([b] if b.shape[0] <= 8 else [b, b.view(8, 2, 8, 2).mean(dim=(1, 3))]) for d in (0, 1))
    assert float(noise_reg.noise_regularizer_ref(bufs)) == pytest.approx(float(want), rel=1e-12)


# ---- verbose logs ----

def test_verbose_logs_and_lazy_imageio(tmp_path):
    """The loss table and plots of a projection (Agg backend); a video without imageio is a clear error, and the
    package is not needed for anything else."""
    import importlib.util
    import pandas as pd
    from genlib.projector import projector as pj
    p = pj.StyleGAN2Projector(outdir=str(tmp_path), device=torch.device('cpu'), modalities=po.MODALITIES, dtype='float32',
                              outdir_model=None, snap_optimization_history=2, snap_video=False, G=torch.nn.Identity())
    cols = ['reg_loss', 'tot_loss'] + [f'{m}_{t}_loss' for m in po.MODALITIES for t in ('lpips', 'pix')]
    history = pd.DataFrame({c: np.linspace(1.0, 0.5, 4) + i for i, c in enumerate(cols)})
    target = torch.zeros(1, 2, 8, 8)
    p.logs('p000', 3, target, history, None)            # slice 3: not a multiple of 2 -> nothing written
    assert os.listdir(tmp_path / 'p000' / 'loss') == []
    p.logs('p000', 4, target, history, None)
    assert sorted(os.listdir(tmp_path / 'p000' / 'loss')) == ['lpips_loss_modalities_00004.png', 'opt_loss_00004.csv',
                                                            'pix_loss_modalities_00004.png']
    back = pd.read_csv(tmp_path / 'p000' / 'loss' / 'opt_loss_00004.csv', index_col=0)
    assert list(back.columns) == cols and np.allclose(back.values, history.values)
    if importlib.util.find_spec('imageio') is None:
        p.snap_video = 1
        with pytest.raises(RuntimeError, match='imageio'):
            p.logs('p000', 4, target, history, torch.zeros(2, 3, 4))
