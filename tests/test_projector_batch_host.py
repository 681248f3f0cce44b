"""The batched latent projection's host side (no GPU): per-sample early stopping, the buffer-major flat layout and
its one-pass flat gradient, and the argument checks of the batched C entry points (no device work)."""
import ctypes

import numpy as np
import pytest
import torch


# ---- optimise_batch: per column exactly optimise ----

def _columns(table, num_steps, early_stopping):
    """optimise on every column alone: (best_step, best_loss, steps seen)."""
    from genlib.projector import projector as pj
    out = []
    for col in zip(*table):
        seen = []

        def step(i, col=col, seen=seen):
            seen.append(i)
            return col[i]

        out.append(pj.optimise(num_steps, early_stopping, step) + (seen[-1],))
    return out


TABLES = {
    # ties (a tie is no improvement), a column that never improves, columns that stop at different steps
    'mixed': ([[5.0, 1.0, 3.0, 9.0],
               [4.0, 1.0, 2.0, 9.5],
               [4.5, 1.0, 2.5, 9.0],
               [4.0, 1.0, 1.0, 8.0],
               [4.2, 2.0, 1.5, 8.5],
               [3.0, 3.0, 1.0, 8.0],
               [9.0, 0.5, 0.9, 7.0]], (100, 3, 2, 1)),
    # every column stops before num_steps: the loop is shorter than num_steps
    'all_stop': ([[1.0, 2.0], [2.0, 1.0], [3.0, 3.0], [4.0, 4.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], (2, 3)),
    'nan_and_inf': ([[float('nan'), float('inf'), 1.0]] * 4, (10, 2)),
}


@pytest.mark.parametrize('name', list(TABLES))
def test_optimise_batch_equals_optimise_per_column(name):
    from genlib.projector import projector as pj
    table, stoppings = TABLES[name]
    num_steps = len(table)
    for early_stopping in stoppings:
        seen = []

        def step(i):
            seen.append(i)
            return table[i]

        best_steps, best_losses, stop_steps = pj.optimise_batch(num_steps, early_stopping, step)
        want = _columns(table, num_steps, early_stopping)
        assert list(zip(best_steps, best_losses, stop_steps)) == want, (name, early_stopping)
        assert seen == list(range(max(w[2] for w in want) + 1)), 'the loop ends when every column has stopped'
    if name == 'all_stop':
        calls = []
        assert pj.optimise_batch(7, 2, lambda i: calls.append(i) or table[i]) == ([0, 1], [1.0, 1.0], [2, 3])
        assert calls == [0, 1, 2, 3], 'both columns stopped: steps 4..6 never run'
    if name == 'nan_and_inf':
        assert pj.optimise_batch(4, 10, lambda i: table[i])[:2] == ([4, 4, 0], [np.inf, np.inf, 1.0])


def test_optimise_batch_takes_a_tensor_of_losses():
    from genlib.projector import projector as pj
    losses = torch.tensor([[3.0, 1.0], [2.0, 1.5], [2.5, 0.5]])
    assert pj.optimise_batch(3, 5, lambda i: losses[i]) == ([1, 2], [2.0, 0.5], [2, 2])


# ---- the buffer-major layout ----

def test_make_batched_table():
    from torch_utils.ops import noise_reg
    sizes = [4, 8, 8, 16]
    for w_dim in (32, 30, 1):
        assert noise_reg.make_batched_table(1, w_dim, sizes) == noise_reg.make_table(w_dim, sizes)
    table, total = noise_reg.make_batched_table(3, 30, sizes)
    assert table == ((96, 4), (144, 8), (336, 8), (528, 16)) and total == 528 + 3 * 256
    for B in (1, 2, 3, 5, 64):
        for w_dim in (1, 30, 32, 511, 512):
            table, total = noise_reg.make_batched_table(B, w_dim, sizes)
            assert all(off % 4 == 0 for off, _ in table) and noise_reg.supported(table)
            assert table[0][0] == B * ((w_dim + 3) // 4 * 4)
            assert all(b[0] == a[0] + B * a[1] ** 2 for a, b in zip(table, table[1:]))
            assert total == table[-1][0] + B * sizes[-1] ** 2
    with pytest.raises(RuntimeError):
        noise_reg.make_batched_table(0, 32, sizes)


@pytest.mark.parametrize('w_dim', [8, 6])
def test_unflatten_batched_views_and_one_flat_gradient(w_dim):
    from torch_utils.ops import noise_reg
    B, sizes = 3, [4, 8]
    table, total = noise_reg.make_batched_table(B, w_dim, sizes)
    x = torch.arange(total + 5, dtype=torch.float32).requires_grad_(True)      # a tail behind `total`
    w, views = noise_reg.unflatten_batched(x, table, B, w_dim)
    assert w.shape == (B, 1, w_dim) and [tuple(v.shape) for v in views] == [(B, 1, 4, 4), (B, 1, 8, 8)]
    assert all(v.is_contiguous() for v in views)
    for b in range(B):
        assert torch.equal(w[b, 0].detach(), x.detach()[8 * b:8 * b + w_dim]), 'latent row b starts at b * Wp'
        for (off, r), v in zip(table, views):
            assert v[b].data_ptr() == x.data_ptr() + 4 * (off + b * r * r), 'sample b of a buffer starts at off + b R^2'
    # sample b of w weighs b + 1, views[1] weighs 3; views[0] gets no gradient
    scale = torch.arange(1.0, B + 1).view(B, 1, 1)
    ((w * scale).sum() + (views[1] * 3.0).sum()).backward()
    want = torch.zeros(total + 5)
    for b in range(B):
        want[8 * b:8 * b + w_dim] = b + 1.0
    want[table[1][0]:table[1][0] + B * 64] = 3.0
    assert x.grad.shape == x.shape and torch.equal(x.grad, want), 'one flat gradient; padding, unused views and the tail zero'
    # at B = 1 the views are unflatten's, with the batch dimensions in front
    t1, total1 = noise_reg.make_batched_table(1, w_dim, sizes)
    y = torch.arange(total1, dtype=torch.float32)
    w1, v1 = noise_reg.unflatten_batched(y, t1, 1, w_dim)
    head, u1 = noise_reg.unflatten(y, t1, head=w_dim)
    assert torch.equal(w1.view(-1), head) and all(torch.equal(a[0, 0], b) for a, b in zip(v1, u1))
    with pytest.raises(RuntimeError, match='past the end'):
        noise_reg.unflatten_batched(torch.zeros(total - 1), table, B, w_dim)
    with pytest.raises(RuntimeError, match='non-overlapping'):
        noise_reg.unflatten_batched(torch.zeros(total), noise_reg.make_batched_table(1, w_dim, sizes)[0], B, w_dim)


def test_batched_ops_refuse_cpu_tensors_and_bad_batches():
    from torch_utils.ops import noise_reg
    table, total = noise_reg.make_batched_table(2, 30, [4, 8])
    with pytest.raises(RuntimeError, match='ROCm'):
        noise_reg.noise_regularizer_batched(torch.zeros(total), table, 2)
    with pytest.raises(RuntimeError, match='ROCm'):
        noise_reg.normalize_noise_batched_(torch.zeros(total), table, 2)
    for B in (0, 65):
        with pytest.raises(RuntimeError, match='B must be in 1..64'):
            noise_reg.noise_regularizer_batched(torch.zeros(total), table, B)


# ---- the batched C entry points: symbols and argument checks only, no device work ----

def test_noise_reg_batched_symbols_and_argument_errors():
    import sg2hip
    L = sg2hip.lib()
    assert L.sg2_abi_version() == 11, 'additive entry points: the ABI version stays'
    names = ('sg2_noise_reg_batched_scratch_bytes', 'sg2_noise_reg_fwd_batched', 'sg2_noise_reg_bwd_batched',
             'sg2_noise_normalize_batched')
    for name in names:
        assert hasattr(L, name) and name in sg2hip.SIGNATURES
    nbytes, one = ctypes.c_int64(-1), ctypes.c_int64(-1)
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below fails its argument checks first

    def table(B):       # make_batched_table(B, 32, [4, 8, 16, 256])
        out, off = [], 32 * B
        for r in (4, 8, 16, 256):
            out += [off, r]
            off += B * r * r
        return sg2hip.i64arr(out)

    # a sample's share is the batch-1 scratch rounded up to 4 floats
    assert L.sg2_noise_reg_scratch_bytes(ctypes.byref(one), table(1), 4) == 0
    share = (one.value // 4 + 3) // 4 * 16
    for B in (1, 2, 3, 64):
        assert L.sg2_noise_reg_batched_scratch_bytes(ctypes.byref(nbytes), table(B), 4, B) == 0
        assert nbytes.value == B * share
    ok = table(3)

    def calls(t, n, B):
        return (L.sg2_noise_reg_batched_scratch_bytes(ctypes.byref(nbytes), t, n, B),
                L.sg2_noise_reg_fwd_batched(p, p, p, t, n, B, p, None),
                L.sg2_noise_reg_bwd_batched(p, p, p, p, t, n, B, p, 0, None),
                L.sg2_noise_normalize_batched(p, t, n, B, None))

    bad = [([0, 6], 1, 2, b'power of two'), ([0, 2048], 1, 2, b'power of two'), ([0, 4], 0, 2, b'nbuf'),
           ([2, 4], 1, 2, b'multiples of 4'), ([0, 4] * 33, 33, 2, b'nbuf'), ([0, 4], 1, 0, b'B must be in 1..64'),
           ([0, 4], 1, 65, b'B must be in 1..64'), ([0, 4], 1, -1, b'B must be in 1..64'),
           ([(1 << 29) - 2 * 1024 * 1024 - 4, 1024], 1, 3, b'2 GiB')]
    for t, n, B, msg in bad:
        for rc in calls(sg2hip.i64arr(t), n, B):
            assert rc != 0 and msg in L.sg2_last_error(), (t, n, B, L.sg2_last_error())
    # (the same table fits at B = 2: the bound counts all B samples of a buffer)
    assert L.sg2_noise_reg_batched_scratch_bytes(ctypes.byref(nbytes),
                                                 sg2hip.i64arr([(1 << 29) - 2 * 1024 * 1024 - 4, 1024]), 1, 2) == 0
    assert L.sg2_noise_reg_fwd_batched(p, p, p, ok, 4, 3, None, None) != 0 and b'scratch' in L.sg2_last_error()
    assert L.sg2_noise_reg_bwd_batched(p, p, p, p, ok, 4, 3, None, 0, None) != 0 and b'scratch' in L.sg2_last_error()
    assert L.sg2_noise_reg_batched_scratch_bytes(ctypes.byref(nbytes), None, 1, 3) != 0 and b'table' in L.sg2_last_error()
    assert L.sg2_noise_normalize_batched(None, ok, 4, 3, None) != 0 and b'non-null' in L.sg2_last_error()
    odd = ctypes.c_void_p(4100)
    assert L.sg2_noise_normalize_batched(odd, ok, 4, 3, None) != 0 and b'16-byte' in L.sg2_last_error()


# ---- the batched projection loop on a recording stub ----

class BatchStub:
    calls = []

    def __init__(self, outdir, device, modalities, dtype, **kwargs):
        self.kwargs = dict(outdir=outdir, modalities=modalities, dtype=dtype, **kwargs)
        BatchStub.calls = []

    @staticmethod
    def _w(num_steps, n, b=0):
        return torch.arange(num_steps * 8, dtype=torch.float32).view(num_steps, 2, 4) + 1000 * n + 100 * b

    def forward(self, id_patient, id_slice, target, num_steps, early_stopping, w_init=None, verbose=False):
        n = len(BatchStub.calls)
        BatchStub.calls.append(dict(kind='forward', ids=[(id_patient, id_slice)], num_steps=num_steps))
        return self._w(num_steps, n), num_steps - 1

    def forward_batch(self, ids, targets, num_steps, early_stopping, w_init=None, verbose=False):
        n = len(BatchStub.calls)
        BatchStub.calls.append(dict(kind='batch', ids=list(ids), shape=tuple(targets.shape), dtype=targets.dtype,
                                    num_steps=num_steps, early_stopping=early_stopping, verbose=verbose,
                                    w_init=None if w_init is None else w_init.clone()))
        # sample b's best step is b (mod num_steps): not the last, and not the same for all
        return torch.stack([self._w(num_steps, n, b) for b in range(len(ids))]), [b % num_steps for b in range(len(ids))]


def _best(num_steps, n, b):
    return BatchStub._w(num_steps, n, b)[b % num_steps]


def test_projection_loop_batched_control_flow(tmp_path, monkeypatch):
    import pickle
    import sys
    import projector_oracle as po
    import synth_zip
    from genlib.projector import projection_loop as pl
    from genlib import run_projector_mi_multimodal as cli
    monkeypatch.setattr(pl, '_device', lambda rank: torch.device('cpu'))
    data = str(tmp_path / 'data.zip')
    synth_zip.make_zip(data, modalities=tuple(po.MODALITIES), res=16, patients=3, slices=3)
    c, _, _, _ = cli.build_config(data=data, outdir=str(tmp_path / 'reports'), gpus=1, experiment='00003',
                                  network_pkl='network-snapshot-000100.pkl', num_steps=3, early_stopping=2,
                                  first_num_steps=5, first_early_stopping=77, verbose=True, batch=2)
    assert c.projector_kwargs.batch == 2
    assert cli.build_config(data=data, outdir=str(tmp_path), gpus=1, experiment='0', network_pkl='x')[0].projector_kwargs.batch == 1
    c.projector_kwargs.class_name = 'test_projector_batch_host.BatchStub'
    c.projector_kwargs.outdir_model = 'unused'

    def run(step, batch):
        c.projector_kwargs.step_patient_slice, c.projector_kwargs.batch = step, batch
        run_dir = tmp_path / f'run{step}_{batch}'
        run_dir.mkdir()
        pl.projection_loop(run_dir=str(run_dir), rank=0, **c)
        calls = sys.modules['test_projector_batch_host'].BatchStub.calls
        with open(run_dir / 'projected_w', 'rb') as f:
            return calls, pickle.load(f)

    P = [f'p{p:03d}' for p in range(3)]

    # every slice, 4 at a time: phase A is one short batch of the three first slices; phase B mixes patients and ends short
    calls, saved = run(1, 4)
    assert all(k['kind'] == 'batch' for k in calls)
    assert [k['ids'] for k in calls] == [[(P[0], 0), (P[1], 0), (P[2], 0)],
                                         [(P[0], 1), (P[0], 2), (P[1], 1), (P[1], 2)], [(P[2], 1), (P[2], 2)]]
    cold, warm = calls[0], calls[1:]
    assert (cold['num_steps'], cold['early_stopping'], cold['w_init'], cold['verbose']) == (5, 77, None, False)
    assert cold['shape'] == (3, 2, 16, 16) and cold['dtype'] == torch.float32
    firsts = {P[b]: _best(5, 0, b) for b in range(3)}       # every group's first best w
    for k in warm:
        assert (k['num_steps'], k['early_stopping'], k['verbose']) == (3, 2, True)
        assert k['shape'] == (len(k['ids']), 2, 16, 16) and k['w_init'].shape == (len(k['ids']), 2, 4)
        for b, (patient, _) in enumerate(k['ids']):         # a per-sample w_init: its OWN group's first best w
            assert torch.equal(k['w_init'][b], firsts[patient])
    assert type(saved) is dict and list(saved) == P, 'patients in dataset order'
    assert all(type(v) is dict and list(v) == ['00000', '00001', '00002'] for v in saved.values()), 'slices in dataset order'
    assert np.array_equal(saved[P[1]]['00000'], firsts[P[1]].numpy())
    assert np.array_equal(saved[P[1]]['00002'], _best(3, 1, 3).numpy()) and saved[P[1]]['00002'].dtype == np.float32
    assert np.array_equal(saved[P[2]]['00001'], _best(3, 2, 0).numpy())

    # items 0, 2, 4, 6, 8 of the whole dataset, 2 at a time: p000/0, p000/2 | p001/1 | p002/0, p002/2 are three groups
    calls, saved = run(2, 2)
    assert [k['ids'] for k in calls] == [[(P[0], 0), (P[1], 1)], [(P[2], 0)], [(P[0], 2), (P[2], 2)]]
    assert [k['w_init'] is None for k in calls] == [True, True, False]
    assert torch.equal(calls[2]['w_init'][0], _best(5, 0, 0)) and torch.equal(calls[2]['w_init'][1], _best(5, 1, 0))
    assert {p: list(v) for p, v in saved.items()} == {P[0]: ['00000', '00002'], P[1]: ['00001'], P[2]: ['00000', '00002']}
    assert list(saved) == P

    # batch = 1 is the sequential loop: forward_batch is never called
    calls, saved1 = run(1, 1)
    assert len(calls) == 9 and all(k['kind'] == 'forward' for k in calls)
    assert {p: list(v) for p, v in saved1.items()} == {p: ['00000', '00001', '00002'] for p in P}


# ---- forward_batch's composition path on the CPU oracle generator, pinned to the reference's fixture ----

@pytest.mark.parametrize('run', ['cold', 'warm'])
def test_forward_batch_composition_reproduces_the_reference(run, tmp_path, monkeypatch):
    """SG2_PROJ_FUSED=0 on a CPU device runs the torch composition with per-sample reductions: at B = 1 under the
    fixture's tape, and as sample 0 of a batch of three (fresh draws and other targets for its batch mates), every
    judged quantity is within the fixture's bounds of the reference-made run."""
    import os
    import projector_oracle as po
    from conftest import GOLDEN
    from rngtape import Tape
    from oracle import sg2_oracle as O
    from genlib.projector import projector as pj
    from metrics import metric_utils
    fix = po.load_fixture(os.path.join(GOLDEN, 'projector_ref.npz'))
    ref = fix[run]
    monkeypatch.setenv('SG2_PROJ_FUSED', '0')
    monkeypatch.setattr(metric_utils, '_detectors', {pj.LPIPS_URL: po.stand_in(fix['det'])})
    G = po.build_generator(O, fix['G'])
    p = pj.StyleGAN2Projector(outdir=str(tmp_path), device=torch.device('cpu'), modalities=po.MODALITIES, dtype='float32',
                              outdir_model=None, w_avg_samples=po.W_AVG_SAMPLES, G=G)

    def sample_run(b, w_steps):
        s = p.last['samples'][b]
        got = {k: np.asarray(v, np.float64) for k, v in s['history'].items()}
        got['w_out'] = w_steps[b][:, 0].double().numpy()
        got['grad0/w'] = s['first_grads']['w'].double().numpy()
        got.update({f'grad0/noise/{i}': g.double().numpy() for i, g in enumerate(s['first_grads']['noise'])})
        return got

    w0 = torch.from_numpy(ref['w_init']) if run == 'warm' else None
    with ref['tape'].replay():
        w_steps, best = p.forward_batch([('p000', 7)], torch.from_numpy(fix['target']), po.K_STEPS, 100000, w_init=w0,
                                        verbose_logger=False)
    assert ref['tape'].pos == len(ref['tape'].entries) and not p.last['fused']
    po.judge(sample_run(0, w_steps), ref, f'B=1 {run}', grads_tight=True)

    nbuf = len(po.noise_names(G))
    init0, steps0 = ref['tape'].entries[:nbuf], ref['tape'].entries[nbuf:]
    rs = np.random.RandomState(1)
    fresh = lambda a: rs.standard_normal(a.shape).astype(np.float32)
    tape = Tape(entries=list(init0) + [('randn', fresh(a)) for _ in range(2) for _, a in init0] +
                [('randn', np.concatenate([a, fresh(a), fresh(a)])) for _, a in steps0])
    targets = torch.from_numpy(np.concatenate([fix['target'], po.make_target(5), po.make_target(9)]))
    w_init = None if w0 is None else torch.stack([w0, w0 * 1.1, w0 * 0.9])
    with tape.replay():
        w_steps, best = p.forward_batch([('p000', 7), ('p001', 3), ('p001', 4)], targets, po.K_STEPS, 100000,
                                        w_init=w_init, verbose_logger=False)
    assert tape.pos == len(tape.entries) and w_steps.shape[:2] == (3, po.K_STEPS) and len(best) == 3
    po.judge(sample_run(0, w_steps), ref, f'B=3 {run} sample 0', grads_tight=True)
    assert len({round(s['best_loss'], 3) for s in p.last['samples']}) == 3, 'three different projections'
    assert sorted(os.listdir(tmp_path)) == ['p000', 'p001']
    assert len(os.listdir(tmp_path / 'p001' / 'projections')) == 2


def test_proj_loss_symbols_and_argument_errors():
    import sg2hip
    L = sg2hip.lib()
    names = ('sg2_proj_prep_scratch_bytes', 'sg2_proj_prep_fwd', 'sg2_proj_prep_bwd', 'sg2_sqdist_rows_scratch_bytes',
             'sg2_sqdist_rows_fwd', 'sg2_sqdist_rows_bwd')
    for name in names:
        assert hasattr(L, name) and name in sg2hip.SIGNATURES
    nbytes = ctypes.c_int64(-1)
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below fails its argument checks first
    # one partial per 256 groups of 4 f^2 elements, per (modality, sample)
    for (B, C, H), want in {(1, 1, 4): 1, (3, 2, 32): 3 * 2 * 1, (2, 3, 32): 2 * 3, (1, 1, 256): 64, (2, 1, 512): 2 * 64,
                            (1, 3, 1024): 192}.items():
        assert L.sg2_proj_prep_scratch_bytes(ctypes.byref(nbytes), B, C, H) == 0 and nbytes.value == 4 * want, (B, C, H)
    for (B, C, H), msg in {(0, 1, 8): b'B must be', (1, 0, 8): b'C must be', (1, 17, 8): b'C must be',
                           (1, 1, 2): b'power of two', (1, 1, 12): b'power of two', (1, 1, 2048): b'power of two'}.items():
        for rc in (L.sg2_proj_prep_scratch_bytes(ctypes.byref(nbytes), B, C, H),
                   L.sg2_proj_prep_fwd(p, p, p, p, B, C, H, p, 1 << 20, None),
                   L.sg2_proj_prep_bwd(p, p, p, p, p, B, C, H, None)):
            assert rc != 0 and msg in L.sg2_last_error(), (B, C, H, L.sg2_last_error())
    assert L.sg2_proj_prep_fwd(p, p, p, p, 1, 1, 8, p, 0, None) != 0 and b'scratch too small' in L.sg2_last_error()
    assert L.sg2_proj_prep_fwd(p, p, None, p, 1, 1, 8, p, 64, None) != 0 and b'non-null' in L.sg2_last_error()
    assert L.sg2_proj_prep_fwd(p, p, ctypes.c_void_p(4100), p, 1, 1, 8, p, 64, None) != 0 and b'aligned' in L.sg2_last_error()
    assert L.sg2_proj_prep_bwd(None, p, p, p, p, 1, 1, 8, None) != 0 and b'non-null' in L.sg2_last_error()

    assert L.sg2_sqdist_rows_scratch_bytes(ctypes.byref(nbytes), 6, 8193) == 0 and nbytes.value == 6 * 2 * 4
    assert L.sg2_sqdist_rows_scratch_bytes(ctypes.byref(nbytes), 1, 1) == 0 and nbytes.value == 4
    for (R, F), msg in {(0, 8): b'R must be', (65536, 8): b'R must be', (1, 0): b'F must be'}.items():
        for rc in (L.sg2_sqdist_rows_scratch_bytes(ctypes.byref(nbytes), R, F),
                   L.sg2_sqdist_rows_fwd(p, p, p, R, F, p, 1 << 20, None), L.sg2_sqdist_rows_bwd(p, p, p, p, R, F, None)):
            assert rc != 0 and msg in L.sg2_last_error(), (R, F, L.sg2_last_error())
    assert L.sg2_sqdist_rows_fwd(p, p, p, 2, 8193, p, 8, None) != 0 and b'scratch too small' in L.sg2_last_error()
    assert L.sg2_sqdist_rows_fwd(p, p, None, 2, 8, p, 64, None) != 0 and b'non-null' in L.sg2_last_error()
    assert L.sg2_sqdist_rows_bwd(p, None, p, p, 2, 8, None) != 0 and b'non-null' in L.sg2_last_error()
