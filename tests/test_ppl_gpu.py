"""The perceptual path length metric on the GPU against the reference-made fixture (tests/golden/ppl_ref.npz) and the
CPU oracle (tests/ppl_oracle.py, pinned to the fixture by test_ppl_host.py).

  * every fixture case: the product's PPLSampler on the product's networks_stylegan2 with the fixture's state and
    draws (fed through forward(draws=...); torch's RNG is not patched on the GPU), on the fused and on the composed
    path: every per-sample distance within max(1e-4, 4 x the reference's own f32 spread) of the reference run, and for
    the 128-sample cases the ppl within its bound of the same kind; fused against composed on the same draws within
    1e-5 (the same images; only the order of the feature sum differs);
  * compute_ppl end to end on a registered stand-in: the same seed gives the same float, and the CPU oracle recomputed
    from the draws actually used agrees within the ('w', 'end', 1e-4) bound;
  * the offline CLI in-process with a test-registered metric on a snapshot written by legacy.save_network_pkl.

Measured on the MI355X (profiles/ppl/tests_gpu.txt): per-sample errors 2.6e-2 / 2.2e-2 (bounds 0.124 / 0.118) and ppl errors
8.4e-4 / 1.4e-4 (bounds 4.4e-3 / 4.9e-3) on the two 128-sample cases; 2.2e-4 at epsilon = 1e-2 (bounds 1.1e-3 and
8.5e-4); 0.116 in Z (bound 0.223); fused against composed at most 2.5e-7.
"""
import json
import os

import numpy as np
import pytest
import torch

import ppl_oracle as pp
import projector_oracle as po
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def fix():
    f = pp.load_fixture(os.path.join(GOLDEN, 'ppl_ref.npz'))
    f['G'] = po.load_fixture(os.path.join(GOLDEN, 'projector_ref.npz'))['G']
    return f


@pytest.fixture(scope='module')
def product_G(fix):
    from training import networks_stylegan2 as net
    return po.build_generator(net, fix['G']).to(DEV)


def _run(fix, G, case, fused, monkeypatch):
    from metrics import perceptual_path_length as ppl
    monkeypatch.setenv('SG2_PPL_FUSED', '1' if fused else '0')
    kw = dict(pp.CASES[case])
    n, mode_idx = kw.pop('num_samples'), kw.pop('mode_idx')
    sampler = ppl.PPLSampler(G, {}, vgg16=po.stand_in(fix['det']),
                             mode_dict={'mode_name': po.MODALITIES[mode_idx], 'mode_idx': mode_idx}, **kw)
    sampler.eval().requires_grad_(False).to(DEV)
    c = torch.zeros([pp.BATCH, G.c_dim], device=DEV)
    draws = pp.tape_draws(fix['cases'][case]['tape'], G, n // pp.BATCH)
    dist = torch.cat([sampler(c, draws=d) for d in draws])
    assert sampler.last_fused == fused and dist.shape == (n,) and dist.dtype == torch.float32
    return dist.cpu().double().numpy()


@pytest.mark.parametrize('case', list(pp.CASES))
def test_sampler_against_the_reference(fix, product_G, case, monkeypatch):
    from metrics import perceptual_path_length as ppl
    ref = fix['cases'][case]
    before = {n: b.clone() for n, b in product_G.named_buffers() if 'noise_const' in n}
    with_ppl = pp.CASES[case]['num_samples'] >= 100
    got, bad = {}, []
    for fused in (True, False):
        got[fused] = _run(fix, product_G, case, fused, monkeypatch)
        what = f'{case} {"fused" if fused else "composition"}'
        try:
            pp.judge(got[fused], ref, what, with_ppl=with_ppl,
                     got_ppl=ppl.ppl_from_distances(got[fused].astype(np.float32)) if with_ppl else None)
        except AssertionError as err:
            bad.append(str(err))
    ab = float(pp.rel_each(got[True], got[False]).max())
    print(f'{case}: fused against composition on the same draws: rel {ab:.3g} (bound 1e-05)')
    assert not bad, bad
    assert ab <= 1e-5
    assert all(torch.equal(b, before[n]) for n, b in product_G.named_buffers() if 'noise_const' in n), \
        'the generator handed in keeps its noise'


def test_compute_ppl_end_to_end(fix, product_G, monkeypatch):
    from metrics import metric_utils
    from metrics import perceptual_path_length as ppl
    from oracle import sg2_oracle as O
    monkeypatch.setenv('SG2_PPL_FUSED', '1')
    det = po.stand_in(fix['det'])
    monkeypatch.setattr(metric_utils, '_detectors', {ppl.DETECTOR_URL: det})
    opts = metric_utils.MetricOptions(G=product_G, num_gpus=1, rank=0, device=torch.device(DEV),
                                      mode_dict={'mode_name': po.MODALITIES[0], 'mode_idx': 0})
    args = dict(num_samples=16, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2)
    used = []
    torch.manual_seed(11)
    first = ppl.compute_ppl(opts, draws_out=used, **args)
    torch.manual_seed(11)
    second = ppl.compute_ppl(opts, **args)
    print(f'compute_ppl, 16 samples: {first!r} and {second!r}')
    assert np.isfinite(first) and first == second, 'the same seed gives the same float'
    assert len(used) == 8
    got = torch.cat([d for _, _, d in used]).cpu().double().numpy()
    assert first == ppl.ppl_from_distances(got.astype(np.float32))
    # the CPU oracle on the draws actually used
    G = po.build_generator(O, fix['G'])
    cpu = po.stand_in(fix['det'])
    want = torch.cat([pp.sample(G, cpu, c.cpu(), 1e-4, 'w', 'end', False, mode_idx=0,
                                draws=(t.cpu(), z.cpu(), [n.cpu() for n in noise]))
                      for c, (t, z, noise) in [(c, d) for c, d, _ in used]]).double().numpy()
    (bound, spread), _ = pp.bounds(fix['cases']['wend_e4_m0'])
    err = pp.rel_each(got, want)
    print(f'compute_ppl against the CPU oracle on its own draws: per-sample rel error max {err.max():.3g} median '
          f'{np.median(err):.3g} (bound {bound:.3g}, reference spread {spread:.3g})')
    assert err.max() <= bound
    assert len({float(t[0]) for _, (t, _, _), _ in used}) == 8, 'every call draws afresh'


def test_cli_in_process(fix, tmp_path, monkeypatch):
    """calc_metrics_mi_multimodal on the GPU: a test-registered metric that calls compute_ppl with 8 samples."""
    import legacy
    from click.testing import CliRunner
    import calc_metrics_mi_multimodal as cli
    from metrics import metric_main_mi_multimodal as mm
    from metrics import metric_utils
    from metrics import perceptual_path_length as ppl
    from training import networks_stylegan2 as net
    monkeypatch.setattr(metric_utils, '_detectors', {ppl.DETECTOR_URL: po.stand_in(fix['det'])})

    def ppl_test8(opts):
        return dict(ppl_test8=ppl.compute_ppl(opts, num_samples=8, epsilon=1e-4, space='w', sampling='end', crop=False,
                                              batch_size=2))

    monkeypatch.setattr(mm._REGISTRY, 'fns', dict(mm._REGISTRY.fns))
    mm.register_metric(ppl_test8)
    G = po.build_generator(net, fix['G'])
    kw = dict(c_dim=0, img_resolution=32, img_channels=2, channel_base=128, channel_max=16)
    D = net.Discriminator(num_fp16_res=0, **kw)
    run = tmp_path / 'run'
    run.mkdir()
    (run / 'training_options.json').write_text('{}')
    path = str(run / 'network-snapshot-000001.pkl')
    legacy.save_network_pkl(path, G, D, G, None, dict(path='unused.zip', modalities=po.MODALITIES))
    res = CliRunner().invoke(cli.calc_metrics, ['--network', path, '--metrics', 'ppl_test8', '--verbose', 'False'],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    values = []
    for m in po.MODALITIES:
        with open(run / f'metric-{m}-ppl_test8.jsonl') as f:
            lines = [json.loads(line) for line in f]
        assert len(lines) == 1 and lines[0]['mode'] == m and lines[0]['snapshot_pkl'] == 'network-snapshot-000001.pkl'
        assert np.isfinite(lines[0]['results']['ppl_test8']) and lines[0]['results']['ppl_test8'] > 0
        values.append(lines[0]['results']['ppl_test8'])
    print(f'CLI: ppl of 8 samples per modality {values}')
    assert values[0] != values[1]
