"""Average power spectra, the parts that need no GPU: the fixture check that pins batch_power_ref, kaiser_window, the
.npz format, construct_heatmap and the per-seed draws to the reference's own numbers (tests/golden/spectra_ref.npz,
written by tests/golden/make_spectra_golden.py), the tests' oracle and bound (spectra_oracle.py), avg_spectra.py's
commands on the CPU (where batch_power runs the composition), and the two entry points' argument errors."""
import ctypes
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import spectra_oracle as so
import synth_zip
from conftest import GOLDEN

FAKE = ctypes.c_void_p(4096)      # a non-null, aligned pointer: argument checks come before any device work


@pytest.fixture(scope='module')
def ref():
    with np.load(os.path.join(GOLDEN, 'spectra_ref.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def cli(monkeypatch):
    import avg_spectra
    monkeypatch.setattr(avg_spectra, '_device', lambda: torch.device('cpu'))
    monkeypatch.delenv('SG2_SPECTRA_FUSED', raising=False)
    return avg_spectra


def _params(ref):
    image_seed, num, size, mean, std, beta, interp, draw_seed, draw_num, z_dim, c_dim = ref['params']
    return dict(image_seed=int(image_seed), num=int(num), size=int(size), mean=float(mean), std=float(std),
                beta=float(beta), interp=int(interp), draw_seed=int(draw_seed), draw_num=int(draw_num),
                z_dim=int(z_dim), c_dim=int(c_dim))


def _fixture_images(p):
    return np.random.RandomState(p['image_seed']).randint(0, 256, size=[p['num'], 1, p['size'], p['size']]).astype(np.uint8)


# ---- the reference's numbers ----

def test_composition_reproduces_the_reference_fixture(ref):
    """The reference's window, and its outer product, are float32 (torch.kaiser_window's default dtype), widened when
    they meet the float64 image; batch_power_ref takes a float64 window and forms the product in float64.  The bound
    is worked out from exactly that difference: with D = |w[y] w[x] as batch_power_ref forms it - the reference's
    float32 product|, an image's F moves by at most dF = sum |whitened pixel| D, its power by 2 |F| dF + dF^2; plus
    1e-13 of the largest power for the float64 roundings of the two FFT runs and the order of the sum over images.
    Checked for the recorded float32 window widened (only the product's rounding differs) and for the op's own
    float64 window (the window's float32 rounding differs too)."""
    from torch_utils.ops import power_spectrum
    p = _params(ref)
    x = torch.from_numpy(_fixture_images(p))
    w32 = torch.from_numpy(ref['window_f32'])
    assert w32.dtype == torch.float32
    S = p['size'] * p['interp']
    want = ref['spectrum']
    assert want.dtype == np.float64 and want.shape == (S, S) and int(ref['image_size']) == p['size']
    w64 = power_spectrum.kaiser_window(p['size'], p['beta'])
    assert w64.dtype == torch.float64 and w64.device.type == 'cpu'
    assert abs(float(w64.square().sum()) - 1) < 1e-15
    # (the reference's window goes through float32 i0, sum, rsqrt and multiply: a few float32 ulp, 2^-21 allowed)
    assert (w64 - w32.double()).abs().max() <= 2.0 ** -21 * float(w64.max())
    white = ((x.double() - p['mean']) / p['std']).abs()
    for w in (w32.double(), w64):
        got = power_spectrum.batch_power_ref(x, [p['mean']], [p['std']], w, p['interp']) / p['num']
        assert got.dtype == torch.float64 and tuple(got.shape) == (1, S, S)
        D = (w.ger(w) - w32.ger(w32).double()).abs()
        dF = (white * D).sum(dim=[2, 3], keepdim=True)                           # [B, 1, 1, 1]
        F = power_spectrum.spectrum_ref(x, [p['mean']], [p['std']], w, p['interp']).abs()
        bound = (2 * F * dF + dF * dF).mean(dim=0)[0].numpy() + 1e-13 * want.max()
        err = np.abs(got[0].numpy() - want)
        print(f'worst error {err.max():.3g}, {float((err / bound).max()):.3f} of the bound; largest bound {bound.max():.3g}')
        assert bound.max() < 1e-5 * want.max()                                   # (the bound is a float32 rounding level)
        assert (err <= bound).all()


def test_npz_format_and_heatmap_match_the_reference(ref, tmp_path):
    from genlib import spectra
    p = _params(ref)
    dest = str(tmp_path / 'sub' / 'out.npz')
    spectra.save_spectrum(dest, ref['spectrum'], p['size'])
    with np.load(dest) as z:
        assert sorted(z.files) == list(ref['npz_keys']) == ['image_size', 'spectrum']
        assert z['spectrum'].dtype == np.float64 and np.array_equal(z['spectrum'], ref['spectrum'])
        assert z['image_size'].shape == () and z['image_size'].dtype == ref['image_size'].dtype
        assert int(z['image_size']) == p['size']
    for name, smooth in (('heatmap_smooth0', 0), ('heatmap_smooth125', 1.25)):
        db, size = spectra.construct_heatmap(dest, smooth)
        assert int(size) == p['size'] and db.shape == ref[name].shape == (65, 65)
        np.testing.assert_array_equal(db, ref[name])
    assert np.abs(ref['heatmap_smooth0'] - ref['heatmap_smooth125']).max() > 0.1


def test_latent_and_label_draws_match_the_reference(ref):
    from genlib import spectra
    p = _params(ref)
    assert ref['draw_z'].shape == (p['draw_num'], p['z_dim']) and ref['draw_c'].shape == (p['draw_num'], p['c_dim'])
    for i in range(p['draw_num']):
        z, k = spectra.latent_draw(p['draw_seed'] + i, p['z_dim'], p['c_dim'])
        assert z.dtype == np.float64 and z.shape == (1, p['z_dim'])
        np.testing.assert_array_equal(z[0], ref['draw_z'][i])
        onehot = np.zeros(p['c_dim'], dtype=np.float32)
        onehot[k] = 1
        np.testing.assert_array_equal(onehot, ref['draw_c'][i])
    assert spectra.latent_draw(3, 4, 0)[1] is None


class _StubG:
    """A generator that records what it is called with and returns an image made from z."""
    z_dim, c_dim, img_resolution, img_channels = 8, 3, 16, 2

    def __init__(self):
        self.calls = []

    def __call__(self, z, c, noise_mode='random'):
        self.calls.append((z.cpu().numpy().copy(), c.cpu().numpy().copy(), noise_mode))
        ramp = torch.linspace(-1.5, 1.5, 16 * 16, device=z.device).reshape(1, 1, 16, 16)
        return torch.tanh(z[:, :2].reshape(-1, 2, 1, 1) + ramp) * 1.2


def test_generator_source_batches_the_reference_draws_and_quantises(ref, monkeypatch):
    from genlib import generate, spectra
    p = _params(ref)
    G = _StubG()
    monkeypatch.setattr(generate, 'load_snapshot', lambda path, device: (G, None))
    n, size, names, it = spectra.stream_source_images('x.pkl', p['draw_num'], p['draw_seed'], torch.device('cpu'), batch=3)
    assert (n, size, names) == (p['draw_num'], 16, ['ch0', 'ch1'])
    batches = list(it)
    assert [b.shape[0] for b in batches] == [3, 1] and all(b.dtype == torch.uint8 for b in batches)
    z = np.concatenate([c[0] for c in G.calls])
    c = np.concatenate([c[1] for c in G.calls])
    assert z.dtype == np.float32
    np.testing.assert_array_equal(z, ref['draw_z'].astype(np.float32))
    np.testing.assert_array_equal(c, ref['draw_c'])
    assert {c[2] for c in G.calls} == {'random'}
    # the quantisation rule, and --float
    img = torch.cat([G(torch.from_numpy(a), torch.from_numpy(b)) for a, b, _ in G.calls[:2]])
    want = (img * 127.5 + 128).clamp(0, 255).to(torch.uint8)
    assert torch.equal(torch.cat(batches), want) and int(want.min()) == 0 and int(want.max()) == 255
    _, _, _, it = spectra.stream_source_images('x.pkl', 4, p['draw_seed'], torch.device('cpu'), batch=4, as_float=True,
                                               noise_mode='const')
    (f,) = list(it)
    assert f.dtype == torch.float32 and torch.equal(f, img * 127.5 + 128) and float(f.max()) > 255
    assert G.calls[-1][2] == 'const'


def test_quantisation_rules():
    from genlib import spectra
    g = torch.tensor([-1.5, -1.0, -0.004, 0.0, 0.0039, 0.5, 0.996, 1.0, 2.0])
    assert spectra.quantise_generated(g).tolist() == [0, 0, 127, 128, 128, 191, 254, 255, 255]
    r = torch.tensor([-3.0, 0.0, 0.99, 1.0, 127.5, 254.999, 255.0, 300.0])
    assert spectra.quantise_real(r).tolist() == [0, 0, 0, 1, 127, 254, 255, 255]


def test_dataset_source_quantises_unless_float(tmp_path):
    from genlib import spectra
    path = str(tmp_path / 'd.zip')
    synth_zip.make_zip(path, modalities=('CT', 'MR'), res=16, patients=2, slices=3, scale=300.0)
    cpu = torch.device('cpu')
    n, size, names, it = spectra.stream_source_images(path, None, 0, cpu, batch=4, modalities='CT,MR', as_float=True)
    assert (n, size, names) == (6, 16, ['CT', 'MR'])
    raw = torch.cat(list(it))
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (6, 2, 16, 16) and float(raw.max()) > 255
    _, _, _, it = spectra.stream_source_images(path, None, 0, cpu, batch=4, modalities='CT,MR')
    q = torch.cat(list(it))
    assert q.dtype == torch.uint8 and torch.equal(q, raw.clamp(0, 255).to(torch.uint8))
    # --num picks the reference's seeded subset; too many is the reference's error
    n, _, _, it = spectra.stream_source_images(path, 4, 3, cpu, modalities='MR', as_float=True)
    keep = np.sort(np.random.RandomState(3).permutation(6)[:4])
    assert n == 4 and torch.equal(torch.cat(list(it)), raw[keep][:, 1:2])
    with pytest.raises(spectra.SourceError, match='--source contains fewer than 7 images'):
        spectra.stream_source_images(path, 7, 0, cpu, modalities='CT')
    with pytest.raises(spectra.SourceError, match='network pickle or dataset zip'):
        spectra.stream_source_images(str(tmp_path), None, 0, cpu)


def test_mean_std_parsing_and_destination_names():
    from genlib import spectra
    assert spectra.parse_floats('112.684', 1, '--mean') == [112.684]
    assert spectra.parse_floats('112.684', 3, '--mean') == [112.684] * 3
    assert spectra.parse_floats('1,2.5', 2, '--std') == [1.0, 2.5]
    with pytest.raises(ValueError, match=r'--mean: 2 values for 3 modalities'):
        spectra.parse_floats('1,2', 3, '--mean')
    with pytest.raises(ValueError, match='cannot parse'):
        spectra.parse_floats('1;2', 2, '--mean')
    assert spectra.dest_paths('tmp/a.npz', ['CT']) == ['tmp/a.npz']
    assert spectra.dest_paths('tmp/a.npz', ['CT', 'MR']) == ['tmp/a-CT.npz', 'tmp/a-MR.npz']
    assert spectra.dest_paths('a', ['CT', 'MR']) == ['a-CT.npz', 'a-MR.npz']


# ---- the commands ----

def test_click_errors(cli, tmp_path):
    path = str(tmp_path / 'd.zip')
    synth_zip.make_zip(path, modalities=('CT', 'MR'), res=16, patients=2, slices=2)
    dest = str(tmp_path / 'o.npz')
    run = CliRunner().invoke
    res = run(cli.main, ['calc', '--source', 'snap.pkl', '--dest', dest, '--mean', '1', '--std', '1'])
    assert res.exit_code != 0 and '--num is required when --source points to network pickle' in res.output
    res = run(cli.main, ['stats', '--source', 'snap.pkl'])
    assert res.exit_code != 0 and '--num is required' in res.output
    res = run(cli.main, ['calc', '--source', path, '--modalities', 'CT,MR', '--dest', dest, '--mean', '1', '--std', '1',
                         '--num', '5'])
    assert res.exit_code != 0 and '--source contains fewer than 5 images' in res.output
    res = run(cli.main, ['calc', '--source', path, '--modalities', 'CT,MR', '--dest', dest, '--mean', '1,2,3', '--std', '1'])
    assert res.exit_code != 0 and '--mean: 3 values for 2 modalities' in res.output
    res = run(cli.main, ['calc', '--source', path, '--modalities', 'CT,MR', '--dest', dest, '--mean', '1', '--std', '1,0'])
    assert res.exit_code != 0 and '--std must be > 0' in res.output
    res = run(cli.main, ['calc', '--source', str(tmp_path / 'x.png'), '--dest', dest, '--mean', '1', '--std', '1'])
    assert res.exit_code != 0 and 'network pickle or dataset zip' in res.output
    assert not os.path.exists(dest)
    assert sorted(cli.main.commands) == ['calc', 'heatmap', 'slices', 'stats']


def test_stats_matches_numpy_float64(cli, tmp_path):
    from genlib import spectra
    path = str(tmp_path / 'd.zip')
    synth_zip.make_zip(path, modalities=('CT', 'MR'), res=16, patients=3, slices=3)
    res = CliRunner().invoke(cli.main, ['stats', '--source', path, '--modalities', 'CT,MR', '--batch', '4'],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    _, _, _, it = spectra.stream_source_images(path, None, 0, torch.device('cpu'), modalities='CT,MR')
    x = torch.cat(list(it)).numpy().astype(np.float64)
    mean = x.mean(axis=(0, 2, 3))
    std = np.sqrt((x * x).mean(axis=(0, 2, 3)) - mean * mean)
    lines = res.output.strip().splitlines()
    assert lines[0] == f'CT: --mean={mean[0]:g} --std={std[0]:g}'
    assert lines[1] == f'MR: --mean={mean[1]:g} --std={std[1]:g}'
    assert lines[2] == f'--mean={mean[0]:g},{mean[1]:g} --std={std[0]:g},{std[1]:g}'
    _, _, _, it = spectra.stream_source_images(path, None, 0, torch.device('cpu'), modalities='CT,MR', batch=5)
    m, s = spectra.channel_moments(it)
    assert m.dtype == np.float64 and np.abs(m - mean).max() < 1e-12 * 255 and np.abs(s - std).max() < 1e-11 * 255


def test_calc_writes_one_npz_per_modality_and_the_plots_save(cli, tmp_path):
    from torch_utils.ops import power_spectrum
    from genlib import spectra
    path = str(tmp_path / 'd.zip')
    synth_zip.make_zip(path, modalities=('CT', 'MR'), res=16, patients=2, slices=3)
    dest = str(tmp_path / 'out' / 'data.npz')
    res = CliRunner().invoke(cli.main, ['calc', '--source', path, '--modalities', 'CT,MR', '--dest', dest, '--mean',
                                        '120,131.5', '--std', '70', '--interp', '2', '--batch', '4'],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    _, _, _, it = spectra.stream_source_images(path, None, 0, torch.device('cpu'), modalities='CT,MR', batch=6)
    (x,) = list(it)
    want = power_spectrum.batch_power_ref(x, [120, 131.5], [70, 70], power_spectrum.kaiser_window(16, 8), 2) / 6
    files = [str(tmp_path / 'out' / f'data-{m}.npz') for m in ('CT', 'MR')]
    assert not os.path.exists(dest)
    for k, f in enumerate(files):
        with np.load(f) as z:
            assert z['spectrum'].dtype == np.float64 and z['spectrum'].shape == (32, 32) and int(z['image_size']) == 16
            assert np.abs(z['spectrum'] - want[k].numpy()).max() <= 1e-13 * float(want[k].max())
    # a single modality writes --dest itself
    one = str(tmp_path / 'one.npz')
    res = CliRunner().invoke(cli.main, ['calc', '--source', path, '--modalities', 'MR', '--dest', one, '--mean', '131.5',
                                        '--std', '70', '--interp', '2', '--num', '4', '--seed', '1'], catch_exceptions=False)
    assert res.exit_code == 0 and os.path.exists(one)
    png = str(tmp_path / 'plots' / 'h.png')
    res = CliRunner().invoke(cli.main, ['heatmap', files[0], '--save', png, '--dpi', '40'], catch_exceptions=False)
    assert res.exit_code == 0 and os.path.getsize(png) > 1000
    png2 = str(tmp_path / 'plots' / 's.png')
    res = CliRunner().invoke(cli.main, ['slices', files[0], files[1], '--save', png2, '--dpi', '40'], catch_exceptions=False)
    assert res.exit_code == 0 and os.path.getsize(png2) > 1000
    res = CliRunner().invoke(cli.main, ['slices', files[0], one, '--save', png2])
    assert res.exit_code == 0                           # same resolution: fine
    big = str(tmp_path / 'big.npz')
    spectra.save_spectrum(big, np.ones([64, 64]), 16)
    res = CliRunner().invoke(cli.main, ['slices', files[0], big, '--save', png2])
    assert res.exit_code != 0 and 'same resolution' in res.output


# ---- the op on the host ----

def test_oracle_bound_and_the_kernel_formulation_in_numpy():
    """DELTA_REF is a float64 rounding level; the reference's own FFT and the kernel's formulation in float64 numpy
    (two GEMMs, twiddles from the op's table, mirrored half) both lie well inside the bound on every element."""
    from torch_utils.ops import power_spectrum
    for case in so.CASES:
        N, interp, B, C, _ = case
        o = so.oracle(case)
        assert 2.0 ** -54 < o['delta_ref'] < 2.0 ** -44
        assert so.share(o['power_ref'], case) <= 0.25
        mean, std = so.moments(C)
        g = so.gemm_dft_f64(so.images(case), mean, std, so.window(N), interp)
        share = so.share(g, case)
        print(f'{so.case_id(case)}: DELTA_REF {o["delta_ref"]:.3g}, GEMM-DFT {share:.3f} of the bound, powers '
              f'{o["power"].min():.3g} .. {o["power"].max():.3g}')
        assert share <= 0.5
        S = N * interp
        tw = power_spectrum.twiddle_table(S)
        k = np.arange(1, S)
        assert np.array_equal(tw[S - k, 0], tw[k, 0]) and np.array_equal(tw[S - k, 1], -tw[k, 1])
        assert tuple(tw[0]) == (1.0, 0.0) and tuple(tw[S // 2]) == (-1.0, 0.0) and tuple(tw[S // 4]) == (0.0, -1.0)
        assert not np.signbit(tw[tw == 0]).any()
        ang = 2 * np.longdouble('3.14159265358979323846264338327950288') * np.arange(S).astype(np.longdouble) / S
        half_ulp = 2.0 ** -53                               # correctly rounded values of magnitude <= 1, nearly
        assert np.abs(tw[:, 0] - np.cos(ang)).max() <= 1.01 * half_ulp
        assert np.abs(tw[:, 1] + np.sin(ang)).max() <= 1.01 * half_ulp


def test_batch_power_checks_shapes_and_runs_the_composition_on_cpu():
    from torch_utils.ops import power_spectrum
    w = power_spectrum.kaiser_window(16, 8)
    x = torch.zeros([2, 3, 16, 16], dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r'images must be \[B, C, N, N\].*\[2, 3, 16, 12\]'):
        power_spectrum.batch_power(x[..., :12], [1] * 3, [1] * 3, w, 4)
    with pytest.raises(RuntimeError, match=r'B >= 1.*\[0, 3, 16, 16\]'):
        power_spectrum.batch_power(x[:0], [1] * 3, [1] * 3, w, 4)
    with pytest.raises(RuntimeError, match=r'mean \[2\] and std \[3\].*\[2, 3, 16, 16\]'):
        power_spectrum.batch_power(x, [1] * 2, [1] * 3, w, 4)
    with pytest.raises(RuntimeError, match=r'std must be > 0; got \[1.0, 0.0, 1.0\]'):
        power_spectrum.batch_power(x, [1] * 3, [1, 0, 1], w, 4)
    with pytest.raises(RuntimeError, match=r'window must be float64 \[16\]'):
        power_spectrum.batch_power(x, [1] * 3, [1] * 3, w[:8], 4)
    with pytest.raises(RuntimeError, match='uint8 or float32'):
        power_spectrum.batch_power(x.double(), [1] * 3, [1] * 3, w, 4)
    with pytest.raises(RuntimeError, match='interp'):
        power_spectrum.batch_power(x, [1] * 3, [1] * 3, w, 0)
    case = so.CASES[2]
    mean, std = so.moments(case[3])
    got = power_spectrum.batch_power(torch.from_numpy(np.array(so.images(case))), mean, std,
                                     torch.from_numpy(np.array(so.window(case[0]))), case[1])
    assert got.device.type == 'cpu' and so.share(got.numpy(), case) <= 0.25
    assert power_spectrum.kernel_takes(32, 1, 256, 4) and power_spectrum.kernel_takes(1, 1, 1024, 4)
    assert not power_spectrum.kernel_takes(1, 1, 1024, 5) and not power_spectrum.kernel_takes(1, 1, 18, 1)
    assert not power_spectrum.kernel_takes(1, 1, 4, 4)


def test_switch_and_default_size_threshold(monkeypatch):
    """Unset, the kernel runs below N = 512 (measured faster at 256, slower at 512 and 1024); 0 and 1 force a side."""
    from torch_utils.ops import power_spectrum
    monkeypatch.delenv('SG2_SPECTRA_FUSED', raising=False)
    assert power_spectrum.fused_enabled(8) and power_spectrum.fused_enabled(256) and power_spectrum.fused_enabled(508)
    assert not power_spectrum.fused_enabled(512) and not power_spectrum.fused_enabled(1024)
    monkeypatch.setenv('SG2_SPECTRA_FUSED', '1')
    assert power_spectrum.fused_enabled(1024) and power_spectrum.fused_enabled(8)
    monkeypatch.setenv('SG2_SPECTRA_FUSED', '0')
    assert not power_spectrum.fused_enabled(8) and not power_spectrum.fused_enabled(256)


def _lib():
    import sg2hip
    return sg2hip, sg2hip.lib()


def test_entry_points_exist_and_refuse_bad_arguments():
    """Argument checks only: every call returns before any launch."""
    hip, lib = _lib()
    assert 'sg2_power_spectrum_scratch_bytes' in hip.SIGNATURES and 'sg2_power_spectrum_sum' in hip.SIGNATURES
    assert lib.sg2_power_spectrum_scratch_bytes and lib.sg2_power_spectrum_sum and lib.sg2_abi_version() == 11
    b = ctypes.c_int64(0)
    sb = lib.sg2_power_spectrum_scratch_bytes
    assert sb(ctypes.byref(b), 1, 1, 8, 4) == 0
    # S = 32: T = 2 planes x 8 rows x 32 padded columns, one group of P = 32 x 17
    assert b.value == 2 * 8 * 32 * 8 + 32 * 17 * 8
    assert sb(ctypes.byref(b), 32, 1, 256, 4) == 0
    assert b.value == 32 * 2 * 256 * 544 * 8 + 4 * 1024 * 513 * 8          # four batch groups at the production shape
    # the plan of the cases that are about the batch groups: T = B C x 2 planes x N x Vp, P = G x C x S x (S / 2 + 1)
    for (N, interp, B, C), (G, per) in so.GROUPS.items():
        S = N * interp
        vh = S // 2 + 1
        assert sb(ctypes.byref(b), B, C, N, interp) == 0
        assert b.value == B * C * 2 * N * (-(-vh // 32) * 32) * 8 + G * C * S * vh * 8, (N, interp, B, C)
        assert (G - 1) * per < B <= G * per
        assert (N, interp, B, C) in [c[:4] for c in so.CASES]
    assert sb(None, 1, 1, 8, 4) == -1 and b'non-null' in lib.sg2_last_error()
    for n in (4, 6, 10, 1028, 2048, 0, -8):
        assert sb(ctypes.byref(b), 1, 1, n, 1) == -1 and b'multiple of 4 in 8..1024' in lib.sg2_last_error(), n
    assert sb(ctypes.byref(b), 1, 1, 16, 0) == -1 and b'interp must be >= 1' in lib.sg2_last_error()
    assert sb(ctypes.byref(b), 1, 1, 1024, 5) == -1 and b'<= 4096' in lib.sg2_last_error()
    assert sb(ctypes.byref(b), 0, 1, 16, 4) == -1 and b'B and C must be >= 1' in lib.sg2_last_error()
    assert sb(ctypes.byref(b), 1, 0, 16, 4) == -1 and b'B and C must be >= 1' in lib.sg2_last_error()
    assert sb(ctypes.byref(b), 70000, 1, 16, 4) == -1 and b'65535' in lib.sg2_last_error()
    big = 1 << 40
    strides = hip.i64arr([256, 256, 16, 1])

    def call(out=FAKE, img=FAKE, dtype=hip.U8, st=strides, B=2, C=1, N=16, interp=4, window=FAKE, mean=FAKE, std=FAKE,
             twiddle=FAKE, scratch=FAKE, nbytes=big):
        return lib.sg2_power_spectrum_sum(out, img, dtype, st, B, C, N, interp, window, mean, std, twiddle, scratch,
                                          nbytes, None)

    for name in ('out', 'img', 'st', 'window', 'mean', 'std', 'twiddle', 'scratch'):
        assert call(**{name: None}) == -1 and b'non-null' in lib.sg2_last_error(), name
    for n in (4, 18, 1028):
        assert call(N=n) == -1 and b'multiple of 4 in 8..1024' in lib.sg2_last_error(), n
    assert call(interp=0) == -1 and b'interp must be >= 1' in lib.sg2_last_error()
    assert call(N=1024, interp=8) == -1 and b'<= 4096' in lib.sg2_last_error()
    assert call(B=0) == -1 and b'B and C must be >= 1' in lib.sg2_last_error()
    assert call(dtype=hip.F16) == -1 and b'SG2_F32 or SG2_U8' in lib.sg2_last_error()
    assert call(twiddle=ctypes.c_void_p(4104)) == -1 and b'aligned' in lib.sg2_last_error()
    assert call(img=ctypes.c_void_p(4098), dtype=hip.F32) == -1 and b'4-byte aligned' in lib.sg2_last_error()
    assert sb(ctypes.byref(b), 2, 1, 16, 4) == 0
    assert call(nbytes=b.value - 1) == -1 and b'scratch too small' in lib.sg2_last_error()
