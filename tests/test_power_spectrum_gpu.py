"""The fused power-spectrum kernel (sg2_power_spectrum_sum; torch_utils/ops/power_spectrum.py) and avg_spectra.py's
`calc` on the GPU against the long-double oracle of spectra_oracle.py.

Shapes (spectra_oracle.CASES): the smallest accepted size (N = 8), one tile per side (S = 64), S = 60 with tile and K
tails and two channels, S = N, several tiles with an odd batch and three channels, S = 256 with the batch split into
groups, float32 pixels; batches of 17 and 33 small images, which the kernel's plan runs as groups of 2 and 3 images
with a short last group (the column pass's loop over a group's images), and N = 72 and 128 (more than one block of rows
in the row pass).
Tolerance: every element of out within sum_b (2 sqrt(P_b) delta + delta^2), delta = 16 x the measured error of the
reference's own float64 FFT composition (spectra_oracle); no element is left out.

Every test runs with the op module's torch.empty NaN-filled (poison.poisoned_empties): output and scratch are float64,
so an element the call reads or returns without having written it is a NaN."""
import os

import numpy as np
import pytest
import torch

import poison
import spectra_oracle as so

pytestmark = pytest.mark.gpu

DEV = 'cuda'
IDS = [so.case_id(c) for c in so.CASES]
MULTI = so.CASES[4]         # (48, 2, 5, 3): three channels, five images
SPLIT = so.CASES[5]         # (64, 4, 4, 1): the batch runs as several groups (of one image each)
LOOPS = so.CASES[7:9]       # (8, 4, 17, 1), (8, 4, 33, 2): several images per group, a short last group
ROWS = so.CASES[9:11]       # (72, 1, 2, 1), (128, 2, 3, 1): more than one block of rows in the row pass


@pytest.fixture(autouse=True)
def _poisoned(monkeypatch):
    monkeypatch.delenv('SG2_SPECTRA_FUSED', raising=False)
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.power_spectrum'])


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _power(x, mean, std, w, interp):
    from torch_utils.ops import power_spectrum
    x = x if isinstance(x, torch.Tensor) else _dev(x)
    out = power_spectrum.batch_power(x, mean, std, torch.from_numpy(np.array(w)), interp)
    S = x.shape[2] * interp
    assert out.dtype == torch.float64 and tuple(out.shape) == (x.shape[1], S, S) and out.device.type == 'cuda'
    return out


def _case_power(case, x=None):
    N, interp, B, C, _ = case
    mean, std = so.moments(C)
    return _power(so.images(case) if x is None else x, mean, std, so.window(N), interp)


def _mirror(S):
    return (S - np.arange(S)) % S


@pytest.mark.parametrize('case', so.CASES, ids=IDS)
def test_power_matches_the_oracle(case):
    got = _case_power(case).cpu().numpy()
    share = so.share(got, case)
    print(f'{so.case_id(case)}: DELTA_REF {so.DELTA_REF(case):.3g}, worst error {share:.3f} of the bound')
    assert share <= 1.0


@pytest.mark.parametrize('case', so.CASES, ids=IDS)
def test_two_calls_give_equal_bits_and_hermitian_symmetry(case):
    a, b = _case_power(case), _case_power(case)
    assert torch.equal(a, b)
    m = torch.from_numpy(_mirror(a.shape[1])).to(DEV)
    assert torch.equal(a, a[:, m][:, :, m])             # includes the self-mirrored lines v = 0 and v = S / 2


@pytest.mark.parametrize('case', [MULTI, SPLIT] + LOOPS + ROWS,
                         ids=[so.case_id(c) for c in [MULTI, SPLIT] + LOOPS + ROWS])
def test_batch_equals_the_sum_of_single_image_calls(case):
    N, interp, B, C, _ = case
    x = _dev(so.images(case))
    whole = _case_power(case, x).cpu().numpy()
    singles = np.stack([_case_power(case, x[b:b + 1]).cpu().numpy() for b in range(B)])
    o = so.oracle(case)
    for b in range(B):                                  # each single-image call against its own bound
        err = np.abs(singles[b] - o['per_image'][b])
        assert (err <= so.bound_of(o['per_image'][b:b + 1], o['delta_ref'])).all()
    assert (np.abs(whole - singles.sum(axis=0)) <= o['bound']).all()
    assert so.share(singles.sum(axis=0), case) <= 1.0


def test_channel_is_unaffected_by_its_neighbours():
    N, interp, B, C, _ = MULTI
    x = so.images(MULTI)
    mean, std = so.moments(C)
    base = _power(x, mean, std, so.window(N), interp)
    y = np.array(x)
    y[:, 0] = 255 - y[:, 0]
    y[:, 2] = 7
    mean2, std2 = mean.copy(), std.copy()
    mean2[0], std2[0], mean2[2], std2[2] = 3.5, 200.0, 250.0, 0.125
    other = _power(y, mean2, std2, so.window(N), interp)
    assert torch.equal(base[1], other[1])
    alone = _power(np.ascontiguousarray(x[:, 1:2]), mean[1:2], std[1:2], so.window(N), interp)
    assert torch.equal(base[1], alone[0])


@pytest.mark.parametrize('case', [so.CASES[2], SPLIT], ids=[so.case_id(so.CASES[2]), so.case_id(SPLIT)])
def test_uint8_and_float32_of_the_same_values_give_equal_bits(case):
    x = so.images(case)
    assert x.dtype == np.uint8
    assert torch.equal(_case_power(case, _dev(x)), _case_power(case, _dev(x.astype(np.float32))))


def test_non_contiguous_views_equal_their_copies():
    N, interp, B, C, _ = MULTI
    x = _dev(so.images(MULTI))
    mean, std = so.moments(C)
    w = so.window(N)
    view = x[:, 1:3]                                    # a channel slice
    assert not view.is_contiguous()
    assert torch.equal(_power(view, mean[1:3], std[1:3], w, interp),
                       _power(view.contiguous(), mean[1:3], std[1:3], w, interp))
    crop = x[:, :, 5:5 + 20, 9:9 + 20]                  # a crop of a larger image
    assert not crop.is_contiguous()
    assert torch.equal(_power(crop, mean, std, so.window(20), 3), _power(crop.contiguous(), mean, std, so.window(20), 3))
    tr = x.transpose(2, 3)                              # x stride larger than y stride
    assert torch.equal(_power(tr, mean, std, w, interp), _power(tr.contiguous(), mean, std, w, interp))


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_constant_image_at_the_mean_gives_exact_zeros(dtype):
    x = np.full([3, 2, 20, 20], 100, dtype=dtype)
    x[:, 1] = 37
    out = _power(x, [100.0, 37.0], [69.5, 3.0], so.window(20), 3)
    assert torch.equal(out, torch.zeros_like(out))


def test_single_bright_pixel_has_a_flat_spectrum():
    N, interp, y0, x0 = 16, 4, 5, 11
    x = np.full([1, 1, N, N], 16, dtype=np.uint8)
    x[0, 0, y0, x0] = 255
    mean, std = 16.0, 69.509
    w = so.window(N)
    got = _power(x, [mean], [std], w, interp).cpu().numpy()
    amp = np.longdouble(255 - mean) / np.longdouble(std) * (np.longdouble(w[y0]) * np.longdouble(w[x0]))
    want = float(amp * amp)
    assert want > 1e-4
    # |F| = amp at every bin; the bound with delta from the case of this size (16, 4)
    delta = so.MARGIN * so.DELTA_REF(so.CASES[1])
    bound = 2 * float(amp) * delta + delta * delta
    worst = float(np.abs(got - want).max())
    print(f'single pixel: power {want:.6g}, worst error {worst:.3g} = {worst / bound:.3f} of the bound')
    assert got.shape == (1, N * interp, N * interp) and worst <= bound


def test_switch_selects_the_composition(monkeypatch):
    from torch_utils.ops import power_spectrum
    case = so.CASES[2]
    calls = []
    real = power_spectrum.batch_power_ref
    monkeypatch.setattr(power_spectrum, 'batch_power_ref', lambda *a: calls.append(1) or real(*a))
    fused = _case_power(case)
    assert not calls
    monkeypatch.setenv('SG2_SPECTRA_FUSED', '0')
    ref = _case_power(case)
    assert calls == [1]
    assert so.share(ref.cpu().numpy(), case) <= 1.0 and so.share(fused.cpu().numpy(), case) <= 1.0
    monkeypatch.setenv('SG2_SPECTRA_FUSED', '1')
    assert torch.equal(_case_power(case), fused) and calls == [1]


# ---- end to end: avg_spectra.py calc on the GPU against batch_power_ref on the CPU ----

class _StubG:
    """A generator on the device: a smooth image per (z, c), past [-1, 1] in places so that the clamp is exercised."""
    z_dim, c_dim, img_resolution, img_channels = 8, 3, 32, 2

    def __call__(self, z, c, noise_mode='random'):
        assert noise_mode == 'random' and z.dtype == torch.float32 and z.device.type == 'cuda'
        r = torch.linspace(-2.0, 2.0, 32, device=z.device)
        grid = r.reshape(1, 1, 32, 1) * z[:, 0:2].reshape(-1, 2, 1, 1) + r.reshape(1, 1, 1, 32) * z[:, 2:4].reshape(-1, 2, 1, 1)
        return torch.sin(3 * grid + c.argmax(dim=1).reshape(-1, 1, 1, 1)) * 1.1


def _calc_bound(x_cpu, mean, std, w, interp):
    """(batch_power_ref on the CPU / count, the bound / count) of a CPU image stack: the bound of spectra_oracle with
    DELTA_REF measured on these very images (the CPU composition against the long-double definition)."""
    from torch_utils.ops import power_spectrum
    F = power_spectrum.spectrum_ref(x_cpu, mean, std, w, interp).numpy()
    fr, fi = so.spectrum_ld(x_cpu.numpy(), mean, std, w.numpy(), interp)
    delta_ref = float(np.hypot(F.real.astype(np.longdouble) - fr, F.imag.astype(np.longdouble) - fi).max())
    n = x_cpu.shape[0]
    want = power_spectrum.batch_power_ref(x_cpu, mean, std, w, interp).numpy() / n
    return want, so.bound_of((fr * fr + fi * fi).astype(np.float64), delta_ref) / n


def _check_files(files, want, bound, S, size):
    for k, f in enumerate(files):
        with np.load(f) as z:
            got = z['spectrum']
            assert got.dtype == np.float64 and got.shape == (S, S) and int(z['image_size']) == size
        share = float(np.max(np.abs(got - want[k]) / bound[k]))
        print(f'{os.path.basename(f)}: worst error {share:.3f} of the bound')
        assert np.isfinite(got).all() and share <= 1.0


def test_calc_on_the_synthetic_zip(tmp_path):
    """calc over 9 two-modality 48 x 48 slices in batches of 4 (4 + 4 + 1): the fused result against batch_power_ref on
    the CPU within the kernel's bound divided by the count."""
    import avg_spectra
    import synth_zip
    from click.testing import CliRunner
    from genlib import spectra
    from torch_utils.ops import power_spectrum
    path = str(tmp_path / 'd.zip')
    synth_zip.make_zip(path, modalities=('CT', 'MR'), res=48, patients=3, slices=3)
    dest = str(tmp_path / 'data.npz')
    res = CliRunner().invoke(avg_spectra.main, ['calc', '--source', path, '--modalities', 'CT,MR', '--dest', dest,
                                                '--mean', '127.3,120', '--std', '73.5,70', '--interp', '2', '--batch', '4'],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    _, _, _, it = spectra.stream_source_images(path, None, 0, torch.device('cpu'), modalities='CT,MR', batch=9)
    (x,) = list(it)
    assert x.dtype == torch.uint8
    want, bound = _calc_bound(x, [127.3, 120], [73.5, 70], power_spectrum.kaiser_window(48, 8), 2)
    _check_files([str(tmp_path / f'data-{m}.npz') for m in ('CT', 'MR')], want, bound, 96, 48)


def test_calc_on_a_stub_generator(tmp_path, monkeypatch):
    import avg_spectra
    from click.testing import CliRunner
    from genlib import generate, spectra
    from torch_utils.ops import power_spectrum
    monkeypatch.setattr(generate, 'load_snapshot', lambda path, device: (_StubG(), dict(modalities=['CT', 'MR'])))
    dest = str(tmp_path / 'gen.npz')
    res = CliRunner().invoke(avg_spectra.main, ['calc', '--source', 'stub.pkl', '--dest', dest, '--num', '5', '--seed', '3',
                                                '--mean', '128', '--std', '60,75', '--batch', '2'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    _, _, names, it = spectra.stream_source_images('stub.pkl', 5, 3, torch.device('cuda'), batch=5)
    (x,) = list(it)
    assert names == ['CT', 'MR'] and x.dtype == torch.uint8 and int(x.min()) == 0 and int(x.max()) == 255
    want, bound = _calc_bound(x.cpu(), [128, 128], [60, 75], power_spectrum.kaiser_window(32, 8), 4)
    _check_files([str(tmp_path / f'gen-{m}.npz') for m in ('CT', 'MR')], want, bound, 128, 32)
