"""The fused MMD kernel (sg2_poly_mmd_sums; torch_utils/ops/poly_mmd.py) and compute_kid on the GPU against the
float64 numpy oracle of kid_oracle.py, which test_kid_metric.py pins to the reference's numbers.

Shapes (kid_oracle.CASES): subset sizes one past a 32 x 32 fragment (33), inside one 128 x 128 tile (64, 100), one
past it (130: 2 x 2 tiles, the symmetric Grams skip one) and 2 * 128 + 1 (257: 3 x 3 tiles); K tails of 4 and 8
floats after whole 32-steps (d = 36, 136, 520) and the production d = 2048.
Tolerance: kid_oracle.REL = 16 x the measured error of the reference's own float32 arithmetic, on every one of the
3 S sums (see there); the KID bound follows from it.

Every test runs with the op module's torch.empty NaN-filled (poison.poisoned_empties): both the [S, 3] output and the
per-tile scratch are float64, so an element the call reads or returns without having written it is a NaN."""
import numpy as np
import pytest
import torch

import kid_oracle
import poison
from kid_oracle import REL

pytestmark = pytest.mark.gpu

DEV = 'cuda'
IDS = [kid_oracle.case_id(c) for c in kid_oracle.CASES]
SMALL = kid_oracle.CASES[1]


@pytest.fixture(autouse=True)
def _poisoned(monkeypatch):
    poison.poisoned_empties(monkeypatch, ['torch_utils.ops.poly_mmd'])


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _ratio(got, want):
    """Worst relative error of the sums over REL; NaN counts as inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.abs(want)
    return float(np.where(np.isnan(err), np.inf, err).max() / REL)


def _sums(gen, real, ig, ir):
    from torch_utils.ops import poly_mmd
    out = poly_mmd.subset_sums(gen, real, ig, ir)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(ig), 3) and out.device.type == 'cuda'
    return out


@pytest.mark.parametrize('case', kid_oracle.CASES, ids=IDS)
def test_sums_match_the_oracle(case):
    from torch_utils.ops import poly_mmd
    real, gen = kid_oracle.features(case)
    ig, ir = kid_oracle.draws(case)
    o = kid_oracle.oracle(case)
    got = _sums(_dev(gen), _dev(real), np.array(ig), np.array(ir)).cpu().numpy()
    ratio = _ratio(got, o['sums'])
    kid = poly_mmd.kid_from_sums(got, o['m'])
    print(f'{kid_oracle.case_id(case)}: worst relative error of the sums {ratio * REL:.3e} = {ratio:.3f} x REL '
          f'({REL:.3e}; cap {kid_oracle.cap(case[2]):.3e}); KID {kid:.7f}, float64 {o["kid"]:.7f}, '
          f'error {abs(kid - o["kid"]):.3e} of {kid_oracle.kid_bound(case):.3e}')
    assert ratio <= 1.0
    assert abs(kid - o['kid']) <= kid_oracle.kid_bound(case)


class _FilledEmpties(poison.TorchProxy):
    """torch.empty whose every byte is 0xff (a NaN in every float format, -1 in every integer one), counted."""

    def __init__(self):
        super().__init__()
        object.__setattr__(self, 'filled', [])

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        t.view(torch.uint8).fill_(255)
        self.filled.append(tuple(t.shape))
        return t


@pytest.mark.parametrize('case', [kid_oracle.CASES[0], kid_oracle.CASES[3]], ids=[IDS[0], IDS[3]])
def test_scratch_and_output_start_as_nan(case, monkeypatch):
    """The scratch the op allocates (and its output) filled with NaN bytes before the call: one tile (m = 33) and
    2 x 2 tiles, where the symmetric Grams leave one scratch slot unwritten -- and must not read it."""
    from torch_utils.ops import poly_mmd
    proxy = _FilledEmpties()
    monkeypatch.setattr(poly_mmd, 'torch', proxy)
    real, gen = kid_oracle.features(case)
    ig, ir = kid_oracle.draws(case)
    got = _sums(_dev(gen), _dev(real), np.array(ig), np.array(ir)).cpu().numpy()
    S, T = case[3], -(-kid_oracle.subset_size(case) // 128)
    assert sorted(proxy.filled) == sorted([(S, 3), (S * 3 * T * T,)])
    assert np.isfinite(got).all() and _ratio(got, kid_oracle.oracle(case)['sums']) <= 1.0


def test_two_calls_are_bitwise_equal(monkeypatch):
    from torch_utils.ops import poly_mmd
    case = kid_oracle.CASES[3]
    real, gen = kid_oracle.features(case)
    ig, ir = (np.array(t) for t in kid_oracle.draws(case))
    g, r = _dev(gen), _dev(real)
    first = _sums(g, r, ig, ir)
    assert torch.equal(_sums(g, r, ig, ir), first)
    with poison.unpoisoned([poly_mmd]):         # whatever the allocator hands out
        assert torch.equal(_sums(g, r, ig, ir), first)
    assert torch.equal(_sums(g.clone(), r.clone(), ig, ir), first)      # other addresses


def _hand_tables(n_gen, n_real, m):
    """S = 4, m positions: subset 0 holds row 0 and the last row of both sets at its ends; subsets 1 and 2 share most
    of their rows; subset 3 repeats one row of each set (two positions, one index: still two points)."""
    rs = np.random.RandomState(11)
    ig = np.stack([rs.choice(n_gen, m, replace=False) for _ in range(4)])
    ir = np.stack([rs.choice(n_real, m, replace=False) for _ in range(4)])
    for t, n in ((ig, n_gen), (ir, n_real)):
        rest = np.setdiff1d(t[0], [0, n - 1])
        t[0] = np.concatenate([[0], rest[:m - 2], [n - 1]])
        t[2, : m - 5] = t[1, 5:]
        t[3, m // 2] = t[3, 1]
    return ig, ir


def test_addressing_shared_rows_and_positions():
    case = SMALL
    n_real, n_gen, d = case[0], case[1], case[2]
    real, gen = kid_oracle.features(case)
    m = 67
    ig, ir = _hand_tables(n_gen, n_real, m)
    assert ig[0, 0] == 0 and ig[0, -1] == n_gen - 1 and ir[0, 0] == 0 and ir[0, -1] == n_real - 1
    assert len(np.intersect1d(ig[1], ig[2])) >= m - 5 and len(np.unique(ig[3])) == m - 1
    g, r = _dev(gen), _dev(real)
    got = _sums(g, r, ig, ir).cpu().numpy()
    want = kid_oracle.sums64(gen, real, ig, ir)
    print(f'hand-built tables: {_ratio(got, want):.3f} x REL')
    assert _ratio(got, want) <= 1.0
    # the same subsets with their positions permuted (each table on its own): the same sums
    rs = np.random.RandomState(12)
    pg = np.stack([row[rs.permutation(m)] for row in ig])
    pr = np.stack([row[rs.permutation(m)] for row in ir])
    perm = _sums(g, r, pg, pr).cpu().numpy()
    assert _ratio(perm, want) <= 1.0 and _ratio(perm, got) <= 1.0
    # one subset alone gives what it gives among others (the fold's order depends on (S, m) alone: bitwise)
    alone = _sums(g, r, ig[2:3], ir[2:3]).cpu().numpy()
    assert np.array_equal(alone[0], got[2])


@pytest.mark.parametrize('m', [100, 130])
def test_diagonal_is_left_out_by_position(m):
    """gen is real and idx_gen == idx_real: x = y, so Sxy - Sxx is the diagonal sum_i k(x_i, x_i) the xx Gram leaves
    out (one tile, and 2 x 2 tiles where only the diagonal tiles hold diagonal entries)."""
    case = kid_oracle.CASES[3]
    real, _ = kid_oracle.features(case)
    idx = np.stack([np.random.RandomState(21 + s).choice(real.shape[0], m, replace=False) for s in range(2)])
    x = _dev(real)
    got = _sums(x, x, idx, idx).cpu().numpy()
    assert np.array_equal(got[:, 0], got[:, 1])
    for s in range(2):
        diag = kid_oracle.diag64(real, idx[s])
        err = abs((got[s, 2] - got[s, 0]) - diag)
        print(f'm {m} subset {s}: Sxy - Sxx = {got[s, 2] - got[s, 0]:.6f}, diagonal {diag:.6f}, '
              f'error {err / (REL * got[s, 2]):.3f} x REL Sxy')
        assert err <= REL * got[s, 2]


def test_input_forms():
    """fp16 features and non-contiguous features give the sums of their float32 contiguous copies, bitwise; index
    tables may be tensors, int32 or strided."""
    case = SMALL
    real, gen = kid_oracle.features(case)
    ig, ir = (np.array(t) for t in kid_oracle.draws(case))
    g, r = _dev(gen), _dev(real)
    base = _sums(g, r, ig, ir)
    g16, r16 = g.to(torch.float16), r.to(torch.float16)
    assert torch.equal(_sums(g16, r16, ig, ir), _sums(g16.float(), r16.float(), ig, ir))
    wide_g = torch.zeros([g.shape[0], 2 * g.shape[1]], device=DEV)
    wide_g[:, ::2] = g
    rt = r.T.contiguous().T
    assert not wide_g[:, ::2].is_contiguous() and not rt.is_contiguous()
    assert torch.equal(_sums(wide_g[:, ::2], rt, ig, ir), base)
    assert torch.equal(_sums(g, r, torch.from_numpy(ig).to(DEV), torch.from_numpy(ir.astype(np.int32))), base)
    both = np.stack([ig, ir], axis=2)
    assert torch.equal(_sums(g, r, both[:, :, 0], both[:, :, 1]), base)
    with pytest.raises(RuntimeError, match='outside the'):
        _sums(g, r, ig + gen.shape[0], ir)
    with pytest.raises(RuntimeError, match='d must be'):
        _sums(g[:, :6], r[:, :6], ig, ir)


def test_compute_kid_end_to_end(tmp_path, monkeypatch):
    """compute_kid over the synthetic zip with the stub detector and generator, per modality: the fused kernel and the
    SG2_KID_FUSED=0 composition see the same features and draws and agree within the KID bound."""
    import dnnlib
    import synth_zip
    from stub_metric import StubDetector, StubGenerator
    from metrics import metric_utils, kernel_inception_distance as kid
    from torch_utils.ops import poly_mmd
    zpath = str(tmp_path / 'pelvis.zip')
    synth_zip.make_zip(zpath, modalities=('MR_MR_T2', 'MR_nonrigid_CT'), res=16, patients=3, slices=4, labels=False)
    dkw = dnnlib.EasyDict(class_name='training.dataset_mi_multimodal.CustomImageFolderDataset', path=zpath,
                          dtype='float32', split='train', use_labels=False, xflip=False, max_size=None,
                          modalities=['MR_MR_T2', 'MR_nonrigid_CT'])
    monkeypatch.setattr(metric_utils, '_detectors', {kid.DETECTOR_URL: StubDetector(res=16)})
    G = StubGenerator(c_dim=0, img_channels=2)
    recorded = []
    real_subset_sums = poly_mmd.subset_sums

    def recording(gen, real, ig, ir):
        recorded.append((tuple(gen.shape), tuple(real.shape), np.array(ig).shape, real_subset_sums(gen, real, ig, ir)))
        return recorded[-1][-1]

    monkeypatch.setattr(poly_mmd, 'subset_sums', recording)
    got = {}
    for fused in ('1', '0'):
        monkeypatch.setenv('SG2_KID_FUSED', fused)
        opts = metric_utils.MetricOptions(G=G, dataset_kwargs=dkw, device=torch.device(DEV, 0), cache=False,
                                          mode_dict=dict(mode_idx=1, mode_name='MR_nonrigid_CT'))
        np.random.seed(5)
        torch.manual_seed(6)
        got[fused] = kid.compute_kid(opts, max_real=50000, num_gen=20, num_subsets=3, max_subset_size=1000)
    (gshape, rshape, ishape, sums), = recorded                   # the composition did not call the kernel
    assert gshape == (20, 8) and rshape == (12, 8) and ishape == (3, 12)
    bound = kid_oracle.kid_bound(kid_oracle.kid_scale(sums.cpu().numpy(), 12))
    print(f'KID fused {got["1"]:.9f}, composition {got["0"]:.9f}, difference {abs(got["1"] - got["0"]):.3e} '
          f'of {bound:.3e}')
    assert np.isfinite(got['1']) and np.isfinite(got['0'])
    assert abs(got['1'] - got['0']) <= bound
