"""The producer / consumer contract of the ADA geometric chain as region arithmetic (no kernel, no GPU).

Every kernel of the chain stores the logical image plus a band (64 rows / columns in reflect_pad_kernel, kZeroBand =
32 in the limited FIR passes, 96 in zero_region_kernel and the deterministic gather) and leaves the rest of its
static buffer untouched; every consumer is trusted to read no further.  tests/ada_regions.py states the regions;
here each consumer's furthest read, derived from its taps, padding and extent, must lie inside what its producer
stored (or inside the static buffer's clamp), and every zero band must be exact: beyond the producer's computed
extent the true value is zero.  test_ada_geom_gpu.py holds the kernels to the same regions on poisoned buffers.
"""
import itertools
import os
import re

import pytest

import ada_regions as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gan-track_amd', 'csrc')
PKG = os.path.dirname(CSRC)


def _src(*path):
    with open(os.path.join(PKG, *path)) as f:
        return f.read()


def test_constants_mirror_the_sources():
    """The mirrors of ada_regions.py against the lines they name."""
    gs, upf, aug, py = (_src('csrc', 'grid_sample.hip'), _src('csrc', 'upfirdn2d.hip'), _src('csrc', 'augment.hip'),
                        _src('training', 'augment_mi.py'))
    # csrc/grid_sample.hip:204 (reflect_pad_kernel)
    m = re.search(r'hl = min\(Hs, Hd \+ (\d+)\), wl = min\(Ws, Wd \+ (\d+)\)', gs)
    assert m and {int(m.group(1)), int(m.group(2))} == {R.PAD_BAND}
    # csrc/upfirdn2d.hip:53
    m = re.search(r'constexpr int kZeroBand = (\d+);', upf)
    assert m and int(m.group(1)) == R.FIR_BAND
    # csrc/grid_sample.hip:309 (the scatter's zero fill) and :126 (the deterministic gather)
    m = re.search(r'zero_region_kernel<<<[^>]*>>>\(gin, p, dyn_hw, (\d+)\)', gs)
    assert m and int(m.group(1)) == R.GRAD_BAND
    m = re.search(r'hl = p\.dyn_hw \? min\(p\.Hi, Hi \+ (\d+)\) : p\.Hi, wl = p\.dyn_hw \? min\(p\.Wi, Wi \+ (\d+)\)', gs)
    assert m and {int(m.group(1)), int(m.group(2))} == {R.GRAD_BAND}
    # the extents: csrc/augment.hip:133 and training/augment_mi.py:270-271
    sym = {'hd': 1000, 'wd': 10}
    want = [v for pair in R.lims(sym['hd'], sym['wd']) for v in pair]
    m = re.search(r'const int l\[8\] = \{([^}]*)\};', aug)
    assert m and [eval(e.strip(), {}, sym) for e in m.group(1).split(',')] == want
    m = re.search(r'lims = torch\.stack\(\[([^\]]*)\]\)', py)
    assert m and [eval(e.strip(), {}, sym) for e in m.group(1).split(',')] == want
    # the padding of the up-2 pass (torch_utils/ops/upfirdn2d.py upsample2d_limited) and of its adjoint
    fw, up = R.TAPS, 2
    assert ((fw + up - 1) // 2, (fw - up) // 2) == (R.UP_PAD0, R.UP_PAD0 - 1)
    assert fw - R.UP_PAD0 - 1 == R.ADJ_PAD0


@pytest.mark.parametrize('up,down,pad0,taps', [(2, 1, 6, 12), (1, 2, 5, 12), (1, 1, 2, 5), (3, 2, 4, 7)])
def test_reach_and_support_against_enumeration(up, down, pad0, taps):
    """reach() and support() against every (output, tap) pair of the definition."""
    def inputs(o):
        return [u // up for u in (o * down - pad0 + t for t in range(taps)) if u % up == 0]
    for n_out in range(0, 40):
        far = max([i for o in range(n_out) for i in inputs(o)] + [-1]) + 1
        assert R.reach(n_out, up, down, pad0, taps) == far
    for n_in in range(0, 30):
        s = R.support(n_in, up, down, pad0)
        assert all(i >= n_in for o in range(s, s + 8) for i in inputs(o))


@pytest.mark.parametrize('h', [32, 128, 256])
def test_every_consumer_reads_inside_its_producer(h):
    w = h
    values = [0, 1, h // 2, h - 1]
    for margins in itertools.product(values, repeat=4):
        ch = R.chain(h, w, margins)
        for name in ('pad', 'fh', 'fv', 'sg', 'ah', 'av'):
            st = ch[name]
            # a zero band is exact: the true value vanishes beyond the computed extent (or the buffer ends first)
            assert st['support'][0] <= st['computed'][0] and st['support'][1] <= st['computed'][1], (margins, name, st)
            assert st['computed'][0] <= st['written'][0] <= st['buf'][0], (margins, name, st)
            assert st['computed'][1] <= st['written'][1] <= st['buf'][1], (margins, name, st)
        for consumer, producer, rows, cols in R.needs(ch):
            wr = ch[producer]['written']
            assert rows <= wr[0] and cols <= wr[1], \
                f'{consumer} reads {rows} x {cols} of {producer}, which stored {wr} (margins {margins})'


@pytest.mark.parametrize('h', [32, 128, 256])
def test_a_narrower_band_breaks_the_contract(h, monkeypatch):
    """The check above has teeth where the chain has no spare: the adjoint horizontal pass computes rows out to
    2 hd + 96, exactly the gradient's band, so 95 fails it; the forward horizontal pass computes rows out to
    hd + 32 (and reads 19 columns past the logical image), so a pad band of 31 fails it."""
    def holds():
        for margins in [(0, 0, 0, 0), (1, 0, 1, 0)]:
            ch = R.chain(h, h, margins)
            for _, producer, rows, cols in R.needs(ch):
                wr = ch[producer]['written']
                if rows > wr[0] or cols > wr[1]:
                    return False
        return True
    assert holds()
    monkeypatch.setattr(R, 'GRAD_BAND', 95)
    assert not holds()
    monkeypatch.setattr(R, 'GRAD_BAND', 96)
    monkeypatch.setattr(R, 'PAD_BAND', 31)
    assert not holds()


# ------------------------------------------------------------------ the judges of test_ada_geom_gpu.py, on CPU stand-ins
def _left(values, computed, band, shape):
    """A buffer as a kernel of the chain leaves it: NaN, zeros out to `band`, `values` inside `computed`."""
    import torch
    y = torch.full(shape, float('nan'))
    y[:, :, :band[0], :band[1]] = 0
    y[:, :, :computed[0], :computed[1]] = values[:, :, :computed[0], :computed[1]]
    return y


def test_assert_regions_sees_each_region():
    """A band one row or column short (a pad band of 63, a kZeroBand of 31), a store past the band (a run of 4
    whose tail ignores `rows`) and a wrong computed element each fail EW.assert_regions."""
    import torch
    import elementwise as EW
    ref = torch.randn(2, 1, 60, 64, generator=torch.Generator().manual_seed(0)).double()
    slack = torch.full_like(ref, 1e-6)
    c, b = (10, 12), (10 + R.FIR_BAND, 12 + R.FIR_BAND)
    assert EW.assert_regions(_left(ref, c, b, ref.shape), c, b, 'ok', ref=ref, slack=slack) < 1
    with pytest.raises(AssertionError, match='zero-band elements'):
        EW.assert_regions(_left(ref, c, (b[0] - 1, b[1]), ref.shape), c, b, 'short rows', ref=ref, slack=slack)
    with pytest.raises(AssertionError, match='zero-band elements'):
        EW.assert_regions(_left(ref, c, (b[0], b[1] - 1), ref.shape), c, b, 'short cols', ref=ref, slack=slack)
    with pytest.raises(AssertionError, match='beyond the band'):
        EW.assert_regions(_left(ref, c, (b[0] + 2, b[1]), ref.shape), c, b, 'tail of a run', ref=ref, slack=slack)
    y = _left(ref, c, b, ref.shape)
    y[1, 0, 9, 11] += 1e-3
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        EW.assert_regions(y, c, b, 'one element', ref=ref, slack=slack)
    with pytest.raises(AssertionError, match='differ'):
        EW.assert_regions(y, c, b, 'one element, bitwise', ref=ref, exact=True)


def test_pad_adjoint_bound_sees_a_dropped_term():
    """The f32 adjoint of F.pad(reflect) sits inside reflect_pad_adjoint_ref's bound; without the far-side
    reflection of the rows (the third term of the 3 x 3 gather) it does not."""
    import torch
    import torch.nn.functional as F
    import elementwise as EW
    h, w, m = 9, 11, (6, 5, 4, 7)
    gy = torch.randn(2, 2, h + m[1] + m[3], w + m[0] + m[2], generator=torch.Generator().manual_seed(1))
    ref, slack = EW.reflect_pad_adjoint_ref(gy.double(), (h, w), m)
    x = torch.zeros(2, 2, h, w, requires_grad=True)
    y = F.pad(x, (m[0], m[2], m[1], m[3]), mode='reflect')
    good, = torch.autograd.grad(y, [x], gy, retain_graph=True)
    assert EW.assert_elementwise(good, ref, slack, torch.float32, 'f32 adjoint') <= 1
    dropped = gy.clone()
    dropped[:, :, m[1] + h:] = 0
    bad, = torch.autograd.grad(y, [x], dropped)
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        EW.assert_elementwise(bad, ref, slack, torch.float32, 'dropped term')


@pytest.mark.parametrize('hw', [(20, 24), (40, 36)])
def test_grid_sample_bound_sees_swapped_weights(hw):
    """A plain f32 bilinear sample (the kernel's formulas: corners_g, four products) sits inside grid_sample_ref's
    bound, centre-snapped points included; with w01 and w10 swapped it does not."""
    import torch
    import elementwise as EW
    H, W = hw
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, H, W, generator=g)
    grid = torch.rand(2, 30, 26, 2, generator=g) * 2.6 - 1.3
    grid[1, :, :, 1] = ((2 * torch.arange(-2, 28) + 1).float() / H - 1)[:, None]      # rows on pixel centres
    grid[1, :, :, 0] = ((2 * torch.arange(-2, 24) + 1).float() / W - 1)[None]         # columns on pixel centres
    ref, slack = EW.grid_sample_ref(x.double(), grid.double())

    def sample(swap):
        one, half = torch.tensor(1.0), torch.tensor(0.5)
        ix, iy = ((grid[..., 0] + one) * W - one) * half, ((grid[..., 1] + one) * H - one) * half
        fx, fy = ix.floor(), iy.floor()
        ax, ay, bx, by = ix - fx, iy - fy, (fx + one) - ix, (fy + one) - iy
        w00, w01, w10, w11 = bx * by, ax * by, bx * ay, ax * ay
        if swap:
            w01, w10 = w10, w01
        xp = torch.nn.functional.pad(x, [1, 1, 1, 1])
        x0, y0 = fx.long().clamp(-1, W - 1) + 1, fy.long().clamp(-1, H - 1) + 1
        inside = ((fx >= -1) & (fx <= W - 1) & (fy >= -1) & (fy <= H - 1)).float()[:, None]
        n = torch.arange(2)[:, None, None]
        at = lambda yy, xx: xp[n, :, yy, xx].permute(0, 3, 1, 2)     # noqa: E731
        return inside * (at(y0, x0) * w00[:, None] + at(y0, x0 + 1) * w01[:, None] + at(y0 + 1, x0) * w10[:, None] +
                         at(y0 + 1, x0 + 1) * w11[:, None])
    ratio = EW.assert_elementwise(sample(False), ref, slack, torch.float32, 'f32 replay')
    print(f'f32 replay of the forward sampler at {H} x {W}: worst error / bound {ratio:.3g}')
    with pytest.raises(AssertionError, match='outside the elementwise bound'):
        EW.assert_elementwise(sample(True), ref, slack, torch.float32, 'swapped weights')
