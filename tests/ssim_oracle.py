"""Float64 numpy restatement of SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) and MSE, the seeded fixtures of the SSIM
tests, and the bounds those tests hold every implementation to (test infrastructure; a plain module).

    window:  w = g g^T, g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)), k = 0..10, normalised to sum 1; valid positions only
    moments: mx = sum w x, sxx = sum w x^2 - mx^2, sxy = sum w x y - mx my      (population form)
    ssim = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),  C1 = (0.01 L)^2, C2 = (0.03 L)^2

ssim_mse_direct sums the 121 taps of w one after another, ssim_mse_separable filters rows, then columns, with the 11
weights; `moments` takes the dtype, so the float32 restatement the host test plants is the same code.

The bounds are derived, not measured.  Every implementation under test keeps float64 moments, so two of them differ
only in summation order, in whether a multiply-add is fused and in the rounding of w against g g^T.  With
u = 2^-53 and pixels in [0, L] (every term of every moment is >= 0, so a sum of T terms carries a relative error of at
most (T + 1) u whatever its order; T = 121 taps is the longest chain, + 3 for the rounding of the weights and products):

  * a raw moment E[.] <= L^2 is off by at most (TAPS + 4) u L^2; mx my by no more; so sxx, syy and sxy are each off
    by at most 3 (TAPS + 4) u L^2 in ABSOLUTE terms -- the subtraction cancels, the error does not;
  * the structure factor (2 sxy + C2) / (sxx + syy + C2) has a denominator >= C2 and magnitude <= 1: its error is at
    most (2 + 2) 3 (TAPS + 4) u L^2 / C2, and L^2 / C2 = 1 / 0.03^2 = 1111 whatever L is;
  * the luminance factor is a ratio of sums of non-negative terms, accurate to a relative ~4 (TAPS + 4) u = 6e-14, and
    <= 1; the final products and the division add 4 u;
  * two implementations may err in opposite directions: twice the above;
  * the mean over the positions adds the summation error of values in [-1, 1]: the kernel's tree is 2 serial terms,
    8 levels in the tile, at most 8 serial tiles and 8 levels in the finalize (26 roundings on a path), numpy's
    pairwise sum about as many: 64 u covers both.

    SSIM_TOL = 2 (12 (TAPS + 4) u / 0.03^2 + 4 (TAPS + 4) u + 4 u) + 64 u = 3.7e-10   (<= 1e-9)

A float32 restatement of the moments replaces u by 2^-24 in the first line and lands at 5e-8 .. 1.5e-5 on the fixtures
(test_ssim_host.py measures it): the bound separates the two by two orders of magnitude.  The f32 map adds half an ulp
of a value <= 1: MAP_TOL = SSIM_TOL + 2^-24.

MSE: (x - y) is exact in float64 for float32 inputs, each square is rounded once, all terms are >= 0; the kernel's path
from a pixel to the result has at most 5 + 8 + 8 + 8 additions and a division, numpy's pairwise sum 16 + 3 + 13 at
1024^2, torch's sum no more than either.  MSE_REL = 256 u = 2.8e-14 covers any two of them with room for a fused
multiply-add on one side.  Sums of integers below 2^53 are exact in any order: the integer pair is compared bitwise.
"""
import functools

import numpy as np

TAPS = 11
SIGMA = 1.5
U = 2.0 ** -53
SSIM_TOL = 2 * (12 * (TAPS * TAPS + 4) * U / 0.03 ** 2 + 4 * (TAPS * TAPS + 4) * U + 4 * U) + 64 * U
MAP_TOL = SSIM_TOL + 2.0 ** -24
MSE_REL = 256 * U
assert SSIM_TOL <= 1e-9


def gaussian_window():
    k = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    g = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def moments(x, y, form='separable', dtype=np.float64):
    """The five windowed moments (E x, E y, E x^2, E y^2, E x y) of [..., H, W] arrays at the valid positions, every
    product and sum in `dtype`.  form: 'separable' (rows, then columns, 11 taps each) or 'direct' (121 taps)."""
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    g = gaussian_window().astype(dtype)
    H, W = x.shape[-2:]
    oh, ow = H - TAPS + 1, W - TAPS + 1
    out = []
    for m in (x, y, x * x, y * y, x * y):
        if form == 'separable':
            rows = np.zeros(m.shape[:-1] + (ow,), dtype=dtype)
            for k in range(TAPS):
                rows += g[k] * m[..., :, k:k + ow]
            acc = np.zeros(m.shape[:-2] + (oh, ow), dtype=dtype)
            for k in range(TAPS):
                acc += g[k] * rows[..., k:k + oh, :]
        else:
            assert form == 'direct', form
            acc = np.zeros(m.shape[:-2] + (oh, ow), dtype=dtype)
            for i in range(TAPS):
                for j in range(TAPS):
                    acc += (g[i] * g[j]) * m[..., i:i + oh, j:j + ow]
        out.append(acc)
    return out


def ssim_map(x, y, data_range=255.0, form='separable', dtype=np.float64):
    """float64 [..., H - 10, W - 10]; with dtype=float32 the moments (only) are kept in float32."""
    ex, ey, exx, eyy, exy = moments(x, y, form, dtype)
    mxx, myy, mxy = ex * ex, ey * ey, ex * ey
    sxx, syy, sxy = [a.astype(np.float64) for a in (exx - mxx, eyy - myy, exy - mxy)]
    mxx, myy, mxy = [a.astype(np.float64) for a in (mxx, myy, mxy)]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2.0 * mxy + c1) * (2.0 * sxy + c2)) / ((mxx + myy + c1) * (sxx + syy + c2))


def mse(x, y):
    d = np.asarray(x).astype(np.float64) - np.asarray(y).astype(np.float64)
    return (d * d).mean(axis=(-2, -1))


def ssim_mse(x, y, data_range=255.0, form='separable', dtype=np.float64):
    """(out float64 [..., 2] = (mean SSIM, MSE), map float64 [..., H - 10, W - 10]) of [..., H, W] arrays."""
    smap = ssim_map(x, y, data_range, form, dtype)
    return np.stack([smap.mean(axis=(-2, -1)), mse(x, y)], axis=-1), smap


# ---- fixtures: float32 arrays, seeded, cached and read-only ----

def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _box(a, r=2):
    """(2r + 1)^2 box blur with edge replication."""
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode='edge')
    H, W = a.shape[-2:]
    return sum(p[..., i:i + H, j:j + W] for i in range(2 * r + 1) for j in range(2 * r + 1)) / (2 * r + 1) ** 2


@functools.lru_cache(maxsize=None)
def smooth_pair(shape, seed=0):
    """x: a box-blurred uniform field scaled to [0, 255], distinct per (n, c); y = clip(x + 8 randn)."""
    rs = np.random.RandomState(seed)
    f = _box(rs.rand(*shape))
    lo, hi = f.min(axis=(-2, -1), keepdims=True), f.max(axis=(-2, -1), keepdims=True)
    x = (255.0 * (f - lo) / np.maximum(hi - lo, 1e-12)).astype(np.float32)
    y = np.clip(x + 8.0 * rs.randn(*shape), 0, 255).astype(np.float32)
    return _freeze(x, y)


@functools.lru_cache(maxsize=None)
def flat_pair(shape=(1, 1, 64, 64), seed=1):
    """Flat 200 with sparse +-1 pixels (one in 16): sxx is ~0.1 beside E x^2 = 40000."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        spikes = (rs.rand(*shape) < 1 / 16) * rs.choice([-1.0, 1.0], size=shape)
        out.append((200.0 + spikes).astype(np.float32))
    return _freeze(*out)


@functools.lru_cache(maxsize=None)
def integer_pair(shape=(2, 2, 45, 77), seed=2):
    rs = np.random.RandomState(seed)
    return _freeze(rs.randint(0, 256, size=shape).astype(np.float32), rs.randint(0, 256, size=shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def unit_pair(shape=(2, 1, 40, 53), seed=3):
    """A pair in [0, 1] for data_range = 1."""
    x, y = smooth_pair(shape, seed)
    return _freeze((x / np.float32(255)).astype(np.float32), (y / np.float32(255)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(name, shape, data_range=255.0):
    """The oracle's (out, map) of a named fixture, computed once and shared."""
    x, y = {'smooth': smooth_pair, 'flat': flat_pair, 'integer': integer_pair, 'unit': unit_pair}[name](shape)
    return _freeze(*ssim_mse(x, y, data_range))
