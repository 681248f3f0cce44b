"""Shared inputs and float64 numpy oracle of the kernel-inception-distance tests (test_kid_metric.py,
test_poly_mmd_gpu.py) and of the fixture generator tests/golden/make_kid_golden.py.

Semantics under test (include/sg2hip.h, sg2_poly_mmd_sums): per subset s of m generated rows x_i and m real rows y_j,
with k(a, b) = (a.b / d + 1)^3,
    (Sxx, Syy, Sxy) = (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j))
    KID = mean_s[(Sxx + Syy) / (m - 1) - 2 Sxy / m] / m
The subsets are drawn from the global np.random after np.random.seed(SEED), per subset first the generated rows,
then the real rows, both without replacement (SG3/metrics/kernel_inception_distance.py:37-39).

Tolerance.  The reference computes the sums in float32 numpy.  E_REF, computed when this module is imported, is the
worst relative error of that float32 restatement (ref32) against float64 over all cases, subsets and the three sums;
the kernel's bound on every sum is REL = 16 * E_REF.  The factor 16 allows for the f32-input MFMA's strictly
sequential k-order fma chain (0.75 - 3.5e-7 sum|a b| for K from 1024 to 4096 per entry), where BLAS' blocked dot
products and numpy's pairwise sums grow more slowly; it stays about an order of magnitude below what a 16-bit operand
would give.  The worst case analysis -- the chain's d roundings, `/ d`, `+ 1` and two multiplies of the cube at three
times the relative error of its argument, a 64-term f32 partial -- is CAP = (3 (d + 2) + 68) 2^-24 per sum.
The bound on the KID follows from the sums: REL * mean_s[(Sxx + Syy) / (m - 1) + 2 Sxy / m] / m.
"""
import functools

import numpy as np

SEED = 123
LOWRANK = 8
# (n_real, n_gen, d, S, max_subset_size, spread of gen, seed of gen)
CASES = [
    (300, 260, 36, 3, 33, 1.3, 2),          # m = 33: one past a 32 x 32 fragment; K tail (36 = 32 + 4)
    (515, 389, 136, 7, 100, 1.3, 2),        # m = 100: ragged edge inside one 128 tile, K tail 136 = 4 * 32 + 8
    (515, 389, 136, 7, 100, 1.0, 2),        # the same at a smaller distance
    (300, 300, 520, 4, 130, 0.8, 2),        # m = 130: one past the 128 tile, 2 x 2 tiles
    (400, 300, 2048, 2, 257, 1.3, 2),       # the production d; m = 2 * 128 + 1, 3 x 3 tiles
    (300, 300, 136, 5, 64, 1.0, 3),         # the same distribution on both sides: KID near 0; m = a whole wave tile
]
# float64 KID of each case as measured on the CPU (documentation; test_kid_metric.py checks them within 1e-4)
KID_MEASURED = [0.3390, 0.3507, 0.0506, 0.0717, 0.2250, 0.0077]


def case_id(case):
    n_real, n_gen, d, S, msub, s, gseed = case
    return f'r{n_real}_g{n_gen}_d{d}_S{S}_m{msub}_s{int(round(s * 10)):02d}_seed{gseed}'


def subset_size(case):
    return min(min(case[0], case[1]), case[4])


def blob(seed, n, d, s, shift=0.5):
    r = np.random.RandomState(seed)
    B = np.random.RandomState(7).randn(LOWRANK, d) / np.sqrt(LOWRANK)
    x = (r.randn(n, LOWRANK) * s) @ B + 0.25 * r.randn(n, d) + shift
    return np.maximum(x, 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def features(case):
    """(real [n_real, d], gen [n_gen, d]) float32; treat as read-only."""
    n_real, n_gen, d, _, _, s, gseed = case
    real, gen = blob(1, n_real, d, 1.0), blob(gseed, n_gen, d, s)
    real.setflags(write=False)
    gen.setflags(write=False)
    return real, gen


@functools.lru_cache(maxsize=None)
def draws(case):
    """(idx_gen, idx_real) int64 [S, m]: the reference's draws.  Seeds and restores the global np.random."""
    n_real, n_gen, _, S, _, _, _ = case
    m = subset_size(case)
    state = np.random.get_state()
    try:
        np.random.seed(SEED)
        ig, ir = np.empty([S, m], dtype=np.int64), np.empty([S, m], dtype=np.int64)
        for s in range(S):
            ig[s] = np.random.choice(n_gen, m, replace=False)
            ir[s] = np.random.choice(n_real, m, replace=False)
    finally:
        np.random.set_state(state)
    ig.setflags(write=False)
    ir.setflags(write=False)
    return ig, ir


def sums64(gen, real, idx_gen, idx_real):
    """float64 [S, 3] of float32 (or any) features: the Gram entries exact to float64 rounding."""
    gen, real = np.asarray(gen, dtype=np.float64), np.asarray(real, dtype=np.float64)
    d = gen.shape[1]
    out = np.empty([len(idx_gen), 3], dtype=np.float64)
    for s, (ig, ir) in enumerate(zip(idx_gen, idx_real)):
        x, y = gen[np.asarray(ig)], real[np.asarray(ir)]
        kxx, kyy, kxy = (x @ x.T / d + 1) ** 3, (y @ y.T / d + 1) ** 3, (x @ y.T / d + 1) ** 3
        off = ~np.eye(len(ig), dtype=bool)
        out[s] = kxx[off].sum(), kyy[off].sum(), kxy.sum()
    return out


def sums32(gen, real, idx_gen, idx_real):
    """The reference's expressions in float32 numpy, per sum: `(x @ x.T / n + 1) ** 3`, `.sum() - np.diag().sum()`."""
    gen, real = np.asarray(gen, dtype=np.float32), np.asarray(real, dtype=np.float32)
    n = gen.shape[1]
    out = np.empty([len(idx_gen), 3], dtype=np.float64)
    for s, (ig, ir) in enumerate(zip(idx_gen, idx_real)):
        x, y = gen[np.asarray(ig)], real[np.asarray(ir)]
        kxx, kyy, kxy = (x @ x.T / n + 1) ** 3, (y @ y.T / n + 1) ** 3, (x @ y.T / n + 1) ** 3
        assert kxx.dtype == np.float32 and kxy.dtype == np.float32
        out[s] = kxx.sum() - np.diag(kxx).sum(), kyy.sum() - np.diag(kyy).sum(), kxy.sum()
    return out


def diag64(feats, idx):
    """float64 sum_i k(x_i, x_i) of one subset."""
    x = np.asarray(feats, dtype=np.float64)[np.asarray(idx)]
    return float((((x * x).sum(axis=1) / x.shape[1] + 1) ** 3).sum())


def kid_from_sums(sums, m):
    s = np.asarray(sums, dtype=np.float64)
    return float(np.mean((s[:, 0] + s[:, 1]) / (m - 1) - 2.0 * s[:, 2] / m) / m)


def kid_scale(sums, m):
    """The magnitude the KID's terms have before they cancel: mean_s[(Sxx + Syy) / (m - 1) + 2 Sxy / m] / m."""
    s = np.asarray(sums, dtype=np.float64)
    return float(np.mean((s[:, 0] + s[:, 1]) / (m - 1) + 2.0 * s[:, 2] / m) / m)


@functools.lru_cache(maxsize=None)
def oracle(case):
    """dict(sums [S, 3] float64, sums32 [S, 3], kid, scale, m) of one case."""
    real, gen = features(case)
    ig, ir = draws(case)
    m = subset_size(case)
    s64 = sums64(gen, real, ig, ir)
    s64.setflags(write=False)
    return dict(sums=s64, sums32=sums32(gen, real, ig, ir), kid=kid_from_sums(s64, m), scale=kid_scale(s64, m), m=m)


def checksum(feats):
    return float(np.asarray(feats, dtype=np.float64).sum())


def cap(d):
    """The worst-case relative error of one sum (module docstring)."""
    return (3 * (d + 2) + 68) * 2.0 ** -24


def _e_ref():
    worst = 0.0
    for case in CASES:
        o = oracle(case)
        worst = max(worst, float(np.max(np.abs(o['sums32'] - o['sums']) / np.abs(o['sums']))))
    return worst


E_REF = _e_ref()
REL = 16.0 * E_REF


def kid_bound(case_or_scale):
    """Absolute bound on the KID: REL times the magnitude of its terms."""
    scale = case_or_scale if isinstance(case_or_scale, float) else oracle(case_or_scale)['scale']
    return REL * scale
