"""Shared inputs and float64 numpy oracle of the precision / recall tests (test_pr_metric.py, test_manifold_gpu.py)
and of the fixture generator tests/golden/make_pr_golden.py.

Semantics under test (include/sg2hip.h, sg2_knn_radii / sg2_manifold_member): dist = sqrt(max(|a|^2 + |b|^2 - 2 a.b,
0)) of the fp16 inputs, the diagonal of a manifold against itself exactly 0; with round16 the distance is rounded to
fp16 before it is ranked (the (k + 1)-th smallest per row) or compared (`<=` against the column's radius, any).

The only inexact step of the kernels is d2 in f32: its error is at most about d 2^-24 (|a|^2 + |b|^2 + 2 |a.b|), for
these inputs (d2 comparable to the norms) below 2^-16 relative on dist at d = 136.  TAU = 2^-14 on dist is a 4 x
margin over that.  A distance within TAU of an fp16 rounding boundary may round either way, so every rounded quantity
is evaluated twice, with the distances scaled by (1 + eps) for eps = -TAU, +TAU: where the two runs agree the element
is decidable and the kernels must reproduce it bit for bit.
"""
import functools

import numpy as np

TAU = 2.0 ** -14
K = 3
SHAPES = [(300, 260, 40), (515, 389, 72), (1000, 900, 136)]     # (n real, m generated, d)
SPREADS = [0.8, 1.3]
CASES = [(n, m, d, s) for (n, m, d) in SHAPES for s in SPREADS]
SMALL = (515, 389, 72, 1.3)


def case_id(case):
    n, m, d, s = case
    return f'n{n}_m{m}_d{d}_s{int(round(s * 10)):02d}'


def shape_id(case):
    n, m, d, _ = case
    return f'n{n}_m{m}_d{d}'


def blob(seed, n, d, s, lowrank=8):
    r = np.random.RandomState(seed)
    B = np.random.RandomState(7).randn(lowrank, d) / np.sqrt(lowrank)
    x = (r.randn(n, lowrank) * s) @ B + 0.25 * r.randn(n, d) + 0.5
    return np.maximum(x, 0).astype(np.float16)


@functools.lru_cache(maxsize=None)
def features(case):
    n, m, d, s = case
    return blob(1, n, d, 1.0), blob(2, m, d, s)


def dist64(a, b):
    """float64 distances of fp16 rows: sqrt(sum((a - b)^2)), the differences exact, identical rows exactly 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty([a.shape[0], b.shape[0]], dtype=np.float64)
    for i in range(0, a.shape[0], 32):
        diff = a[i:i + 32, None, :] - b[None, :, :]
        out[i:i + 32] = np.einsum('ijk,ijk->ij', diff, diff)
    return np.sqrt(out)


def kth_smallest(D, k):
    """(k + 1)-th smallest per row (torch's kthvalue(k + 1))."""
    return np.partition(D, k, axis=1)[:, k]


def radii16(D_self, k, eps=0.0):
    """fp16 radii of a manifold from its float64 self-distances scaled by (1 + eps)."""
    return kth_smallest((D_self * (1.0 + eps)).astype(np.float16), k)


def member16(D_pm, radii, eps=0.0):
    """bool [p]: any_j fp16(dist(probe, manifold_j) (1 + eps)) <= radii[j]."""
    return ((D_pm * (1.0 + eps)).astype(np.float16) <= np.asarray(radii)[None, :]).any(axis=1)


@functools.lru_cache(maxsize=None)
def distances(case):
    """(D_rr, D_gg, D_gr) in float64; D_gr is [m generated, n real]."""
    real, gen = features(case)
    return dist64(real, real), dist64(gen, gen), dist64(gen, real)


@functools.lru_cache(maxsize=None)
def oracle(case, k=K):
    """The reference's numbers for one case, restated: fp16 radii of both manifolds, both prediction vectors,
    precision and recall (float32 means, as torch takes them), plus the lenient / strict evaluations."""
    D_rr, D_gg, D_gr = distances(case)
    o = {}
    for name, D_self, D_pm in (('real', D_rr, D_gr), ('gen', D_gg, D_gr.T)):
        o[f'radii_{name}'] = radii16(D_self, k)
        o[f'radii_{name}_lo'] = radii16(D_self, k, -TAU)
        o[f'radii_{name}_hi'] = radii16(D_self, k, +TAU)
        # probes against this manifold: generated probes for the real manifold (precision), real for gen (recall)
        o[f'pred_{name}'] = member16(D_pm, o[f'radii_{name}'])
        # the oracle's radii fed in: only the probe distances are uncertain
        o[f'pred_{name}_fed_lenient'] = member16(D_pm, o[f'radii_{name}'], -TAU)
        o[f'pred_{name}_fed_strict'] = member16(D_pm, o[f'radii_{name}'], +TAU)
        # end to end: the radii come from the kernels too
        o[f'pred_{name}_lenient'] = member16(D_pm, o[f'radii_{name}_hi'], -TAU)
        o[f'pred_{name}_strict'] = member16(D_pm, o[f'radii_{name}_lo'], +TAU)
    o['precision'] = float(o['pred_real'].astype(np.float32).mean())
    o['recall'] = float(o['pred_gen'].astype(np.float32).mean())
    return o
