"""Float64 numpy oracle of the density / coverage tests (test_prdc_host.py, test_prdc_gpu.py): the published
definition (Naeem et al., ICML 2020) restated on pr_oracle's inputs, distances and tolerance.

Semantics under test (include/sg2hip.h, sg2_manifold_count): with dist and round16 as in pr_oracle and r the fp16
k-NN radii of the real set (pr_oracle.radii16: the k-th neighbour, the point itself excluded),

    M[i, j]    = fp16(dist(gen_i, real_j)) <= r[j]
    count[i]   = sum_j M[i, j]        covered[j] = any_i M[i, j]
    density    = sum(count) / (k p)   coverage   = sum(covered) / n        precision = #{count > 0} / p

A distance within TAU of an fp16 rounding boundary may round either way (pr_oracle), so M is evaluated with the
distances scaled by (1 + eps): eps = -TAU is the lenient matrix, +TAU the strict one.  Scaling and rounding are
monotone, so M_strict <= M <= M_lenient elementwise and every count, flag and ratio of the kernels must lie between
the two evaluations; where they agree the element is decidable and must be reproduced exactly.  The `fed` variants
take the oracle's radii as given (only the probe distances are uncertain); the end-to-end ones widen the radii too
(radii_hi with the lenient matrix, radii_lo with the strict one), as pr_oracle.oracle does.
"""
import functools
import types

import numpy as np

import pr_oracle
from pr_oracle import TAU

K = 5           # the paper's neighbourhood


def pairs(D_gr, radii, eps=0.0):
    """bool [p, n]: fp16(D_gr (1 + eps)) <= radii[None, :]."""
    return (D_gr * (1.0 + eps)).astype(np.float16) <= np.asarray(radii)[None, :]


def count(M):
    return M.sum(axis=1).astype(np.int32)


def covered(M):
    return M.any(axis=0)


def evaluate(D_gr, radii, k, radii_lenient=None, radii_strict=None):
    """The exact, lenient and strict evaluations of one probe set against one manifold, with the ratios."""
    radii_lenient = radii if radii_lenient is None else radii_lenient
    radii_strict = radii if radii_strict is None else radii_strict
    o = types.SimpleNamespace(k=k, p=D_gr.shape[0], n=D_gr.shape[1], radii=radii)
    for name, r, eps in (('', radii, 0.0), ('_lenient', radii_lenient, -TAU), ('_strict', radii_strict, +TAU)):
        M = pairs(D_gr, r, eps)
        c, f = count(M), covered(M)
        setattr(o, 'count' + name, c)
        setattr(o, 'covered' + name, f)
        setattr(o, 'density' + name, int(c.sum()) / (k * o.p))
        setattr(o, 'coverage' + name, int(f.sum()) / o.n)
        setattr(o, 'precision' + name, int((c > 0).sum()) / o.p)
    assert (o.count_strict <= o.count).all() and (o.count <= o.count_lenient).all()
    assert (o.covered_strict <= o.covered).all() and (o.covered <= o.covered_lenient).all()
    o.undecidable_probes = float((o.count_lenient != o.count_strict).mean())
    o.undecidable_reals = float((o.covered_lenient != o.covered_strict).mean())
    return o


@functools.lru_cache(maxsize=None)
def fed(case, k=K):
    """Generated probes against the real manifold, the oracle's radii fed in."""
    D_rr, _, D_gr = pr_oracle.distances(case)
    return evaluate(D_gr, pr_oracle.radii16(D_rr, k), k)


@functools.lru_cache(maxsize=None)
def end_to_end(case, k=K):
    """The same with the radii uncertain too, plus the recall side (real probes against the generated manifold)."""
    D_rr, D_gg, D_gr = pr_oracle.distances(case)
    o = evaluate(D_gr, pr_oracle.radii16(D_rr, k), k, pr_oracle.radii16(D_rr, k, +TAU), pr_oracle.radii16(D_rr, k, -TAU))
    o.recall = float(pr_oracle.member16(D_gr.T, pr_oracle.radii16(D_gg, k)).mean())
    o.recall_lenient = float(pr_oracle.member16(D_gr.T, pr_oracle.radii16(D_gg, k, +TAU), -TAU).mean())
    o.recall_strict = float(pr_oracle.member16(D_gr.T, pr_oracle.radii16(D_gg, k, -TAU), +TAU).mean())
    return o


def judge(got_count, got_covered, o, probe_cap=0.02, real_cap=0.01):
    """The verdict on one (count, covered) pair against an evaluation `o`: shapes and dtypes, strict <= got <= lenient
    on every probe and every real, equality (with the exact evaluation) wherever the two coincide, and at most
    probe_cap / real_cap of the elements outside that comparison."""
    got_count, got_covered = np.asarray(got_count), np.asarray(got_covered)
    assert got_count.dtype == np.int32 and got_count.shape == (o.p,), (got_count.dtype, got_count.shape)
    assert got_covered.dtype == np.bool_ and got_covered.shape == (o.n,), (got_covered.dtype, got_covered.shape)
    assert o.undecidable_probes <= probe_cap and o.undecidable_reals <= real_cap, \
        (o.undecidable_probes, o.undecidable_reals)
    low, high = got_count < o.count_strict, got_count > o.count_lenient
    assert not low.any() and not high.any(), \
        f'{int(low.sum())} counts below the strict and {int(high.sum())} above the lenient evaluation'
    decidable = o.count_strict == o.count_lenient
    assert np.array_equal(got_count[decidable], o.count[decidable])
    assert not (got_covered < o.covered_strict).any(), 'a real that is covered for certain is not flagged'
    assert not (got_covered > o.covered_lenient).any(), 'a real that no probe can reach is flagged'
    decidable = o.covered_strict == o.covered_lenient
    assert np.array_equal(got_covered[decidable], o.covered[decidable])


# ---- the planted-padding fixture ----
# A probe panel is padded to whole 256-row tiles, and a padded row reads as zeros.  If such a row took part, its
# distance to manifold row j would be |x_j|: it would cover every real feature with |x_j| <= r_j.  The fixture plants
# two such features (j0: all zeros, j1: a single 0.5; radius 1.0 both) among blob rows; every genuine probe is a blob
# row whose norm is well above 1, so neither may be covered or counted -- unless a zero row is a genuine probe (the
# mirrored case: the last probe is all zeros and must count and cover both).
PAD_P, PAD_N, PAD_D = 260, 300, 40
PAD_J0, PAD_J1 = 7, 299


@functools.lru_cache(maxsize=None)
def padding_fixture(mirrored=False, p=PAD_P, k=K):
    """(probes fp16 [p, 40], manifold fp16 [300, 40], radii fp16 [300], evaluation)."""
    mani = pr_oracle.blob(1, PAD_N, PAD_D, 1.0).copy()
    mani[PAD_J0] = 0
    mani[PAD_J1] = 0
    mani[PAD_J1, 3] = 0.5
    probes = pr_oracle.blob(2, p, PAD_D, 1.3).copy()
    assert np.sqrt((probes.astype(np.float64) ** 2).sum(1)).min() > 1.5
    if mirrored:
        probes[p - 1] = 0
    radii = pr_oracle.radii16(pr_oracle.dist64(mani, mani), k).copy()
    radii[PAD_J0] = radii[PAD_J1] = 1.0
    o = evaluate(pr_oracle.dist64(probes, mani), radii, k)
    planted = [PAD_J0, PAD_J1]
    if mirrored:
        assert o.covered_strict[planted].all() and pairs(pr_oracle.dist64(probes[-1:], mani), radii, TAU)[0, planted].all()
    else:
        assert not o.covered_lenient[planted].any()
    return probes, mani, radii, o
