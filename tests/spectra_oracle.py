"""Shared inputs, long-double oracle and error bound of the power-spectrum tests (test_power_spectrum_gpu.py,
test_spectra_host.py).

Semantics under test (include/sg2hip.h, sg2_power_spectrum_sum):
    F_b[c, u, v] = sum_{y, x} ((x[b, c, y, x] - mean[c]) / std[c]) w[y] w[x] exp(-2 pi i (u y + v x) / S)
    out[c, u, v] = sum_b |F_b[c, u, v]|^2,     S = N * interp
The oracle evaluates exactly this in numpy.longdouble with direct DFT matrices (angles reduced as (u y) mod S in
integers, so the long-double sin / cos see arguments below 2 pi).

Tolerance.  DELTA_REF(case) is measured when this module is imported, never hard-coded: the worst |F_f64 - F_longdouble|
over every image, channel and bin of the reference's own float64 composition (whiten, window, pad, torch.fft.fftn on
the CPU: power_spectrum.spectrum_ref).  The kernel may err by delta = 16 * DELTA_REF(case) in F -- the margin
kid_oracle.REL uses; it covers a direct sum of length N against the FFT's log2 S stages -- which bounds every element
of out by
    bound[c, u, v] = sum_b (2 sqrt(P_b[c, u, v]) delta + delta^2),     P_b = |F_b|^2 of the oracle.
"""
import functools

import numpy as np
import torch

from torch_utils.ops import power_spectrum

BETA = 8.0
MARGIN = 16.0
# (N, interp, B, C, dtype)
CASES = [
    (8, 4, 1, 1, 'uint8'),          # the smallest accepted size: one 16 x 16 MFMA tile of T, K = 2 steps
    (16, 4, 1, 1, 'uint8'),         # S = 64: one tile per side of the row pass's operand
    (20, 3, 2, 2, 'uint8'),         # S = 60: tile and K tails, S not a power of two
    (20, 1, 1, 1, 'uint8'),         # S = N: no padding
    (48, 2, 5, 3, 'uint8'),         # several tiles, odd batch
    (64, 4, 4, 1, 'uint8'),         # S = 256: many workgroups, the batch split into groups
    (36, 4, 1, 1, 'float32'),       # the float path
    # the column pass's loop over the images of one batch group (the cases above all run one image per group: the
    # plan gives a group per image while B <= 16 and the grid is small), and the row pass's second block of rows
    (8, 4, 17, 1, 'uint8'),         # 9 groups of 2 images, the last one short (1 image)
    (8, 4, 33, 2, 'uint8'),         # 11 groups of 3 images, two channels
    (72, 1, 2, 1, 'uint8'),         # N > 64: two blocks of rows in the row pass, the second one 8 rows; S = 72 tails
    (128, 2, 3, 1, 'uint8'),        # N = 128: two whole blocks of rows, four K-loops of 8 steps; S = 256
]
# (B, C, N, interp) -> (groups, images per group) of the kernel's plan for the cases that are about it; pinned
# against the scratch size the library reports in test_spectra_host.py
GROUPS = {(8, 4, 17, 1): (9, 2), (8, 4, 33, 2): (11, 3), (64, 4, 4, 1): (4, 1), (128, 2, 3, 1): (3, 1)}


def case_id(case):
    N, interp, B, C, dtype = case
    return f'N{N}_i{interp}_B{B}_C{C}_{dtype}'


def moments(C):
    """(mean [C], std [C]) float64: the reference's FFHQ numbers, shifted per channel so that channels differ."""
    c = np.arange(C, dtype=np.float64)
    return 112.684 + 7.25 * c, 69.509 - 11.5 * c


@functools.lru_cache(maxsize=None)
def images(case):
    """numpy [B, C, N, N] of the case's dtype, seeded; treat as read-only."""
    N, interp, B, C, dtype = case
    r = np.random.RandomState(1000 + 13 * N + interp)
    if dtype == 'uint8':
        x = r.randint(0, 256, size=[B, C, N, N]).astype(np.uint8)
    else:
        x = (r.rand(B, C, N, N) * 255).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def window(N):
    w = power_spectrum.kaiser_window(N, BETA).numpy()
    w.setflags(write=False)
    return w


def dft_matrix(S, N):
    """longdouble (cos, -sin) [S, N] of 2 pi ((u y) mod S) / S."""
    k = (np.arange(S)[:, None] * np.arange(N)[None, :]) % S
    ang = k.astype(np.longdouble) * (2 * np.longdouble('3.14159265358979323846264338327950288') / np.longdouble(S))
    return np.cos(ang), -np.sin(ang)


def spectrum_ld(x, mean, std, w, interp):
    """(Fr, Fi) longdouble [B, C, S, S] of any image array: the definition, term by term."""
    x = np.asarray(x)
    B, C, N, _ = x.shape
    S = N * interp
    ld = np.longdouble
    xw = (x.astype(ld) - np.asarray(mean, dtype=ld).reshape(1, C, 1, 1)) / np.asarray(std, dtype=ld).reshape(1, C, 1, 1)
    w = np.asarray(w, dtype=ld)
    xw = xw * (w[:, None] * w[None, :])
    er, ei = dft_matrix(S, N)
    # T[.., y, v] = sum_x Xw[y, x] E[v, x];  F[.., u, v] = sum_y E[u, y] T[y, v]
    tr, ti = xw @ er.T, xw @ ei.T
    fr = er @ tr - ei @ ti
    fi = er @ ti + ei @ tr
    return fr, fi


def gemm_dft_f64(x, mean, std, w, interp):
    """float64 [C, S, S]: the kernel's formulation in float64 numpy -- the two GEMMs with twiddles taken from the
    op's table of S values, the columns past S / 2 mirrored."""
    x = np.asarray(x)
    B, C, N, _ = x.shape
    S = N * interp
    tw = power_spectrum.twiddle_table(S)
    k = (np.arange(S)[:, None] * np.arange(N)[None, :]) % S
    er, ei = tw[k, 0], tw[k, 1]
    w = np.asarray(w, dtype=np.float64)
    xw = ((x.astype(np.float64) - np.asarray(mean).reshape(1, C, 1, 1)) / np.asarray(std).reshape(1, C, 1, 1)) \
        * (w[:, None] * w[None, :])
    vh = S // 2 + 1
    tr, ti = xw @ er[:vh].T, xw @ ei[:vh].T
    fr = er @ tr - ei @ ti
    fi = er @ ti + ei @ tr
    half = (fr * fr + fi * fi).sum(axis=0)                          # [C, S, vh]
    out = np.empty([C, S, S], dtype=np.float64)
    out[:, :, :vh] = half
    u = (S - np.arange(S)) % S
    out[:, :, vh:] = half[:, u][:, :, S - np.arange(vh, S)]
    return out


@functools.lru_cache(maxsize=None)
def oracle(case):
    """dict(power [C, S, S] float64 (rounded from power_ld, the long double), per_image [B, C, S, S] float64 P_b,
    delta_ref, bound [C, S, S]) of one case; arrays are read-only."""
    N, interp, B, C, dtype = case
    x = images(case)
    mean, std = moments(C)
    w = window(N)
    fr, fi = spectrum_ld(x, mean, std, w, interp)
    f_ref = power_spectrum.spectrum_ref(torch.from_numpy(np.array(x)), mean, std, torch.from_numpy(np.array(w)),
                                        interp).numpy()
    err = np.hypot(f_ref.real.astype(np.longdouble) - fr, f_ref.imag.astype(np.longdouble) - fi)
    delta_ref = float(err.max())
    p_b = fr * fr + fi * fi
    delta = MARGIN * delta_ref
    bound = (2 * np.sqrt(p_b) * delta + delta * delta).sum(axis=0).astype(np.float64)
    power = p_b.sum(axis=0).astype(np.float64)
    per_image = p_b.astype(np.float64)
    for a in (bound, power, per_image):
        a.setflags(write=False)
    return dict(power=power, power_ld=p_b.sum(axis=0), per_image=per_image, delta_ref=delta_ref, bound=bound,
                power_ref=(f_ref.real ** 2 + f_ref.imag ** 2).sum(axis=0))


def DELTA_REF(case):
    return oracle(case)['delta_ref']


def bound_of(per_image, delta_ref):
    """The bound for any stack of per-image powers [B, ...] at a given DELTA_REF."""
    delta = MARGIN * delta_ref
    return (2 * np.sqrt(np.asarray(per_image, dtype=np.float64)) * delta + delta * delta).sum(axis=0)


def share(got, case):
    """The worst |got - power| / bound over every element of out (no element left out)."""
    o = oracle(case)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == o['power'].shape, (got.shape, o['power'].shape)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got.astype(np.longdouble) - o['power_ld']) / o['bound']))


for _case in CASES:     # measured at import
    oracle(_case)
