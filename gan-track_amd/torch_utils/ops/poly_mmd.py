"""Polynomial-kernel MMD sums of the kernel inception distance (HIP kernel sg2_poly_mmd_sums, csrc/mmd.hip).

The reference draws, per subset, m generated and m real feature rows, builds the three m x m float32 Gram matrices
on the host (x @ x.T, y @ y.T, x @ y.T), cubes and sums them (SG3/metrics/kernel_inception_distance.py:37-43).
Here the subsets are index tables: one exact-f32 MFMA GEMM gathers the rows through them, applies
k(a, b) = (a.b / d + 1)^3 in its epilogue and reduces every Gram to one float64 number, so neither the gathered
rows nor a Gram matrix ever exist in memory.

ROCm tensors only (no CPU fallback); not differentiable.
"""
import ctypes

import numpy as np
import torch

import sg2hip as _hip


def _features(t, what):
    if t.ndim != 2:
        raise RuntimeError(f'{what} must be [n, d]; got {list(t.shape)}')
    return t.detach().to(torch.float32).contiguous()


def _table(idx, n, what):
    """int32 host table [S, m] of row numbers below n, checked: the kernel trusts it."""
    if isinstance(idx, torch.Tensor):
        idx = idx.detach().cpu().numpy()
    idx = np.asarray(idx)
    if idx.dtype.kind not in 'iu':
        raise RuntimeError(f'{what} must hold integers; got dtype {idx.dtype}')
    if idx.ndim != 2:
        raise RuntimeError(f'{what} must be [S, m]; got {list(idx.shape)}')
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise RuntimeError(f'{what} {list(idx.shape)} holds row numbers in [{int(idx.min())}, {int(idx.max())}], '
                           f'outside the {n} rows of its feature set')
    return np.ascontiguousarray(idx, dtype=np.int32)


def check_tables(idx_gen, idx_real, n_gen, n_real):
    """The two index tables as int32 host arrays of one shape [S, m], every entry a row of its feature set; a
    RuntimeError naming the shapes otherwise.  (The kernel trusts what it is given: this is the trust boundary.)"""
    ig, ir = _table(idx_gen, n_gen, 'idx_gen'), _table(idx_real, n_real, 'idx_real')
    if ig.shape != ir.shape:
        raise RuntimeError(f'subset_sums: idx_gen {list(ig.shape)} and idx_real {list(ir.shape)} must have one shape')
    return ig, ir


def subset_sums(gen, real, idx_gen, idx_real):
    """float64 [S, 3] on the features' device: per subset s, with x_i = gen[idx_gen[s, i]], y_j = real[idx_real[s, j]]
    and k(a, b) = (a.b / d + 1)^3,
        (sum_{i != j} k(x_i, x_j),  sum_{i != j} k(y_i, y_j),  sum_{i, j} k(x_i, y_j)).
    gen [n_gen, d], real [n_real, d] (made float32 and contiguous; d % 4 == 0); idx_gen, idx_real: integer arrays or
    tensors [S, m] (m >= 2), read on the host and checked there.  Two calls give the same bits."""
    _hip.require_device(gen, real)
    gen, real = _features(gen, 'gen'), _features(real, 'real')
    if gen.shape[1] != real.shape[1] or gen.device != real.device:
        raise RuntimeError(f'subset_sums: gen {list(gen.shape)} and real {list(real.shape)} do not fit together '
                           f'(one device, one d)')
    ig, ir = check_tables(idx_gen, idx_real, gen.shape[0], real.shape[0])
    (S, m), d = ig.shape, gen.shape[1]
    nbytes = ctypes.c_int64(0)
    _hip.check(_hip.lib().sg2_poly_mmd_scratch_bytes(ctypes.byref(nbytes), S, m), 'sg2_poly_mmd_scratch_bytes')
    with torch.cuda.device(gen.device):
        dg, dr = torch.from_numpy(ig).to(gen.device), torch.from_numpy(ir).to(gen.device)
        sums = torch.empty([S, 3], dtype=torch.float64, device=gen.device)
        scratch = torch.empty([(nbytes.value + 7) // 8], dtype=torch.float64, device=gen.device)
        _hip.check(_hip.lib().sg2_poly_mmd_sums(_hip.ptr(sums), _hip.ptr(gen), gen.shape[0], _hip.ptr(real),
                                                real.shape[0], _hip.ptr(dg), _hip.ptr(dr), S, m, d,
                                                _hip.ptr(scratch), scratch.numel() * 8,
                                                _hip.stream_ptr(gen.device)),
                   'sg2_poly_mmd_sums')
    return sums


def kid_from_sums(sums, m):
    """The unbiased MMD^2 estimate averaged over the subsets, in float64:
    mean_s[(Sxx + Syy) / (m - 1) - 2 Sxy / m] / m (SG3/metrics/kernel_inception_distance.py:42-43)."""
    s = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    s = s.astype(np.float64)
    return float(np.mean((s[:, 0] + s[:, 1]) / (m - 1) - 2.0 * s[:, 2] / m) / m)
