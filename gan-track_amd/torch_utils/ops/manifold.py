"""k-nearest-neighbour manifolds of the improved precision / recall metric (HIP kernels sg2_knn_radii and
sg2_manifold_member, csrc/knn.hip).

The reference builds the [rows, cols] fp16 distance matrix with torch.cdist in 10 000 x 10 000 blocks, copies every
block to the host and takes `kthvalue(nhood_size + 1)` and `(dist <= kth).any(dim=1)` there
(SG3/metrics/precision_recall.py:19-61).  Here the matrix never exists: one fp16 MFMA GEMM whose epilogue keeps the
k + 1 smallest entries, or one flag, per row.  With round16 (the default) the distances are rounded to fp16 before
they are ranked or compared, which is where the reference holds them; round16=False keeps them in float32.

ROCm tensors only (no CPU fallback); neither op is differentiable.
"""
import ctypes

import torch

import sg2hip as _hip


def _features(t, what):
    if t.ndim != 2:
        raise RuntimeError(f'{what} must be [n, d]; got {list(t.shape)}')
    return t.detach().to(torch.float16).contiguous()


def _scratch(rows, cols, k, device):
    nbytes = ctypes.c_int64(0)
    _hip.check(_hip.lib().sg2_knn_scratch_bytes(ctypes.byref(nbytes), rows, cols, k), 'sg2_knn_scratch_bytes')
    return torch.empty([(nbytes.value + 3) // 4], dtype=torch.float32, device=device)


def knn_radii(x, k, round16=True):
    """float32 [n]: per row of x [n, d] the (k + 1)-th smallest distance to the rows of x, itself (distance exactly 0)
    included -- the reference's `dist.kthvalue(k + 1)` of a manifold against itself.  1 <= k <= 7, d % 8 == 0."""
    _hip.require_device(x)
    x = _features(x, 'x')
    n, d = x.shape
    with torch.cuda.device(x.device):
        radii = torch.empty([n], dtype=torch.float32, device=x.device)
        scratch = _scratch(n, n, int(k), x.device)
        _hip.check(_hip.lib().sg2_knn_radii(_hip.ptr(radii), _hip.ptr(x), _hip.F16, n, d, int(k), int(bool(round16)),
                                            _hip.ptr(scratch), scratch.numel() * 4, _hip.stream_ptr(x.device)),
                   'sg2_knn_radii')
    return radii


def manifold_member(probes, manifold, radii, round16=True):
    """bool [p]: whether probe i lies within radii[j] of any manifold row j (`(dist <= kth).any(dim=1)`).
    probes [p, d], manifold [n, d], radii [n] (knn_radii of the manifold)."""
    _hip.require_device(probes, manifold, radii)
    probes, manifold = _features(probes, 'probes'), _features(manifold, 'manifold')
    radii = radii.detach().to(torch.float32).contiguous()
    (p, d), n = probes.shape, manifold.shape[0]
    if manifold.shape[1] != d or radii.shape != (n,) or not (manifold.device == radii.device == probes.device):
        raise RuntimeError(f'manifold_member: probes {list(probes.shape)}, manifold {list(manifold.shape)} and radii '
                           f'{list(radii.shape)} do not fit together (one device, one d, one radius per manifold row)')
    with torch.cuda.device(probes.device):
        hit = torch.empty([p], dtype=torch.uint8, device=probes.device)
        scratch = _scratch(p, n, 1, probes.device)
        _hip.check(_hip.lib().sg2_manifold_member(_hip.ptr(hit), _hip.ptr(probes), p, _hip.ptr(manifold), n,
                                                  _hip.ptr(radii), _hip.F16, d, int(bool(round16)), _hip.ptr(scratch),
                                                  scratch.numel() * 4, _hip.stream_ptr(probes.device)),
                   'sg2_manifold_member')
    return hit.bool()


def manifold_count(probes, manifold, radii, round16=True):
    """(count int32 [p], covered bool [n]) of one pass over the p x n distances (HIP kernel sg2_manifold_count):
    count[i] = the number of manifold rows j with dist(probe_i, manifold_j) <= radii[j], covered[j] = whether any probe
    lies within radii[j] of manifold row j.  The balls, the distances and the `<=` are manifold_member's, so
    `count > 0` equals manifold_member(...) bit for bit; density = count.sum() / (k p), coverage = covered.mean()
    (Naeem et al. 2020).  probes [p, d], manifold [n, d], radii [n] (knn_radii of the manifold)."""
    _hip.require_device(probes, manifold, radii)
    probes, manifold = _features(probes, 'probes'), _features(manifold, 'manifold')
    radii = radii.detach().to(torch.float32).contiguous()
    (p, d), n = probes.shape, manifold.shape[0]
    if manifold.shape[1] != d or radii.shape != (n,) or not (manifold.device == radii.device == probes.device):
        raise RuntimeError(f'manifold_count: probes {list(probes.shape)}, manifold {list(manifold.shape)} and radii '
                           f'{list(radii.shape)} do not fit together (one device, one d, one radius per manifold row)')
    with torch.cuda.device(probes.device):
        count = torch.empty([p], dtype=torch.int32, device=probes.device)
        covered = torch.empty([n], dtype=torch.uint8, device=probes.device)
        nbytes = ctypes.c_int64(0)
        _hip.check(_hip.lib().sg2_manifold_count_scratch_bytes(ctypes.byref(nbytes), p, n),
                   'sg2_manifold_count_scratch_bytes')
        scratch = torch.empty([(nbytes.value + 3) // 4], dtype=torch.float32, device=probes.device)
        _hip.check(_hip.lib().sg2_manifold_count(_hip.ptr(count), _hip.ptr(covered), _hip.ptr(probes), p,
                                                 _hip.ptr(manifold), n, _hip.ptr(radii), _hip.F16, d,
                                                 int(bool(round16)), _hip.ptr(scratch), scratch.numel() * 4,
                                                 _hip.stream_ptr(probes.device)), 'sg2_manifold_count')
    return count, covered.bool()
