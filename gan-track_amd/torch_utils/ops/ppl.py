"""The two streaming passes of a perceptual-path-length sampler call (HIP kernels sg2_ppl_prep and
sg2_lpips_pair_dist, csrc/ppl.hip).

prep_images(img, channel, crop, factor)   the LPIPS detector's input from the generator's f32 output in one pass:
                                          centre crop, factor x factor mean, (x + 1) * 127.5, one channel repeated to 3
pair_distances(feats, eps)                dist[b] = |feats[b] - feats[B + b]|^2 / eps^2 in one read of the features

The reference composes the first from 2-4 small torch passes and the second from three passes with two temporaries
of the features' size (SG3/metrics/perceptual_path_length.py:71-89).  ROCm tensors only (no CPU fallback); neither op
is differentiable.  The `*_ref` functions are the reference's composition on any device: the SG2_PPL_FUSED=0 path of
the metric and the cross-check of the kernels.
"""
import ctypes

import torch

import sg2hip as _hip

PAIR_CHUNK = 8192           # elements per stage-1 workgroup of sg2_lpips_pair_dist
PAIR_THREADS = 256


def pair_dist_tree(F):
    """(longest serial runs added, tree depth) of sg2_lpips_pair_dist's fixed summation tree for rows of F elements
    (csrc/ppl.hip): runs of 8 squares per lane and of ceil(chunks / 256) chunk partials, depth 2 + 6 + 2 + 6 + 2."""
    chunks = -(-int(F) // PAIR_CHUNK)
    return 8 + -(-chunks // PAIR_THREADS), 18


def _plain_f32(t, what, ndim):
    _hip.require_device(t)
    if t.ndim != ndim or t.dtype != torch.float32:
        raise RuntimeError(f'{what} must be a float32 tensor with {ndim} dimensions; got {t.dtype} {list(t.shape)}')
    return t.detach().contiguous()


def prep_images(img, channel=None, crop=False, factor=1):
    """img f32 [N, C, H, W] in [-1, 1] -> f32 [N, 3, H' / factor, W' / factor] in [0, 255].  channel: the source channel
    that becomes all three output channels (None: all channels; C must then be 1 or 3).  crop: rows 3c..7c, columns
    2c..6c with c = H // 8.  factor: side of the averaging window (0 and 1: none).  At factor <= 1 the result is
    bitwise (x + 1) * (255 / 2) of torch."""
    img = _plain_f32(img, 'prep_images: img', 4)
    n, c, h, w = img.shape
    factor = max(int(factor), 1)
    c8 = h // 8
    hc, wc = (4 * c8, 4 * c8) if crop else (h, w)
    with torch.cuda.device(img.device):
        out = torch.empty([n, 3, hc // factor, wc // factor], dtype=torch.float32, device=img.device)
        _hip.check(_hip.lib().sg2_ppl_prep(_hip.ptr(out), _hip.ptr(img), n, c, h, w, -1 if channel is None else
                                           int(channel), int(bool(crop)), factor, _hip.stream_ptr(img.device)),
                   'sg2_ppl_prep')
    return out


def pair_distances(feats, eps):
    """feats f32 [2B, F] (rows 0..B-1 at t, rows B..2B-1 at t + eps) -> f32 [B]: the squared feature distance of
    every pair over eps^2.  Bitwise reproducible; a pair gives the same bits alone or in a batch."""
    feats = _plain_f32(feats, 'pair_distances: feats', 2)
    rows, f = feats.shape
    if rows < 2 or rows % 2 or f < 1:
        raise RuntimeError(f'pair_distances: feats must be [2B, F] with B, F >= 1; got {list(feats.shape)}')
    b = rows // 2
    L = _hip.lib()
    nbytes = ctypes.c_int64(0)
    _hip.check(L.sg2_lpips_pair_dist_scratch_bytes(ctypes.byref(nbytes), b, f), 'sg2_lpips_pair_dist_scratch_bytes')
    with torch.cuda.device(feats.device):
        scratch = torch.empty([(nbytes.value + 3) // 4], dtype=torch.float32, device=feats.device)
        dist = torch.empty([b], dtype=torch.float32, device=feats.device)
        _hip.check(L.sg2_lpips_pair_dist(_hip.ptr(dist), _hip.ptr(feats), b, f, float(eps), _hip.ptr(scratch),
                                         scratch.numel() * 4, _hip.stream_ptr(feats.device)), 'sg2_lpips_pair_dist')
    return dist


# ---- the reference's composition (any device) ----

def prep_images_ref(img, channel=None, crop=False, factor=1):
    """SG3/metrics/perceptual_path_length.py:71-85, with the per-modality channel selection in front."""
    if channel is not None:
        img = img[:, int(channel)].unsqueeze(1)
    if crop:
        assert img.shape[2] == img.shape[3]
        c = img.shape[2] // 8
        img = img[:, :, 3 * c:7 * c, 2 * c:6 * c]
    if factor > 1:
        n, ch, h, w = img.shape
        img = img.reshape(n, ch, h // factor, factor, w // factor, factor).mean(dim=(3, 5))
    img = (img + 1) * (255 / 2)
    return img.repeat([1, 3, 1, 1]) if img.shape[1] == 1 else img


def pair_distances_ref(feats, eps):
    """:88-89."""
    t0, t1 = feats.chunk(2)
    return (t0 - t1).square().sum(1) / eps ** 2
