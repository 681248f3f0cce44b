"""The per-sample loss of a batched latent projection step (HIP kernels of csrc/proj_loss.hip).

prep(synth, target)       (det_in [M B, 3, Hd, Hd], pix [B, M]): the detector's input (x + 1) * 127.5 split into the
                          modalities' three-channel images (row m B + b; above 256^2 the f x f mean), and the
                          per-sample, per-modality mean squared pixel error at full resolution.  2 + 1 launches.
sqdist_rows(f, tf)        dist [R] = sum_j (f[r][j] - tf[r][j])^2, two row pointers.  2 + 1 launches.

The reference composes these per projection from a dozen elementwise and reduction launches per modality, with one
scalar per reduction (SG3/genlib/projector/projector.py:248-257); here every sample of a batch keeps its own sums, on
fixed trees without atomics: a sample gives the same bits alone or in a batch.  Both ops are first-order autograd
Functions (target and tf take no gradient) and take ROCm tensors only.  The `*_ref` functions are the torch
composition with the per-sample reductions written out, on any device: the SG2_PROJ_FUSED=0 path of the projector and
the cross-check of the kernels.
"""
import ctypes

import torch
import torch.nn.functional as F

import sg2hip as _hip

from torch_utils.ops.ppl import pair_dist_tree as sqdist_tree       # (serial runs, depth) of sqdist_rows' tree


def num_modalities(channels):
    """projector.split_modalities' rule: 1 channel or 3 (RGB) are one modality, any other count one per channel."""
    return 1 if channels in (1, 3) else int(channels)


def det_side(h):
    """The detector's input side and the pooling factor: 256 and H / 256 above 256^2, else H and 1."""
    f = h // 256 if h > 256 else 1
    return h // f, f


def _check_images(synth, target):
    _hip.require_device(synth, target)
    if synth.ndim != 4 or synth.shape != target.shape or synth.dtype != torch.float32 or target.dtype != torch.float32:
        raise RuntimeError(f'proj_loss.prep: synth and target must be float32 [B, C, H, W] of one shape; got '
                           f'{synth.dtype} {list(synth.shape)} and {target.dtype} {list(target.shape)}')
    b, c, h, w = synth.shape
    if h != w or h < 4 or h > 1024 or h & (h - 1):
        raise RuntimeError(f'proj_loss.prep: H = W must be a power of two in 4..1024; got {h} x {w}')


class _Prep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, synth, target):
        _check_images(synth, target)
        synth, target = synth.contiguous(), target.detach().contiguous()
        b, c, h, _ = synth.shape
        m, (hd, _) = num_modalities(c), det_side(h)
        L = _hip.lib()
        nbytes = ctypes.c_int64(0)
        _hip.check(L.sg2_proj_prep_scratch_bytes(ctypes.byref(nbytes), b, c, h), 'sg2_proj_prep_scratch_bytes')
        with torch.cuda.device(synth.device):
            scratch = torch.empty([nbytes.value // 4], dtype=torch.float32, device=synth.device)
            det_in = torch.empty([m * b, 3, hd, hd], dtype=torch.float32, device=synth.device)
            pix = torch.empty([b, m], dtype=torch.float32, device=synth.device)
            _hip.check(L.sg2_proj_prep_fwd(_hip.ptr(det_in), _hip.ptr(pix), _hip.ptr(synth), _hip.ptr(target), b, c, h,
                                           _hip.ptr(scratch), scratch.numel() * 4, _hip.stream_ptr(synth.device)),
                       'sg2_proj_prep_fwd')
        ctx.save_for_backward(synth, target)
        return det_in, pix

    @staticmethod
    def backward(ctx, gdet_in, gpix):
        if torch.is_grad_enabled():
            raise RuntimeError('proj_loss.prep is first order only: its backward cannot be differentiated '
                               '(create_graph=True)')
        synth, target = ctx.saved_tensors
        b, c, h, _ = synth.shape
        gdet_in, gpix = gdet_in.to(torch.float32).contiguous(), gpix.to(torch.float32).contiguous()
        with torch.cuda.device(synth.device):
            gsynth = torch.empty_like(synth)
            _hip.check(_hip.lib().sg2_proj_prep_bwd(_hip.ptr(gsynth), _hip.ptr(gdet_in), _hip.ptr(gpix), _hip.ptr(synth),
                                                    _hip.ptr(target), b, c, h, _hip.stream_ptr(synth.device)),
                       'sg2_proj_prep_bwd')
        return gsynth, None


def prep(synth, target):
    """synth f32 [B, C, H, H] (the generator's output, [-1, 1]) and target f32 [B, C, H, H] in [0, 255] ->
    (det_in f32 [M B, 3, Hd, Hd], row m B + b; pix f32 [B, M] = mean((target - s)^2) per sample and modality), with
    s = (synth + 1) * (255 / 2).  Up to 256^2 det_in is bitwise the torch composition and the modality split."""
    return _Prep.apply(synth, target)


class _SqdistRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, tf):
        _hip.require_device(f, tf)
        if f.ndim != 2 or f.shape != tf.shape or f.dtype != torch.float32 or tf.dtype != torch.float32 or \
                f.shape[0] < 1 or f.shape[1] < 1:
            raise RuntimeError(f'proj_loss.sqdist_rows: f and tf must be float32 [R, F] of one shape with R, F >= 1; '
                               f'got {f.dtype} {list(f.shape)} and {tf.dtype} {list(tf.shape)}')
        f, tf = f.contiguous(), tf.detach().contiguous()
        rows, n = f.shape
        L = _hip.lib()
        nbytes = ctypes.c_int64(0)
        _hip.check(L.sg2_sqdist_rows_scratch_bytes(ctypes.byref(nbytes), rows, n), 'sg2_sqdist_rows_scratch_bytes')
        with torch.cuda.device(f.device):
            scratch = torch.empty([nbytes.value // 4], dtype=torch.float32, device=f.device)
            dist = torch.empty([rows], dtype=torch.float32, device=f.device)
            _hip.check(L.sg2_sqdist_rows_fwd(_hip.ptr(dist), _hip.ptr(f), _hip.ptr(tf), rows, n, _hip.ptr(scratch),
                                             scratch.numel() * 4, _hip.stream_ptr(f.device)), 'sg2_sqdist_rows_fwd')
        ctx.save_for_backward(f, tf)
        return dist

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError('proj_loss.sqdist_rows is first order only: its backward cannot be differentiated '
                               '(create_graph=True)')
        f, tf = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        with torch.cuda.device(f.device):
            gf = torch.empty_like(f)
            _hip.check(_hip.lib().sg2_sqdist_rows_bwd(_hip.ptr(gf), _hip.ptr(g), _hip.ptr(f), _hip.ptr(tf), f.shape[0],
                                                      f.shape[1], _hip.stream_ptr(f.device)), 'sg2_sqdist_rows_bwd')
        return gf, None


def sqdist_rows(f, tf):
    """f, tf f32 [R, F] -> f32 [R]: the squared distance of every row pair.  Bitwise reproducible; a row gives the same
    bits alone or in a batch, aligned or not."""
    return _SqdistRows.apply(f, tf)


# ---- the torch composition with per-sample reductions (any device) ----

def split_rows(img):
    """[B, C, H, W] -> [M B, 3, H, W], row m B + b: projector.split_modalities with the modalities stacked."""
    c = img.shape[1]
    if c == 3:
        return img
    return torch.cat([img[:, i:i + 1].repeat([1, 3, 1, 1]) for i in range(c)], dim=0)


def prep_ref(synth, target):
    b, c, h, _ = synth.shape
    m = num_modalities(c)
    s = split_rows((synth + 1) * (255 / 2))
    t = split_rows(target.to(torch.float32))
    pix = (t - s).square().mean(dim=(1, 2, 3)).view(m, b).t()
    if h > 256:
        s = F.interpolate(s, size=(256, 256), mode='area')
    return s, pix


def sqdist_rows_ref(f, tf):
    return (tf - f).square().sum(dim=1)
