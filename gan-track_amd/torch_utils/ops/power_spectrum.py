"""Summed 2-D power spectrum of a batch of windowed, zero-padded images (HIP kernel sg2_power_spectrum_sum,
csrc/spectrum.hip).

The reference whitens one image at a time in float64, multiplies it with the outer product of a Kaiser window, pads it
to S = N * interp, runs `torch.fft.fftn` and adds `abs().square()` averaged over the channels
(SG3/avg_spectra.py:157-166).  batch_power returns the same quantity summed over a batch and kept per channel:

    out[c, u, v] = sum_b | sum_{y, x} ((x[b, c, y, x] - mean[c]) / std[c]) w[y] w[x] exp(-2 pi i (u y + v x) / S) |^2

as float64 [C, S, S].  On a ROCm tensor it is a pruned DFT on the f64 matrix instruction (no padding, no complex
spectrum in memory); batch_power_ref is the reference's composition in torch on any device, selected by
SG2_SPECTRA_FUSED=0 and used for CPU tensors, for the sizes the kernel does not take and, unless SG2_SPECTRA_FUSED=1,
from N = 512 on, where the FFT was measured faster than the direct DFT.  Not differentiable.
"""
import ctypes
import functools
import os

import numpy as np
import torch

import sg2hip as _hip

MAX_S = 4096


# The direct DFT's work per output bin grows with N where the FFT's does not: measured on the MI355X (DESIGN.md
# section 12) the fused call takes 0.59 of the composition's time at N = 256, 1.10 at N = 512 and 1.64 at N = 1024,
# at a batch of 32 as at equal S^2 B.  Unless SG2_SPECTRA_FUSED says otherwise the kernel runs below this size and
# the composition from it on (which then holds 24 S^2 B bytes of padded input and complex spectrum).
AUTO_FUSED_BELOW_N = 512


def fused_enabled(n):
    """Whether batch_power runs the fused kernel at image size n: SG2_SPECTRA_FUSED=0 never, =1 at every size the
    kernel takes, unset (or anything else) below AUTO_FUSED_BELOW_N."""
    env = os.environ.get('SG2_SPECTRA_FUSED')
    if env in ('0', '1'):
        return env == '1'
    return n < AUTO_FUSED_BELOW_N


def kaiser_window(n, beta):
    """float64 [n] on the CPU: torch.kaiser_window(periodic=False) normalised to unit energy with the reference's
    own operations (SG3/avg_spectra.py:157-158), so the kernel, the composition and the tests' oracle share its bits."""
    window = torch.kaiser_window(int(n), periodic=False, beta=float(beta), dtype=torch.float64, device='cpu')
    window *= window.square().sum().rsqrt()
    return window


@functools.lru_cache(maxsize=8)
def twiddle_table(S):
    """float64 numpy [S, 2]: (cos, -sin)(2 pi k / S), computed in long double on the first octant and completed by
    symmetry, so tw[S - k] = conj(tw[k]) and the axis values are exact: the kernel's Hermitian symmetry rests on it."""
    S = int(S)
    assert S >= 4 and S % 4 == 0, S
    tw = np.zeros([S, 2], dtype=np.float64)
    half, q = S // 2, S // 4
    # the argument is reduced to [0, pi / 4] first: cos and sin of one octant, swapped and negated for the others
    k = np.arange(half + 1)
    r = np.where(k <= q, k, half - k)                               # distance to the nearer of 0 and pi
    r8 = np.where(2 * r <= q, r, q - r)                             # ... reduced to the first octant
    ang = r8.astype(np.longdouble) * (np.longdouble(2) * _PI_LD / np.longdouble(S))
    c8, s8 = np.cos(ang), np.sin(ang)
    cr = np.where(2 * r <= q, c8, s8)                               # cos, sin of 2 pi r / S, r in [0, S / 4]
    sr = np.where(2 * r <= q, s8, c8)
    tw[:half + 1, 0] = np.where(k <= q, cr, -cr).astype(np.float64)
    tw[:half + 1, 1] = -sr.astype(np.float64)
    tw[0], tw[q], tw[half] = (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)
    for j in range(1, half):
        tw[S - j] = (tw[j, 0], -tw[j, 1])
    tw[tw == 0] = 0.0                                               # no negative zeros
    tw.setflags(write=False)
    return tw


_PI_LD = np.longdouble('3.14159265358979323846264338327950288419716939937510')


def _check(images, mean, std, window, interp, what):
    if images.ndim != 4 or images.shape[2] != images.shape[3] or images.shape[0] < 1 or images.shape[1] < 1:
        raise RuntimeError(f'{what}: images must be [B, C, N, N] with B >= 1; got {list(images.shape)}')
    if images.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f'{what}: images must be uint8 or float32; got {images.dtype}')
    C, N = images.shape[1], images.shape[2]
    mean = torch.as_tensor(mean, dtype=torch.float64).detach().cpu().reshape(-1)
    std = torch.as_tensor(std, dtype=torch.float64).detach().cpu().reshape(-1)
    if mean.numel() != C or std.numel() != C:
        raise RuntimeError(f'{what}: mean {list(mean.shape)} and std {list(std.shape)} must hold one value per channel '
                           f'of images {list(images.shape)}')
    if not bool((std > 0).all()):
        raise RuntimeError(f'{what}: std must be > 0; got {std.tolist()}')
    window = torch.as_tensor(window).detach()
    if window.ndim != 1 or window.numel() != N or window.dtype != torch.float64:
        raise RuntimeError(f'{what}: window must be float64 [{N}]; got {window.dtype} {list(window.shape)} '
                           f'for images {list(images.shape)}')
    if int(interp) != interp or interp < 1:
        raise RuntimeError(f'{what}: interp must be an integer >= 1; got {interp}')
    return mean, std, window.cpu(), int(interp)


def kernel_takes(B, C, N, interp):
    """Whether sg2_power_spectrum_sum accepts the shape (include/sg2hip.h)."""
    return N % 4 == 0 and 8 <= N <= 1024 and N * interp <= MAX_S and B * C <= 65535


def spectrum_ref(images, mean, std, window, interp):
    """complex128 [B, C, S, S]: the reference's float64 whitening, window, pad and fft.fftn of every image."""
    mean, std, window, interp = _check(images, mean, std, window, interp, 'spectrum_ref')
    dev = images.device
    N = images.shape[2]
    padding = N * interp - N
    w2 = window.to(dev)
    w2 = w2.ger(w2).unsqueeze(0).unsqueeze(1)
    x = (images.detach().to(torch.float64) - mean.to(dev).reshape(1, -1, 1, 1)) / std.to(dev).reshape(1, -1, 1, 1)
    x = torch.nn.functional.pad(x * w2, [0, padding, 0, padding])
    return torch.fft.fftn(x, dim=[2, 3])


def batch_power_ref(images, mean, std, window, interp):
    """The reference's composition in torch on the images' device: float64 whitening, window, pad, fft.fftn,
    abs().square(), summed over the batch, per channel.  float64 [C, S, S]."""
    return spectrum_ref(images, mean, std, window, interp).abs().square().sum(dim=0)


def batch_power(images, mean, std, window, interp):
    """float64 [C, S, S] on the images' device, S = N * interp: the power spectrum of every channel summed over the
    batch (module docstring).  images uint8 or float32 [B, C, N, N], any strides; mean, std: one value per channel
    (std > 0); window float64 [N].  On a ROCm tensor of a size the kernel takes and fused_enabled(N) selects, one call
    of the fused kernel: two calls give the same bits.  Otherwise batch_power_ref."""
    mean, std, window, interp = _check(images, mean, std, window, interp, 'batch_power')
    B, C, N, _ = images.shape
    if images.device.type != 'cuda' or not fused_enabled(N) or not kernel_takes(B, C, N, interp):
        return batch_power_ref(images, mean, std, window, interp)
    images = images.detach()
    dev = images.device
    S = N * interp
    nbytes = ctypes.c_int64(0)
    lib = _hip.lib()
    _hip.check(lib.sg2_power_spectrum_scratch_bytes(ctypes.byref(nbytes), B, C, N, interp),
               'sg2_power_spectrum_scratch_bytes')
    with torch.cuda.device(dev):
        # one upload; the table first, so that it sits on the allocation's 16-byte boundary
        consts = torch.cat([torch.from_numpy(np.array(twiddle_table(S))).reshape(-1), window, mean, std]).to(dev)
        d_tw, d_window, d_mean, d_std = consts[:2 * S], consts[2 * S:2 * S + N], consts[2 * S + N:2 * S + N + C], \
            consts[2 * S + N + C:]
        out = torch.empty([C, S, S], dtype=torch.float64, device=dev)
        scratch = torch.empty([(nbytes.value + 7) // 8], dtype=torch.float64, device=dev)
        _hip.check(lib.sg2_power_spectrum_sum(_hip.ptr(out), _hip.ptr(images),
                                              _hip.U8 if images.dtype == torch.uint8 else _hip.F32,
                                              _hip.i64arr(images.stride()), B, C, N, interp, _hip.ptr(d_window),
                                              _hip.ptr(d_mean), _hip.ptr(d_std), _hip.ptr(d_tw), _hip.ptr(scratch),
                                              scratch.numel() * 8, _hip.stream_ptr(dev)),
                   'sg2_power_spectrum_sum')
    return out
