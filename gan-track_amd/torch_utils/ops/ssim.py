"""Structural similarity and mean squared error of image pairs (HIP kernel sg2_ssim_mse, csrc/ssim.hip).

SSIM as Wang, Bovik, Sheikh and Simoncelli defined it (IEEE TIP 13(4), 2004): an 11 x 11 Gaussian window of sigma 1.5
normalised to sum 1, valid positions only ((H - 10) x (W - 10), no padding), population moments

    mx = sum w x,   sxx = sum w x^2 - mx^2,   sxy = sum w x y - mx my
    ssim = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),   C1 = (0.01 L)^2, C2 = (0.03 L)^2

with L = data_range.  ssim_mse returns, per image and channel, the mean of the map and the mean of (x - y)^2 over all
pixels, both float64.  The moments are float64 on both paths: sxx is a difference of two numbers near L^2 that is
divided by something as small as C2 = L^2 / 1111, so float32 moments miss the map by 1e-5 on a flat image.

On ROCm tensors it is one fused kernel that reads the two images once (bitwise reproducible; a pair gives the same bits
alone or in a batch).  ssim_mse_ref is the torch composition in float64 on any device (two separable F.conv2d passes
per moment): the A/B partner selected by SG2_SSIM_FUSED=0, and the in-repo cross-check.  Not differentiable.
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import sg2hip as _hip

TAPS = 11
SIGMA = 1.5
TILE_H, TILE_W = 16, 32     # the kernel's output tile (csrc/ssim.hip SS_TH, SS_TW)
MIN_HW, MAX_HW = 11, 1024


def fused_enabled():
    """SG2_SSIM_FUSED=0 selects the composition; anything else the kernel."""
    return os.environ.get('SG2_SSIM_FUSED', '1') != '0'


def gaussian_window():
    """float64 numpy [11]: g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)), normalised to sum 1.  The 2-D window is g g^T."""
    k = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    g = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def psnr(mse, data_range=255.0):
    """10 log10(L^2 / mse) on the host; inf at mse == 0."""
    mse = float(mse)
    if mse == 0.0:
        return math.inf
    return 10.0 * math.log10(float(data_range) ** 2 / mse)


def _check(x, y, data_range, what):
    for name, t in (('x', x), ('y', y)):
        if not isinstance(t, torch.Tensor) or t.ndim != 4:
            raise RuntimeError(f'{what}: {name} must be a [N, C, H, W] tensor; got '
                               f'{list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}')
        if t.dtype != torch.float32:
            raise RuntimeError(f'{what}: {name} must be float32; got {t.dtype}')
    if x.shape != y.shape:
        raise RuntimeError(f'{what}: x {list(x.shape)} and y {list(y.shape)} must have one shape')
    if x.device != y.device:
        raise RuntimeError(f'{what}: x on {x.device} and y on {y.device} must share a device')
    N, C, H, W = x.shape
    if N < 1 or C < 1 or not (MIN_HW <= H <= MAX_HW and MIN_HW <= W <= MAX_HW):
        raise RuntimeError(f'{what}: N, C must be >= 1 and H, W in {MIN_HW}..{MAX_HW}; got {list(x.shape)}')
    if not float(data_range) > 0:
        raise RuntimeError(f'{what}: data_range must be > 0; got {data_range}')


def ssim_mse_ref(x, y, data_range=255.0, want_map=False):
    """The composition in float64 torch on the tensors' device: every moment is a horizontal and a vertical F.conv2d
    with the 11 weights.  Returns f64 [N, C, 2] (mean SSIM, MSE) and, with want_map, the f32 map [N, C, H-10, W-10]."""
    _check(x, y, data_range, 'ssim_mse_ref')
    N, C, H, W = x.shape
    g = torch.from_numpy(gaussian_window()).to(x.device)
    xd = x.detach().to(torch.float64).reshape(N * C, 1, H, W)
    yd = y.detach().to(torch.float64).reshape(N * C, 1, H, W)

    def blur(t):
        return F.conv2d(F.conv2d(t, g.view(1, 1, 1, TAPS)), g.view(1, 1, TAPS, 1))

    mx, my = blur(xd), blur(yd)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = blur(xd * xd) - mxx, blur(yd * yd) - myy, blur(xd * yd) - mxy
    c1, c2 = (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2
    smap = ((2.0 * mxy + c1) * (2.0 * sxy + c2)) / ((mxx + myy + c1) * (sxx + syy + c2))
    out = torch.stack([smap.mean(dim=(1, 2, 3)), (xd - yd).square().mean(dim=(1, 2, 3))], dim=1).reshape(N, C, 2)
    if want_map:
        return out, smap.to(torch.float32).reshape(N, C, H - TAPS + 1, W - TAPS + 1)
    return out


def ssim_mse(x, y, data_range=255.0, want_map=False):
    """x, y: ROCm float32 [N, C, H, W] of one shape, H and W in 11..1024.  Returns float64 [N, C, 2]: per image and
    channel the mean SSIM over the (H - 10) x (W - 10) valid positions and the mean squared error over all pixels;
    with want_map also the float32 SSIM map [N, C, H - 10, W - 10].  One fused kernel call (module docstring);
    SG2_SSIM_FUSED=0 runs ssim_mse_ref on the same tensors instead."""
    _check(x, y, data_range, 'ssim_mse')
    _hip.require_device(x, y)
    if not fused_enabled():
        return ssim_mse_ref(x, y, data_range, want_map)
    N, C, H, W = x.shape
    x, y = x.detach().contiguous(), y.detach().contiguous()
    dev = x.device
    lib = _hip.lib()
    nbytes = ctypes.c_int64(0)
    _hip.check(lib.sg2_ssim_scratch_bytes(ctypes.byref(nbytes), N, C, H, W), 'sg2_ssim_scratch_bytes')
    window = (ctypes.c_double * TAPS)(*gaussian_window().tolist())
    with torch.cuda.device(dev):
        out = torch.empty([N, C, 2], dtype=torch.float64, device=dev)
        smap = torch.empty([N, C, H - TAPS + 1, W - TAPS + 1], dtype=torch.float32, device=dev) if want_map else None
        scratch = torch.empty([(nbytes.value + 7) // 8], dtype=torch.float64, device=dev)
        _hip.check(lib.sg2_ssim_mse(_hip.ptr(out), _hip.ptr(smap), _hip.ptr(x), _hip.ptr(y), N, C, H, W, window,
                                    float(data_range), _hip.ptr(scratch), scratch.numel() * 8, _hip.stream_ptr(dev)),
                   'sg2_ssim_mse')
    return (out, smap) if want_map else out
