"""A/B of the stride-1 halo conv's LDS-DMA form (SG2_HALO_DMA=1, default) against the register-staged kernel (=0) on
the bench's halo shapes, four forms each: plain (dgrad), bias + lrelu epilogue with the raw output (the D block's conv),
out_scale + dot (the modulated layers' dgrad), and the modulated layer with the full epilogue and raw output (G
forward).  The arms alternate several times in one process; prints ms per launch and TFLOP/s for every alternation,
so the spread between repeats of one arm stands beside the difference between the arms.
Usage: python tools/halo_dma_ab.py [alternations, default 3] [fp16 | bf16]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gan-track_amd'), ROOT]
from torch_utils.ops import conv2d_gradfix as cg  # noqa: E402

ALT = int(sys.argv[1]) if len(sys.argv) > 1 else 3
DT = {'fp16': torch.float16, 'bf16': torch.bfloat16}[sys.argv[2] if len(sys.argv) > 2 else 'fp16']
dev = torch.device('cuda', 0)
_t = torch.randn(4096, 4096, device=dev, dtype=torch.float16)
for _ in range(200):
    _t = (_t @ _t).clamp_(-1, 1)


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


for N in (32, 64):
    for C, R in [(128, 128), (256, 64), (512, 32)]:
        x = torch.randn(N, C, R, R, device=dev, dtype=DT).contiguous(memory_format=torch.channels_last)
        wp = cg._pack_conv((torch.randn(C, C, 3, 3, device=dev) / np.sqrt(9 * C)).to(DT))
        s = torch.rand(N, C, device=dev) + 0.5
        nz = torch.randn(N, R, R, device=dev, dtype=DT)
        b = torch.zeros(C, device=dev)
        src = torch.randn(N, C, R, R, device=dev, dtype=DT).contiguous(memory_format=torch.channels_last)
        forms = {
            'plain': lambda: cg.conv3x3_fused(x, wp, C),
            'epi+raw': lambda: cg.conv3x3_fused(x, wp, C, bias=b, act=1, gain=1.41, clamp=256.0, want_raw=True),
            'dgrad+dot': lambda: cg.conv3x3_fused(x, wp, C, out_scale=s, dot_src=src),
            'modulated': lambda: cg.conv3x3_fused(x, wp, C, in_scale=s, out_scale=s, noise=nz, noise_gain=0.1, bias=b,
                                                  act=1, gain=1.41, clamp=256.0, want_raw=True),
        }
        fl = 2.0 * N * C * C * 9 * R * R
        for name, fn in forms.items():
            ms = {'0': [], '1': []}
            for _ in range(ALT):
                for env in ('0', '1'):
                    os.environ['SG2_HALO_DMA'] = env
                    ms[env].append(timeit(fn))
            line = ' | '.join(f"dma={env}: " + ' '.join(f'{m:.4f}' for m in ms[env]) +
                              f" ms ({fl / min(ms[env]) / 1e9:.0f} TF/s best)" for env in ('0', '1'))
            gain = min(ms['0']) / max(ms['1'])      # the slowest new run against the fastest old one
            print(f'N={N} C={C} {R}^2 {name:10s}: {line} | worst-case speed-up {gain:.3f}', flush=True)
os.environ['SG2_HALO_DMA'] = '1'
