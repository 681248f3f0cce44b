"""Time of the summed power spectrum at the production shape (GPU measurement): the fused kernel
(torch_utils/ops/power_spectrum.batch_power) against the reference's composition in torch on the same device
(power_spectrum.batch_power_ref, what SG2_SPECTRA_FUSED=0 runs) -- B = 32 uint8 images of one channel, N = 256,
interp = 4.  Same process, after a warm-up of both, the two alternating; each time is a host clock around one call
that ends in a device synchronise (so the fused time includes the upload of its window and twiddle table), reported
as the median [min, max] of the runs.  If torch.fft does not run in float64 on this build, the composition is timed on
the host instead and the line says so.
    python tools/spectra_time.py [--runs 7] [--B 32] [--C 1] [--N 256] [--interp 4] [--out profiles/spectra]
        [--name spectra_time.txt]
Prints one JSON line and appends it to <out>/<name>.  FLOP/s: `executed` counts the f64 MFMA work the fused
kernel launches (whole 16 x 16 x 4 instructions of both passes, tails and the padded columns included); `algorithm`
counts the pruned DFT itself (row pass 4 N N (S / 2 + 1), column pass 8 S N (S / 2 + 1) per image-channel)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gan-track_amd'), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--B', type=int, default=32)
    ap.add_argument('--C', type=int, default=1)
    ap.add_argument('--N', type=int, default=256)
    ap.add_argument('--interp', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spectra'))
    ap.add_argument('--name', default='spectra_time.txt', help='file name under --out; the line is appended')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'spectra_time.py measures on the GPU'
    assert a.runs >= 5
    from torch_utils.ops import power_spectrum
    os.environ['SG2_SPECTRA_FUSED'] = '1'           # the kernel at every size it takes (the default stops at N = 512)
    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(0)
    host = torch.from_numpy(rs.randint(0, 256, size=[a.B, a.C, a.N, a.N]).astype(np.uint8))
    x = host.to(dev)
    mean, std = [112.684] * a.C, [69.509] * a.C
    w = power_spectrum.kaiser_window(a.N, 8)

    comp_where = 'device'
    try:
        power_spectrum.batch_power_ref(x[:1], mean, std, w, a.interp)
        torch.cuda.synchronize(dev)
        comp_in = x
    except RuntimeError as e:
        comp_where = f'host (torch.fft in float64 failed on the device: {str(e).splitlines()[0][:120]})'
        comp_in = host

    def timed(fn, inp):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn(inp, mean, std, w, a.interp)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    for _ in range(2):                                  # warm-up: code objects, FFT plans
        timed(power_spectrum.batch_power, x)
        timed(power_spectrum.batch_power_ref, comp_in)
    t_fused, t_comp = [], []
    for _ in range(a.runs):
        tf, p_fused = timed(power_spectrum.batch_power, x)
        tc, p_comp = timed(power_spectrum.batch_power_ref, comp_in)
        t_fused.append(tf)
        t_comp.append(tc)
    # the kernels alone: device events around `runs` back-to-back fused calls (uploads overlap the previous call)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.runs):
        power_spectrum.batch_power(x, mean, std, w, a.interp)
    e1.record()
    torch.cuda.synchronize(dev)
    dev_s = e0.elapsed_time(e1) / a.runs / 1e3
    rel = float(((p_fused.cpu() - p_comp.cpu()).abs() / p_comp.cpu().abs()).max())
    S = a.N * a.interp
    vh = S // 2 + 1
    vp = -(-vh // 32) * 32
    n32 = -(-a.N // 32) * 32
    s32 = -(-S // 32) * 32
    flop_alg = float(a.B * a.C) * (4.0 * a.N * a.N * vh + 8.0 * S * a.N * vh)
    flop_exec = float(a.B * a.C) * (4.0 * n32 * a.N * vp + 8.0 * s32 * a.N * vp)
    mf, mc = statistics.median(t_fused), statistics.median(t_comp)
    line = json.dumps(dict(
        shape=dict(B=a.B, C=a.C, N=a.N, interp=a.interp, dtype='uint8'), runs=a.runs, composition_on=comp_where,
        fused_ms=round(mf * 1e3, 3), fused_ms_min_max=[round(min(t_fused) * 1e3, 3), round(max(t_fused) * 1e3, 3)],
        composition_ms=round(mc * 1e3, 3),
        composition_ms_min_max=[round(min(t_comp) * 1e3, 3), round(max(t_comp) * 1e3, 3)],
        composition_over_fused=round(mc / mf, 3),
        fused_f64_tflops_algorithm=round(flop_alg / mf / 1e12, 2),
        fused_f64_tflops_executed=round(flop_exec / mf / 1e12, 2),
        fused_back_to_back_ms=round(dev_s * 1e3, 3),
        fused_back_to_back_f64_tflops_executed=round(flop_exec / dev_s / 1e12, 2),
        power_max_rel_diff=rel))
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), 'a') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
