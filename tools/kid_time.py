"""Time of the kernel inception distance's MMD sums at the production shape (GPU measurement): the fused kernel
(torch_utils/ops/poly_mmd.subset_sums) against the reference's composition in torch on the same device
(metrics/kernel_inception_distance.composed_subset_sums, what SG2_KID_FUSED=0 runs) -- S = 100 subsets of m = 1000
rows, d = 2048, drawn from 50 000 x 2048 features on both sides.  Same process, after a warm-up of both, the two
alternating; each time is a host clock around one call that ends in a device synchronise (so both include the
upload of their index tables), reported as the median of the runs.
    python tools/kid_time.py [--runs 7] [--S 100] [--m 1000] [--d 2048] [--n 50000]
Prints one JSON line.  FLOP/s: `algorithm` counts the reference's three full Gram matrices (6 S m^2 d); `executed`
counts the MFMA work the fused kernel launches (upper-triangle tiles only for the two symmetric Grams, whole 128 x
128 x 32 blocks), against the 157.3 TFLOP/s exact-f32 MFMA peak."""
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

F32_MFMA_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--S', type=int, default=100)
    ap.add_argument('--m', type=int, default=1000)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--n', type=int, default=50000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'kid_time.py measures on the GPU'
    assert a.runs >= 5
    from torch_utils.ops import poly_mmd
    from metrics import kernel_inception_distance as kid
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    # Inception-pool-like features: non-negative, most of the mass in a few directions
    feats = []
    for shift in (0.0, 0.1):
        low = torch.randn([a.n, 8], generator=g, device=dev) @ torch.randn([8, a.d], generator=g, device=dev) / 8 ** 0.5
        feats.append(torch.relu(low + 0.25 * torch.randn([a.n, a.d], generator=g, device=dev) + 0.5 + shift))
    gen, real = feats
    rs = np.random.RandomState(123)
    ig = np.stack([rs.choice(a.n, a.m, replace=False) for _ in range(a.S)])
    ir = np.stack([rs.choice(a.n, a.m, replace=False) for _ in range(a.S)])

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn(gen, real, ig, ir)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    for fn in (poly_mmd.subset_sums, kid.composed_subset_sums) * 2:     # warm-up: code objects, GEMM selection
        timed(fn)
    t_fused, t_comp = [], []
    for _ in range(a.runs):
        tf, s_fused = timed(poly_mmd.subset_sums)
        tc, s_comp = timed(kid.composed_subset_sums)
        t_fused.append(tf)
        t_comp.append(tc)
    rel = float(((s_fused - s_comp).abs() / s_fused.abs()).max())
    kid_f, kid_c = poly_mmd.kid_from_sums(s_fused, a.m), poly_mmd.kid_from_sums(s_comp, a.m)
    T = -(-a.m // 128)
    flop_alg = 6.0 * a.S * a.m * a.m * a.d
    flop_exec = 2.0 * 128 * 128 * (-(-a.d // 32) * 32) * a.S * (T * (T + 1) + T * T)
    mf, mc = statistics.median(t_fused), statistics.median(t_comp)
    print(json.dumps(dict(
        shape=dict(S=a.S, m=a.m, d=a.d, n=a.n), runs=a.runs,
        fused_ms=round(mf * 1e3, 3), fused_ms_min_max=[round(min(t_fused) * 1e3, 3), round(max(t_fused) * 1e3, 3)],
        composition_ms=round(mc * 1e3, 3),
        composition_ms_min_max=[round(min(t_comp) * 1e3, 3), round(max(t_comp) * 1e3, 3)],
        composition_over_fused=round(mc / mf, 3),
        fused_tflops_algorithm=round(flop_alg / mf / 1e12, 2), fused_tflops_executed=round(flop_exec / mf / 1e12, 2),
        fused_executed_share_of_f32_mfma_peak=round(flop_exec / mf / F32_MFMA_PEAK, 3),
        composition_tflops_algorithm=round(flop_alg / mc / 1e12, 2),
        sums_max_rel_diff=rel, kid_fused=kid_f, kid_composition=kid_c)))


if __name__ == '__main__':
    main()
