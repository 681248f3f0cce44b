"""Times the density / coverage distance pass at the metric's own shape (n = m = 50 000, d = 4096, k = 5, random fp16
features): the fused ball-count kernel (torch_utils/ops/manifold.py manifold_count) against the membership kernel it
shares its GEMM with (manifold_member) and against the composition (metrics/density_coverage.py composed_count:
float32 torch.cdist in row blocks, rounded to fp16, `<=`, sum(1), any(0)) on the same GPU.

    python tools/prdc_micro.py [--n 50000 --m 50000 --d 4096 --k 5 --windows 5 --log profiles/prdc_metric/prdc_micro.txt]

All sides run in one process, alternating, after a warm-up; every window is one call between two events; median and
minimum are reported, with the fused passes' TFLOP/s (2 d FLOP per pair) as a fraction of the 2.5 PFLOP/s fp16 MFMA
peak, the count / member ratio (of the medians, and per window: its spread) and how often the fused and the composed
counts and flags agree.  Prints one JSON line last."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gan-track_amd'), ROOT]

import torch  # noqa: E402

PEAK_TFLOPS = 2500.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000, help='manifold size (real features)')
    ap.add_argument('--m', type=int, default=50000, help='probes (generated features)')
    ap.add_argument('--d', type=int, default=4096)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--no-composed', action='store_true', help='time the two fused passes alone')
    ap.add_argument('--log', default=None)
    args = ap.parse_args()

    from metrics import density_coverage
    from torch_utils.ops import manifold
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    g = torch.Generator(device='cuda').manual_seed(0)
    # VGG-like: non-negative, sparse-ish features
    mani = torch.randn([args.n, args.d], device='cuda', generator=g).clamp_(min=0).to(torch.float16)
    probes = torch.randn([args.m, args.d], device='cuda', generator=g).clamp_(min=0).to(torch.float16)
    say(f'{torch.cuda.get_device_name(0)}: n {args.n} m {args.m} d {args.d} k {args.k}')
    radii = manifold.knn_radii(mani, args.k)

    sides = {'fused_count': lambda: manifold.manifold_count(probes, mani, radii),
             'fused_member': lambda: manifold.manifold_member(probes, mani, radii)}
    if not args.no_composed:
        sides['composed_count'] = lambda: density_coverage.composed_count(probes, mani, radii)
    outs = {name: fn() for name, fn in sides.items()}       # warm-up
    torch.cuda.synchronize()
    count, covered = outs['fused_count']
    say(f'count > 0 equals membership on {float(((count > 0) == outs["fused_member"]).float().mean()):.6f} of the '
        f'probes; density {int(count.sum()) / (args.k * args.m):.4f}, coverage {float(covered.float().mean()):.4f}, '
        f'largest count {int(count.max())}')
    agreement = None
    if not args.no_composed:
        c_count, c_covered = outs['composed_count']
        agreement = dict(count=float((count == c_count).float().mean()),
                         covered=float((covered == c_covered).float().mean()))
        say(f'fused vs composed: counts equal on {agreement["count"]:.6f} of the probes, flags on '
            f'{agreement["covered"]:.6f} of the reals')
    del outs
    times = {name: [] for name in sides}
    for w in range(args.windows):
        for name, fn in sides.items():                      # alternate the sides within a window
            ms, out = timed(fn)
            del out
            times[name].append(ms)
        print(f'window {w}: ' + ', '.join(f'{name} {ts[-1]:.2f} ms' for name, ts in times.items()), flush=True)
    result = dict(n=args.n, m=args.m, d=args.d, k=args.k, agreement=agreement)
    for name, ts in times.items():
        med, lo = statistics.median(ts), min(ts)
        tflops = 2.0 * args.d * args.m * args.n / (med * 1e-3) / 1e12
        extra = f'  {tflops:7.1f} TFLOP/s = {tflops / PEAK_TFLOPS:.3f} of peak' if name.startswith('fused') else ''
        say(f'{name:14s} median {med:10.3f} ms  min {lo:10.3f} ms  max {max(ts):10.3f} ms  ({len(ts)} windows){extra}')
        result[name] = dict(median_ms=med, min_ms=lo, max_ms=max(ts))
        if name.startswith('fused'):
            result[name].update(tflops=tflops, of_peak=tflops / PEAK_TFLOPS)
    ratios = [c / h for c, h in zip(times['fused_count'], times['fused_member'])]
    member = times['fused_member']
    result['count_over_member'] = dict(of_medians=result['fused_count']['median_ms'] / result['fused_member']['median_ms'],
                                       min=min(ratios), max=max(ratios),
                                       member_spread=max(member) / min(member))
    say(f'count / member: {result["count_over_member"]["of_medians"]:.4f} of the medians, per window '
        f'{min(ratios):.4f} .. {max(ratios):.4f}; the member pass itself spreads max / min = '
        f'{max(member) / min(member):.4f}')
    say(json.dumps(result))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
