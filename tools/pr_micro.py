"""Times the precision / recall distance passes at the metric's own shape (n = m = 50 000, d = 4096, k = 3, random
fp16 features): the fused radii and membership kernels (torch_utils/ops/manifold.py) against the reference's method
expressed in torch on the same GPU -- fp16 torch.cdist over 10 000 x 10 000 blocks, the blocks concatenated, kthvalue
and `<=` / any kept on the device (generous to the baseline: the reference copies every block to the host first;
SG3/metrics/precision_recall.py:19-61).

    python tools/pr_micro.py [--n 50000 --m 50000 --d 4096 --k 3 --windows 5 --log profiles/pr_metric/pr_micro.txt]

Both sides run in one process, alternating, after a warm-up; every window is one call between two events; median and
minimum are reported, with the fused passes' TFLOP/s (2 d FLOP per pair) as a fraction of the 2.5 PFLOP/s fp16 MFMA
peak.  Prints one JSON line last."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'gan-track_amd'), ROOT]

import torch  # noqa: E402

PEAK_TFLOPS = 2500.0


def ref_distances(rows, cols, col_batch):
    return torch.cat([torch.cdist(rows.unsqueeze(0), c.unsqueeze(0))[0] for c in cols.split(col_batch)], dim=1)


def ref_radii(x, k, batch):
    return torch.cat([ref_distances(rb, x, batch).to(torch.float32).kthvalue(k + 1).values.to(torch.float16)
                      for rb in x.split(batch)])


def ref_member(probes, mani, kth, batch):
    return torch.cat([(ref_distances(pb, mani, batch) <= kth).any(dim=1) for pb in probes.split(batch)])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000, help='manifold size')
    ap.add_argument('--m', type=int, default=50000, help='probes')
    ap.add_argument('--d', type=int, default=4096)
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--batch', type=int, default=10000, help="the baseline's block size")
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--log', default=None)
    args = ap.parse_args()

    from torch_utils.ops import manifold
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    g = torch.Generator(device='cuda').manual_seed(0)
    # VGG-like: non-negative, sparse-ish features
    mani = torch.randn([args.n, args.d], device='cuda', generator=g).clamp_(min=0).to(torch.float16)
    probes = torch.randn([args.m, args.d], device='cuda', generator=g).clamp_(min=0).to(torch.float16)
    say(f'{torch.cuda.get_device_name(0)}: n {args.n} m {args.m} d {args.d} k {args.k} baseline block {args.batch}')

    sides = {'fused_radii': lambda: manifold.knn_radii(mani, args.k)}
    radii = sides['fused_radii']()
    sides['fused_member'] = lambda: manifold.manifold_member(probes, mani, radii)
    if not args.no_baseline:
        sides['torch_radii'] = lambda: ref_radii(mani, args.k, args.batch)
        sides['torch_member'] = lambda: ref_member(probes, mani, radii.to(torch.float16), args.batch)
    outs = {name: fn() for name, fn in sides.items()}       # warm-up
    torch.cuda.synchronize()
    if not args.no_baseline:
        r_f, r_t = outs['fused_radii'], outs['torch_radii'].float()
        h_f, h_t = outs['fused_member'], outs['torch_member']
        say(f'radii: fused vs torch equal {float((r_f == r_t).float().mean()):.4f}, within one fp16 ulp '
            f'{float(((r_f - r_t).abs() <= r_t.abs() * 2.0 ** -10).float().mean()):.4f}; '
            f'membership equal {float((h_f == h_t).float().mean()):.4f} (hits {float(h_f.float().mean()):.4f})')
    times = {name: [] for name in sides}
    for w in range(args.windows):
        for name, fn in sides.items():                      # alternate the sides within a window
            ms, out = timed(fn)
            del out
            times[name].append(ms)
        print(f'window {w}: ' + ', '.join(f'{name} {ts[-1]:.2f} ms' for name, ts in times.items()), flush=True)
    result = dict(n=args.n, m=args.m, d=args.d, k=args.k)
    for name, ts in times.items():
        med, lo = statistics.median(ts), min(ts)
        pairs = args.n * args.n if name.endswith('radii') else args.m * args.n
        tflops = 2.0 * args.d * pairs / (med * 1e-3) / 1e12
        extra = f'  {tflops:7.1f} TFLOP/s = {tflops / PEAK_TFLOPS:.3f} of peak' if name.startswith('fused') else ''
        say(f'{name:13s} median {med:10.3f} ms  min {lo:10.3f} ms  ({len(ts)} windows){extra}')
        result[name] = dict(median_ms=med, min_ms=lo)
        if name.startswith('fused'):
            result[name].update(tflops=tflops, of_peak=tflops / PEAK_TFLOPS)
    say(json.dumps(result))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
