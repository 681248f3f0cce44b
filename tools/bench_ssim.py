"""ms per call of the fused SSIM / MSE kernel (torch_utils.ops.ssim.ssim_mse) against the float64 torch composition
(ssim_mse_ref) at [32, 2, 256, 256] and [8, 2, 1024, 1024], with the map and without.

    python tools/bench_ssim.py [--rounds 3] [--kernel-calls 200] [--ref-calls 5]
    rocprofv3 --pmc FETCH_SIZE -d OUT -- python tools/bench_ssim.py --traffic      (a run of its own per counter:
    rocprofv3 --pmc WRITE_SIZE -d OUT -- python tools/bench_ssim.py --traffic       both in one pass are refused)

Timing: the host clock around `calls` back-to-back calls that end in a device synchronise, divided by `calls`: the op
as a user calls it (its three allocations and two launches included).  Both sides run in one process; a round measures
every configuration once and the order alternates from round to round; one untimed pass over all configurations goes
first (code objects, allocator, library algorithm choices).  Reported per configuration: the median of the rounds and
[min, max].  Before timing, the two sides' outputs are compared at the timed shapes.

Traffic: the algorithm needs 8 bytes read per pixel and channel (x and y once) and, with the map, 4 bytes written per
valid position; the tool prints those bytes per call and the rate they amount to at the measured time.  What the
kernel really moves to and from HBM is counted by the profiler: --traffic runs each kernel configuration exactly once
(after one warm-up call at another shape) for the counter runs, whose FETCH_SIZE + WRITE_SIZE per dispatch over the
pixel count is the measured bytes per pixel.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'gan-track_amd'),):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(32, 2, 256, 256), (8, 2, 1024, 1024)]


def make_pair(shape, dev):
    g = torch.Generator().manual_seed(shape[2])
    x = torch.nn.functional.avg_pool2d(torch.rand(shape, generator=g), 5, stride=1, padding=2) * 255
    y = (x + 8 * torch.randn(shape, generator=g)).clamp(0, 255)
    return x.to(dev).contiguous(), y.to(dev).contiguous()


def algorithmic_bytes(shape, want_map):
    N, C, H, W = shape
    return N * C * (8 * H * W + (4 * (H - 10) * (W - 10) if want_map else 0))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-calls', type=int, default=200)
    ap.add_argument('--ref-calls', type=int, default=5)
    ap.add_argument('--traffic', action='store_true', help='one kernel call per configuration, for a counter run')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ssim measures on the GPU only'
    from torch_utils.ops import ssim
    os.environ.pop('SG2_SSIM_FUSED', None)
    dev = torch.device('cuda', 0)
    pairs = {s: make_pair(s, dev) for s in SHAPES}

    if args.traffic:
        ssim.ssim_mse(*make_pair((1, 1, 64, 64), dev), want_map=True)
        torch.cuda.synchronize()
        for s in SHAPES:
            for want_map in (True, False):
                ssim.ssim_mse(*pairs[s], want_map=want_map)
                torch.cuda.synchronize()
                print(f'traffic: {list(s)} map={want_map}: {s[0] * s[1] * s[2] * s[3]} pixels, algorithmic '
                      f'{algorithmic_bytes(s, want_map)} bytes')
        return

    for s in SHAPES:        # the two sides at the timed shapes: reordered float64 sums only
        (ko, km), (ro, rm) = ssim.ssim_mse(*pairs[s], want_map=True), ssim.ssim_mse_ref(*pairs[s], want_map=True)
        e_ssim = float((ko[..., 0] - ro[..., 0]).abs().max())
        e_mse = float(((ko[..., 1] - ro[..., 1]).abs() / ro[..., 1]).max())
        e_map = float((km.double() - rm.double()).abs().max())
        print(f'{list(s)}: kernel against composition: mean SSIM {e_ssim:.3g}, MSE rel {e_mse:.3g}, f32 map {e_map:.3g}')
        assert e_ssim <= 1e-9 and e_mse <= 1e-13 and e_map <= 1.2e-7
        del km, rm

    configs = [(s, want_map, side) for s in SHAPES for want_map in (True, False) for side in ('kernel', 'composition')]

    def measure(config, scale=1.0):
        s, want_map, side = config
        x, y = pairs[s]
        if side == 'kernel':
            return timed(lambda: ssim.ssim_mse(x, y, want_map=want_map), max(1, int(args.kernel_calls * scale)))
        return timed(lambda: ssim.ssim_mse_ref(x, y, want_map=want_map), max(1, int(args.ref_calls * scale)))

    for c in configs:
        measure(c, 0.2)
    res = {c: [] for c in configs}
    for r in range(args.rounds):
        for c in (configs if r % 2 == 0 else configs[::-1]):
            res[c].append(measure(c))
        print(f'round {r} done', flush=True)

    rows = []
    print(f'\n{"shape":<22s}{"map":<6s}{"side":<13s}{"ms / call (median [min, max])":<34s}{"algorithmic GB/s":>17s}')
    for c in configs:
        s, want_map, side = c
        med = statistics.median(res[c])
        rate = algorithmic_bytes(s, want_map) / (med * 1e-3) / 1e9
        print(f'{str(list(s)):<22s}{str(want_map):<6s}{side:<13s}'
              f'{f"{med:.4f} [{min(res[c]):.4f}, {max(res[c]):.4f}]":<34s}{rate:>17.1f}')
        rows.append(dict(shape=list(s), map=want_map, side=side, ms=med, ms_min=min(res[c]), ms_max=max(res[c]),
                         algorithmic_bytes=algorithmic_bytes(s, want_map), algorithmic_gb_per_s=rate))
    for s in SHAPES:
        for want_map in (True, False):
            k, r = statistics.median(res[(s, want_map, 'kernel')]), statistics.median(res[(s, want_map, 'composition')])
            print(f'{list(s)} map={want_map}: the kernel takes {k / r:.4f} of the composition\'s time ({r / k:.1f}x)')
    print(json.dumps(dict(tool='bench_ssim', rounds=args.rounds, kernel_calls=args.kernel_calls, ref_calls=args.ref_calls,
                          device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == '__main__':
    main()
