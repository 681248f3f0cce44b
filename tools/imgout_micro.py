"""Times of image_tiles_u8 (one launch of sg2_image_tiles_u8) against image_tiles_u8_ref (the reference's torch
composition) on the same device, in the same process.

    python tools/imgout_micro.py                     # device events, alternating windows
    python tools/imgout_micro.py --trace 20          # 20 calls of each, for a kernel trace (launches per call, kernel time):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/imgout_micro.py --trace 20
    python tools/imgout_micro.py --summarise OUT/..._kernel_trace.csv 20     # launches per call and kernel times

Shapes: [32, 2, 256, 256] as grey tiles of an 8 x 8 grid (a snapshot grid of 32 two-modality samples) and
[8, 2, 1024, 1024] as grey tiles of a 4 x 4 grid, float32 and float16 inputs, mode 'trunc'; and [32, 3, 256, 256] as
'hwc' tiles (the 4-byte-store path).  Bytes are what the algorithm needs: the input read once and one byte per pixel
written.  The canvas is allocated once outside the timed window on both sides.

Timing: after an untimed warm-up of every shape, a window of calls between two device events; fused and composition
alternate window by window, the order swapping every round; the figure is the median over the rounds of the window's
time per call.  It holds launches and the gaps between them, not kernel time alone.
"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'gan-track_amd'),):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def cases(dev):
    """name -> (fused callable, composed callable, bytes the algorithm needs)"""
    from torch_utils.ops import image_tiles as ops
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, shape, tiles, grid in (('32x2x256^2 grey 8x8', (32, 2, 256, 256), 'grey', (8, 8)),
                                     ('8x2x1024^2 grey 4x4', (8, 2, 1024, 1024), 'grey', (4, 4)),
                                     ('32x3x256^2 hwc 8x4', (32, 3, 256, 256), 'hwc', (8, 4))):
        x32 = torch.rand(shape, device=dev, generator=g) * 2.6 - 1.3
        for dt in (torch.float32, torch.float16):
            if tiles == 'hwc' and dt != torch.float32:
                continue
            x = x32.to(dt)
            cout = 3 if tiles == 'hwc' else 1
            cv = [torch.zeros([grid[1] * shape[2], grid[0] * shape[3], cout], dtype=torch.uint8, device=dev)
                  for _ in range(2)]
            kw = dict(tiles=tiles, grid=grid)
            out[f'{name} {str(dt)[6:]}'] = (lambda x=x, c=cv[0], kw=kw: ops.image_tiles_u8(x, out=c, **kw),
                                            lambda x=x, c=cv[1], kw=kw: ops.image_tiles_u8_ref(x, out=c, **kw),
                                            x.numel() * (x.element_size() + 1))
    return out


def window(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls * 1e3       # us per call


def summarise(path, calls):
    """The kernels of a --trace run from its kernel trace, grouped by name and grid size: the groups launched at least
    `calls` times are the traced loops (the set-up's kernels run once or twice), launches = count // calls."""
    groups = {}
    for r in csv.DictReader(open(path)):
        us = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        groups.setdefault((r['Kernel_Name'], int(r['Grid_Size_X'])), []).append(us)
    print(f'launches per call ({calls} traced calls)   median us [min, max]   grid   kernel')
    fused = other = 0
    for (name, grid), us in sorted(groups.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        if len(us) < calls:
            continue
        n = len(us) // calls
        fused, other = fused + n * ('tiles_' in name), other + n * ('tiles_' not in name)
        print(f'{n:3d} {statistics.median(us):9.2f} [{min(us):.2f}, {max(us):.2f}] {grid:9d}   {name[:150]}')
    print(f'over the 3 float32 shapes: fused {fused} launches, composition {other} launches')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=500)
    ap.add_argument('--trace', type=int, default=0, metavar='CALLS')
    ap.add_argument('--summarise', nargs=2, metavar=('CSV', 'CALLS'))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise[0], int(args.summarise[1]))
    assert torch.cuda.is_available(), 'imgout_micro measures on the GPU only'
    dev = torch.device('cuda', 0)
    ops = cases(dev)
    if args.trace:
        only = [k for k in ops if 'float32' in k]
        for name in only:
            for fn in ops[name][:2]:
                for _ in range(args.trace):
                    fn()
        torch.cuda.synchronize()
        print(f'traced {args.trace} calls of the fused op and of the composition for each of: {only}')
        return
    for name, (fused, composed, nbytes) in ops.items():
        a, b = fused(), composed()
        print(f'{name}: {int((a != b).sum())} of {a.numel()} bytes differ between fused and composition')
        window(fused, 20), window(composed, 20)
        res = {True: [], False: []}
        for r in range(args.rounds):
            for which in ((True, False) if r % 2 == 0 else (False, True)):
                res[which].append(window(fused if which else composed, args.calls))
        mf, mc = statistics.median(res[True]), statistics.median(res[False])
        print(f'{name}: us per call (device events, median of {args.rounds} windows of {args.calls}): fused {mf:.1f} '
              f'[{min(res[True]):.1f}, {max(res[True]):.1f}], composition {mc:.1f} [{min(res[False]):.1f}, '
              f'{max(res[False]):.1f}]; ratio {mc / mf:.2f}; fused {nbytes / mf / 1e6:.3f} TB/s end to end '
              f'({nbytes / 1e6:.1f} MB needed)', flush=True)


if __name__ == '__main__':
    main()
