"""Times of the two perceptual-path-length ops against their torch compositions, and of one sampler call fused
against composed, at the workload's shapes.

    python tools/ppl_micro.py                        # alternating windows in one process
    python tools/ppl_micro.py --trace 50             # 50 calls of each op and composition, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ppl_micro.py --trace 50
    python tools/ppl_micro.py --summarise OUT/..._kernel_stats.csv 50     # kernel time, bytes/s and share of HBM peak

Shapes: prep_images on [4, 1, 256, 256] (factor 1) and [4, 1, 1024, 1024] (factor 4), the generator's output for
B = 2 at 256^2 and 1024^2; pair_distances on [4, 7,995,392], the VGG16 LPIPS features of four 256^2 images (derived
from the architecture: 64*256^2 + 128*128^2 + 256*64^2 + 512*32^2 + 512*16^2).  Bytes are what the algorithm needs:
every input read once, every output written once.  The sampler: the 256^2 two-modality generator of the benchmark's
widths (tools/projector_micro.py's), B = 2, the tests' stand-in detector (projector_oracle.StandIn) -- NOT a VGG16, so
the whole-call figure leaves out what the real detector costs, and the time of a real ppl2_wend run is not measured.

Timing: a host clock around a window of calls that ends in a device synchronise, after an untimed warm-up of every
shape; fused and composition alternate window by window, the order swapping every round.
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'gan-track_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, the spec figure (MI355X); a float4 copy reaches about 6.3e12
F_VGG = 64 * 256 ** 2 + 128 * 128 ** 2 + 256 * 64 ** 2 + 512 * 32 ** 2 + 512 * 16 ** 2


def cases(dev):
    """name -> (fused callable, composed callable, bytes the algorithm needs)"""
    from torch_utils.ops import ppl as ops
    g = torch.Generator(device=dev).manual_seed(0)
    x256 = torch.rand([4, 1, 256, 256], device=dev, generator=g) * 2 - 1
    x1024 = torch.rand([4, 1, 1024, 1024], device=dev, generator=g) * 2 - 1
    feats = torch.randn([4, F_VGG], device=dev, generator=g)
    feats[2:] = feats[:2] * (1 + 1e-4 * torch.randn([2, F_VGG], device=dev, generator=g))
    return {
        'prep 4x1x256^2 f1': (lambda: ops.prep_images(x256, None, False, 1), lambda: ops.prep_images_ref(x256, None, False, 1),
                              4 * 256 * 256 * 4 * (1 + 3)),
        'prep 4x1x1024^2 f4': (lambda: ops.prep_images(x1024, None, False, 4), lambda: ops.prep_images_ref(x1024, None, False, 4),
                               4 * 1024 * 1024 * 4 + 4 * 3 * 256 * 256 * 4),
        'pair_dist B=2 F=7995392': (lambda: ops.pair_distances(feats, 1e-4), lambda: ops.pair_distances_ref(feats, 1e-4),
                                    4 * F_VGG * 4),
    }


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def build_sampler(dev):
    import projector_micro as pm
    import projector_oracle as po
    from metrics import perceptual_path_length as ppl
    G = pm.build(dev)
    s = ppl.PPLSampler(G, {}, 1e-4, 'w', 'end', False, po.stand_in(), mode_dict={'mode_name': 'm0', 'mode_idx': 0})
    return s.eval().requires_grad_(False).to(dev)


def summarise(path, calls):
    rows = list(csv.DictReader(open(path)))
    b = {'prep256': 4 * 256 * 256 * 4 * 4, 'prep1024': 4 * 1024 * 1024 * 4 + 4 * 3 * 256 * 256 * 4, 'dist': 4 * F_VGG * 4}
    print('  calls   avg us  name')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        print(f"{int(r['Calls']):7d} {float(r['TotalDurationNs']) / int(r['Calls']) / 1e3:8.2f}  {r['Name'][:150]}")
    by = {r['Name']: r for r in rows}

    def avg(sub):
        hit = [r for n, r in by.items() if sub in n]
        return sum(float(r['TotalDurationNs']) for r in hit) / calls / 1e3 if hit else None

    part, final = avg('ppl_dist_partial_kernel'), avg('ppl_dist_final_kernel')
    if part is not None:
        us = part + (final or 0)
        print(f'sg2_lpips_pair_dist: {us:.2f} us of kernel time per call (stage 1 {part:.2f}, stage 2 {final or 0:.2f}); '
              f'{b["dist"] / us / 1e6:.3f} TB/s = {b["dist"] / us * 1e6 / HBM_PEAK:.1%} of the 8 TB/s HBM peak')
    for fac, key in ((1, 'prep256'), (4, 'prep1024')):
        us = avg(f'ppl_prep_kernel<{fac}>')
        if us is not None:
            print(f'sg2_ppl_prep factor {fac}: {us:.2f} us of kernel time per call; {b[key] / us / 1e6:.3f} TB/s = '
                  f'{b[key] / us * 1e6 / HBM_PEAK:.1%} of the 8 TB/s HBM peak')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--sampler-calls', type=int, default=100)
    ap.add_argument('--trace', type=int, default=0, metavar='CALLS')
    ap.add_argument('--summarise', nargs=2, metavar=('CSV', 'CALLS'))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise[0], int(args.summarise[1]))
    assert torch.cuda.is_available(), 'ppl_micro measures on the GPU only'
    dev = torch.device('cuda', 0)
    ops = cases(dev)
    if args.trace:
        for name, (fused, composed, _) in ops.items():
            for fn in (fused, composed):
                for _ in range(args.trace):
                    fn()
        torch.cuda.synchronize()
        print(f'traced {args.trace} calls of every op and composition')
        return
    for name, (fused, composed, nbytes) in ops.items():
        a, b = fused(), composed()
        print(f'{name}: fused against composition max |diff| {float((a - b).abs().max()):.3g}, max |value| '
              f'{float(b.abs().max()):.3g}')
        window(fused, 20), window(composed, 20)
        res = {True: [], False: []}
        for r in range(args.rounds):
            for which in ((True, False) if r % 2 == 0 else (False, True)):
                res[which].append(window(fused if which else composed, args.calls))
        mf, mc = statistics.median(res[True]), statistics.median(res[False])
        print(f'{name}: us per call (host clock, median of {args.rounds} windows of {args.calls}): fused {mf:.1f} '
              f'[{min(res[True]):.1f}, {max(res[True]):.1f}], composition {mc:.1f} [{min(res[False]):.1f}, '
              f'{max(res[False]):.1f}]; fused {nbytes / mf / 1e6:.3f} TB/s end to end', flush=True)
    s = build_sampler(dev)
    c = torch.zeros([2, 0], device=dev)
    res = {True: [], False: []}
    for which in (True, False):
        os.environ['SG2_PPL_FUSED'] = '1' if which else '0'
        window(lambda: s(c), 10)
    for r in range(args.rounds):
        for which in ((True, False) if r % 2 == 0 else (False, True)):
            os.environ['SG2_PPL_FUSED'] = '1' if which else '0'
            res[which].append(window(lambda: s(c), args.sampler_calls) / 1e3)
            assert s.last_fused == which
    print(f'one sampler call, 256^2, B = 2, stand-in detector (ms, median of {args.rounds} windows of '
          f'{args.sampler_calls}): SG2_PPL_FUSED=1 {statistics.median(res[True]):.3f} [{min(res[True]):.3f}, '
          f'{max(res[True]):.3f}], SG2_PPL_FUSED=0 {statistics.median(res[False]):.3f} [{min(res[False]):.3f}, '
          f'{max(res[False]):.3f}]')


if __name__ == '__main__':
    main()
