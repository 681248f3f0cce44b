"""ms per latent-projection step at the Pelvis shape, fused noise step against the reference's composition.

    python tools/projector_micro.py                    # alternating SG2_PROJ_FUSED=0 / 1 rounds in one process
    python tools/projector_micro.py --trace N          # N steps of the setting in SG2_PROJ_FUSED, for a kernel trace:
    SG2_PROJ_FUSED=1 rocprofv3 --kernel-trace --stats -d OUT -- python tools/projector_micro.py --trace 50
    python tools/projector_micro.py --summarise OUT/..._kernel_stats.csv 50      # launches per step from that trace

Shape: 256^2, two modalities, the benchmark's channel widths (cbase 16384, cmax 512, z = w = 512, mapping depth 8,
num_fp16_res 4), batch 1, 13 noise buffers (4 .. 256).  Detector: the file SG2_LPIPS_DETECTOR / SG2_PR_DETECTOR names,
else the tests' small stand-in (tests/projector_oracle.StandIn) -- the output says which; with the stand-in the LPIPS
network's share of a step is NOT what a real VGG16 costs, so the whole-step figures understate the step and overstate
the relative gain; the part timing does not depend on the detector.

Timing (host clock around work that ends in a device synchronise): a projection of n steps costs setup + n x step, so
ms/step = (T(n2) - T(n1)) / (n2 - n1) from two forward() calls; each round times both settings, the order alternating,
after one untimed round.  The part timing runs regulariser + backward + Adam + renormalise alone on the same flat
buffer / the same list of tensors.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODALITIES = ['MR_nonrigid_CT', 'MR_MR_T2']


def build(dev):
    from training import networks_stylegan2 as net
    torch.manual_seed(0)
    G = net.Generator(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=2, channel_base=16384,
                      channel_max=512, num_fp16_res=4, conv_clamp=256, mapping_kwargs=dict(num_layers=8))
    with torch.no_grad():
        for n, p in G.named_parameters():
            if n.endswith('noise_strength'):
                p.fill_(0.1)
    return G.eval().requires_grad_(False).to(dev)


def detector():
    from genlib.projector import projector as pj
    from metrics import metric_utils
    named = [v for v in metric_utils.detector_env_vars(pj.LPIPS_URL) if os.environ.get(v)]
    if named:
        return f'{named[0]}={os.environ[named[0]]}'
    import projector_oracle as po
    metric_utils.register_detector(pj.LPIPS_URL, po.stand_in())
    return 'stand-in (tests/projector_oracle.StandIn): no LPIPS detector file named'


def make_projector(G, dev):
    from genlib.projector import projector as pj
    return pj.StyleGAN2Projector(outdir=os.devnull, device=dev, modalities=MODALITIES, dtype='float32', outdir_model=None,
                                 w_avg_samples=64, save_final_projection=False, G=G)


def timed_forward(p, target, steps, fused):
    os.environ['SG2_PROJ_FUSED'] = '1' if fused else '0'
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.forward('p', 0, target, num_steps=steps, early_stopping=10 ** 9, verbose_logger=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def step_ms(p, target, fused, n1, n2):
    return (timed_forward(p, target, n2, fused) - timed_forward(p, target, n1, fused)) / (n2 - n1) * 1e3


def part_ms(dev, fused, iters):
    """regulariser + backward + Adam + renormalise alone, ms per iteration."""
    from torch_utils.ops import noise_reg
    sizes = [4] + [r for r in (8, 16, 32, 64, 128, 256) for _ in range(2)]
    table, total = noise_reg.make_table(512, sizes)
    g = torch.Generator(device=dev).manual_seed(1)
    if fused:
        from training.optim import FlatAdam
        flat = torch.randn([total], device=dev, generator=g).requires_grad_(True)
        opt = FlatAdam([flat], betas=(0.9, 0.999), lr=0.1)

        def it():
            flat.grad = None
            (noise_reg.noise_regularizer(flat, table) * 1e5).backward()
            opt.step_flat(flat.grad, [0], [0], write_grad=False)
            noise_reg.normalize_noise_(flat, table)
    else:
        w = torch.randn([1, 1, 512], device=dev, generator=g).requires_grad_(True)
        bufs = [torch.randn([r, r], device=dev, generator=g).requires_grad_(True) for r in sizes]
        opt = torch.optim.Adam([w] + bufs, betas=(0.9, 0.999), lr=0.1)

        def it():
            opt.zero_grad(set_to_none=True)
            ((noise_reg.noise_regularizer_ref(bufs) + w.sum() * 0) * 1e5).backward()
            opt.step()
            noise_reg.normalize_noise_ref_(bufs)
    for _ in range(5):
        it()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        it()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def summarise(path, steps):
    rows = list(csv.DictReader(open(path)))
    calls = sum(int(r['Calls']) for r in rows)
    total = sum(float(r['TotalDurationNs']) for r in rows) / 1e6
    print(f'{calls} kernel launches, {total:.1f} ms of kernel time over {steps} steps + setup: '
          f'{calls / steps:.0f} launches and {total / steps:.2f} ms per step (setup included)')
    print(' calls   total ms  name')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:25]:
        print(f"{int(r['Calls']):6d} {float(r['TotalDurationNs']) / 1e6:10.2f}  {r['Name'][:140]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--n1', type=int, default=20)
    ap.add_argument('--n2', type=int, default=120)
    ap.add_argument('--trace', type=int, default=0, metavar='STEPS')
    ap.add_argument('--summarise', nargs=2, metavar=('CSV', 'STEPS'))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise[0], int(args.summarise[1]))
    assert torch.cuda.is_available(), 'projector_micro measures on the GPU only'
    dev = torch.device('cuda', 0)
    print('detector:', detector())
    G = build(dev)
    p = make_projector(G, dev)
    target = torch.from_numpy(np.random.RandomState(0).uniform(0, 255, [1, 2, 256, 256]).astype(np.float32))
    if args.trace:
        fused = os.environ.get('SG2_PROJ_FUSED', '1') != '0'
        timed_forward(p, target, args.trace, fused)
        print(f'traced {args.trace} steps, SG2_PROJ_FUSED={int(fused)}')
        return
    for fused in (True, False):         # untimed: code objects, allocator, algorithm choices
        timed_forward(p, target, 10, fused)
    res = {True: [], False: []}
    parts = {True: [], False: []}
    for r in range(args.rounds):
        for fused in ((True, False) if r % 2 == 0 else (False, True)):
            res[fused].append(step_ms(p, target, fused, args.n1, args.n2))
            parts[fused].append(part_ms(dev, fused, 200))
        print(f'round {r}: step fused {res[True][-1]:.3f} ms, composition {res[False][-1]:.3f} ms; '
              f'noise part fused {parts[True][-1]:.3f} ms, composition {parts[False][-1]:.3f} ms', flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    pmed = {k: statistics.median(v) for k, v in parts.items()}
    print(f'ms per projection step (median of {args.rounds}): SG2_PROJ_FUSED=1 {med[True]:.3f} '
          f'[{min(res[True]):.3f}, {max(res[True]):.3f}], SG2_PROJ_FUSED=0 {med[False]:.3f} '
          f'[{min(res[False]):.3f}, {max(res[False]):.3f}]')
    print(f'regulariser + Adam + renormalise alone: fused {pmed[True]:.3f} ms, composition {pmed[False]:.3f} ms')


if __name__ == '__main__':
    main()
