"""ms per latent-projection step and slices x steps / s: forward (batch 1, the baseline) against forward_batch at
B in {1, 2, 4, 8, 16}, fused and SG2_PROJ_FUSED=0.

    python tools/bench_projector.py [--steps 30] [--warmup 10] [--rounds 3] [--batches 1,2,4,8,16]

Generator: the benchmark's configuration at 256^2 with one image channel (cbase 16384, cmax 512, z = w = 512, mapping
depth 8, num_fp16_res 4), random weights, noise strengths 0.1.  Detector: a VGG16-SHAPED STAND-IN with random weights
and the LPIPS call signature (13 3x3 convolutions, five taps, channel-normalised, 7,995,392 features per 256^2 image)
-- NVIDIA's vgg16.pt cannot be fetched; the stand-in costs what a VGG16 of that shape costs in torch, but it is not
the LPIPS network, and the output says so.

Timing: the optimisation loop of a projection is replaced by one that runs `warmup` untimed steps and then `steps`
timed ones, each timed by the host clock around a step that ends in a device synchronise (no early stopping, no
output files).  A round runs every configuration once; the order of the configurations alternates from round to
round; one untimed round goes first.  Reported per configuration: the median over rounds of the round's median
ms / step, with [min, max] of the round medians as the spread, and slices x steps / s = B / (ms / step).
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

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MODALITIES = ['CT']
VGG16 = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]
TAPS = (1, 3, 6, 9, 12)         # the convolutions whose ReLU output LPIPS reads (relu1_2 ... relu5_3)


class VggShapedStandIn(torch.nn.Module):
    """VGG16's convolution stack with random weights; forward(img [N, 3, H, W] in [0, 255], resize_images,
    return_lpips) -> the five taps, channel-normalised and scaled by 1 / sqrt(H W), flattened and concatenated."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(16)
        self.convs = torch.nn.ModuleList()
        cin = 3
        for c in VGG16:
            if c == 'M':
                continue
            conv = torch.nn.Conv2d(cin, c, 3, padding=1)
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
                conv.bias.zero_()
            self.convs.append(conv)
            cin = c
        self.requires_grad_(False)

    def forward(self, img, resize_images=False, return_lpips=False):
        if not return_lpips:
            raise RuntimeError('the stand-in serves return_lpips=True only')
        x = img / 127.5 - 1.0
        if resize_images:
            x = F.interpolate(x, size=[224, 224], mode='bilinear', align_corners=False)
        feats, i = [], 0
        for c in VGG16:
            if c == 'M':
                x = F.max_pool2d(x, 2)
                continue
            x = F.relu(self.convs[i](x))
            if i in TAPS:
                n = x / (x.square().sum(dim=1, keepdim=True) + 1e-10).sqrt() / float(x.shape[2] * x.shape[3]) ** 0.5
                feats.append(n.flatten(1))
            i += 1
        return torch.cat(feats, dim=1)


def build(dev):
    from training import networks_stylegan2 as net
    torch.manual_seed(0)
    G = net.Generator(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=1, channel_base=16384,
                      channel_max=512, num_fp16_res=4, conv_clamp=256, mapping_kwargs=dict(num_layers=8))
    with torch.no_grad():
        for n, p in G.named_parameters():
            if n.endswith('noise_strength'):
                p.fill_(0.1)
    return G.eval().requires_grad_(False).to(dev)


class StepTimer:
    """Stands in for projector.optimise / optimise_batch: `warmup` untimed steps, then `steps` timed ones."""

    def __init__(self, warmup, steps):
        self.warmup, self.steps, self.times = warmup, steps, []

    def _run(self, step_fn):
        out = None
        for step in range(self.warmup + self.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = step_fn(step)
            torch.cuda.synchronize()
            if step >= self.warmup:
                self.times.append((time.perf_counter() - t0) * 1e3)
        return out

    def optimise(self, num_steps, early_stopping, step_fn):
        return 0, float(self._run(step_fn))

    def optimise_batch(self, num_steps, early_stopping, step_fn):
        losses = self._run(step_fn)
        return [0] * len(losses), list(losses), [num_steps - 1] * len(losses)


def measure(p, pj, config, targets, warmup, steps):
    """The median ms / step of one projection call of a configuration (kind, B, fused)."""
    kind, B, fused = config
    os.environ['SG2_PROJ_FUSED'] = '1' if fused else '0'
    timer = StepTimer(warmup, steps)
    saved = pj.optimise, pj.optimise_batch
    pj.optimise, pj.optimise_batch = timer.optimise, timer.optimise_batch
    try:
        if kind == 'forward':
            p.forward('p', 0, targets[:1], num_steps=warmup + steps, early_stopping=10 ** 9, verbose_logger=False)
        else:
            p.forward_batch([('p', b) for b in range(B)], targets[:B], num_steps=warmup + steps, early_stopping=10 ** 9,
                            verbose_logger=False)
    finally:
        pj.optimise, pj.optimise_batch = saved
    assert len(timer.times) == steps
    return statistics.median(timer.times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=str, default='1,2,4,8,16')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_projector measures on the GPU only'
    from genlib.projector import projector as pj
    from metrics import metric_utils
    dev = torch.device('cuda', 0)
    batches = [int(b) for b in args.batches.split(',')]
    metric_utils.register_detector(pj.LPIPS_URL, VggShapedStandIn().to(dev))
    print('detector: a VGG16-shaped STAND-IN with random weights (not the LPIPS network; vgg16.pt is not available)')
    print(f'device: {torch.cuda.get_device_name(0)}; generator 256^2, 1 channel, cbase 16384, fp16 top blocks')
    G = build(dev)
    p = pj.StyleGAN2Projector(outdir=os.devnull, device=dev, modalities=MODALITIES, dtype='float32', outdir_model=None,
                              w_avg_samples=64, save_final_projection=False, G=G)
    targets = torch.from_numpy(np.random.RandomState(0).uniform(0, 255, [max(batches), 1, 256, 256]).astype(np.float32))
    configs = [('forward', 1, True), ('forward', 1, False)] + [('forward_batch', b, f) for b in batches for f in (True, False)]
    for c in configs:                   # untimed: code objects, allocator, algorithm choices of every shape
        measure(p, pj, c, targets, 2, 3)
    res = {c: [] for c in configs}
    for r in range(args.rounds):
        for c in (configs if r % 2 == 0 else configs[::-1]):
            res[c].append(measure(p, pj, c, targets, args.warmup, args.steps))
        print(f'round {r} done', flush=True)
    base = statistics.median(res[('forward', 1, True)])
    rows = []
    print(f'\n{"configuration":<34s} {"ms/step (median [min, max])":<32s} {"slices x steps / s":>18s} {"per slice vs forward":>21s}')
    for c in configs:
        kind, B, fused = c
        med = statistics.median(res[c])
        name = f'{kind} B={B} ' + ('fused' if fused else 'SG2_PROJ_FUSED=0')
        rate = B / med * 1e3
        print(f'{name:<34s} {f"{med:.2f} [{min(res[c]):.2f}, {max(res[c]):.2f}]":<32s} {rate:>18.1f} {base / (med / B):>20.2f}x')
        rows.append(dict(kind=kind, batch=B, fused=fused, ms_per_step=med, ms_min=min(res[c]), ms_max=max(res[c]),
                         slices_steps_per_s=rate))
    print(json.dumps(dict(tool='bench_projector', detector='vgg16-shaped stand-in (random weights)', steps=args.steps,
                          warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == '__main__':
    main()
