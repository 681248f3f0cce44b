"""Shared infrastructure of the projector tests (no dependency on the reference or on a GPU).

  * the tiny generator of the fixture (tests/golden/projector_ref.npz): resolution 32, two modalities, the widths of
    the smallest parity config (make_golden.NET_CFG), float32, state by golden_init.init_state (noise strengths 0.1);
  * StandIn: a small fixed-seed network with the LPIPS detector's call signature -- forward(img, resize_images,
    return_lpips) -- that stands in for NVIDIA's vgg16.pt (which cannot be fetched): input [N, 3, H, W] in [0, 255],
    two strided convolutions, channel-normalised features of both stages, flattened;
  * project(): a pure-torch restatement of ONE projection (SG3/genlib/projector/projector.py:106-346) on any generator
    implementation -- the tests run it on the CPU oracle (oracle/sg2_oracle.py) with the fixture's tape replayed;
  * the comparison of two runs' quantities under the reference's own spread (judge).
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

CFG = dict(z_dim=32, w_dim=32, c_dim=0, img_resolution=32, img_channels=2, channel_base=128, channel_max=16, map_depth=8)
MODALITIES = ['MR_nonrigid_CT', 'MR_MR_T2']
K_STEPS = 6
W_AVG_SAMPLES = 64
RUNS = ('cold', 'warm')
FLOOR = 1e-4            # the project's f32 parity floor (config_parity.F32_FLOORS, gradients)
FACTOR = 4.0            # config_parity.judge_f32's margin on a reference spread sample


class StandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(2024)
        self.w1 = torch.nn.Parameter(torch.randn([8, 3, 3, 3], generator=g) * 0.2, requires_grad=False)
        self.b1 = torch.nn.Parameter(torch.randn([8], generator=g) * 0.1, requires_grad=False)
        self.w2 = torch.nn.Parameter(torch.randn([16, 8, 3, 3], generator=g) * 0.1, requires_grad=False)
        self.b2 = torch.nn.Parameter(torch.randn([16], generator=g) * 0.1, requires_grad=False)

    def forward(self, img, resize_images: bool = False, return_lpips: bool = False):
        if not return_lpips:
            raise RuntimeError('StandIn serves return_lpips=True only')
        x = img / 127.5 - 1.0
        if resize_images:
            x = F.interpolate(x, size=[32, 32], mode='bilinear', align_corners=False)
        a = F.leaky_relu(F.conv2d(x, self.w1, self.b1, stride=2, padding=1), 0.2)
        b = F.leaky_relu(F.conv2d(a, self.w2, self.b2, stride=2, padding=1), 0.2)
        fa = a / (a.square().sum(dim=1, keepdim=True) + 1e-8).sqrt() / float(a.shape[2] * a.shape[3]) ** 0.5
        fb = b / (b.square().sum(dim=1, keepdim=True) + 1e-8).sqrt() / float(b.shape[2] * b.shape[3]) ** 0.5
        return torch.cat([fa.flatten(1), fb.flatten(1)], dim=1)


def stand_in(state=None):
    m = StandIn().eval()
    if state is not None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return m


def build_generator(mod, state=None, num_fp16_res=0, **extra):
    """The fixture's generator from module `mod` (the product's or the oracle's networks); state: {name: array}."""
    from golden_init import init_state
    G = mod.Generator(z_dim=CFG['z_dim'], c_dim=CFG['c_dim'], w_dim=CFG['w_dim'], img_resolution=CFG['img_resolution'],
                      img_channels=CFG['img_channels'], channel_base=CFG['channel_base'], channel_max=CFG['channel_max'],
                      num_fp16_res=num_fp16_res, conv_clamp=256, mapping_kwargs=dict(num_layers=CFG['map_depth']),
                      **extra).eval().requires_grad_(False)
    if state is None:
        init_state(G, seed=1)
    else:
        own = G.state_dict()
        assert set(state) == set(own), sorted(set(state) ^ set(own))
        with torch.no_grad():
            for k, v in own.items():
                v.copy_(torch.from_numpy(np.asarray(state[k])).to(v.dtype))
    return G


def make_target(seed=77):
    """[1, 2, 32, 32] float32 in [0, 255]: smooth blobs plus noise."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:32, 0:32] / 31.0
    img = np.stack([128 + 100 * np.sin(3 * xx + c) * np.cos(2 * yy - c) + 10 * r.randn(32, 32) for c in range(2)])
    return np.clip(img, 0, 255).astype(np.float32)[None]


def nudge(t, rel, gen):
    u = torch.randint(0, 2, t.shape, generator=gen).to(t.dtype) * 2 - 1
    return t * (1 + rel * u)


def noise_names(G):
    return [n for n, _ in G.synthesis.named_buffers() if 'noise_const' in n]


def _split(img, modalities):
    if img.shape[1] == 1:
        return {modalities[0]: img.repeat([1, 3, 1, 1])}
    if img.shape[1] == 3:
        return {modalities[0]: img}
    return {m: img[:, i:i + 1].repeat([1, 3, 1, 1]) for i, m in enumerate(modalities)}


def project(G, detector, target, num_steps, w_init=None, modalities=MODALITIES, w_avg_samples=W_AVG_SAMPLES, w_lpips=1.0,
            w_pix=1e-4, lr0=0.1, noise0=0.05, rampdown=0.25, rampup=0.05, noise_ramp=0.75, reg_weight=1e5):
    """One projection without early stopping; random draws come from torch.randn_like (replay a tape around the
    call).  -> the quantities of the fixture (numpy): w_avg, w_std, lr[K], w_noise_scale[K], loss terms [K] each,
    w_out [K, C], grad0/w, grad0/noise/<i>, noise/<i>, best_step."""
    G = copy.deepcopy(G).eval().requires_grad_(False)
    real = next(G.parameters()).dtype
    target = target.to(real)
    if w_init is not None:
        w_avg = w_init[None, :1, :]
        w_std = torch.std(w_avg).item()
        w_avg = w_avg.numpy()
    else:
        z = np.random.RandomState(123).randn(w_avg_samples, G.z_dim)
        w = G.mapping(torch.from_numpy(z), None)[:, :1, :].numpy().astype(np.float32)
        w_avg = np.mean(w, axis=0, keepdims=True)
        w_std = (np.sum((w - w_avg) ** 2) / w_avg_samples) ** 0.5
    names = noise_names(G)
    bufs = [G.synthesis.get_buffer(n) for n in names]
    tmod = _split(target, modalities)
    with torch.no_grad():
        tfeat = {m: detector(tmod[m].clone(), resize_images=False, return_lpips=True) for m in modalities}
    w_opt = torch.tensor(w_avg, dtype=torch.float32).to(real).requires_grad_(True)
    opt = torch.optim.Adam([w_opt] + bufs, betas=(0.9, 0.999), lr=lr0)
    for b in bufs:
        b[:] = torch.randn_like(b)
        b.requires_grad = True
    out = {'w_avg': np.asarray(w_avg, np.float64), 'w_std': np.float64(w_std)}
    rows = {k: [] for k in ['lr', 'w_noise_scale', 'reg_loss', 'tot_loss'] +
            [f'{m}_{t}_loss' for m in modalities for t in ('lpips', 'pix')]}
    w_out = []
    for step in range(num_steps):
        t = step / num_steps
        scale = w_std * noise0 * max(0.0, 1.0 - t / noise_ramp) ** 2
        ramp = min(1.0, (1.0 - t) / rampdown)
        ramp = 0.5 - 0.5 * np.cos(ramp * np.pi)
        lr = lr0 * ramp * min(1.0, t / rampup)
        for g in opt.param_groups:
            g['lr'] = lr
        ws = (w_opt + torch.randn_like(w_opt) * scale).repeat([1, G.mapping.num_ws, 1])
        synth = (G.synthesis(ws, noise_mode='const') + 1) * (255 / 2)
        smod = _split(synth, modalities)
        loss_terms = {}
        for m in modalities:
            loss_terms[f'{m}_pix_loss'] = w_pix * torch.mean((tmod[m] - smod[m]) ** 2)
            feat = detector(smod[m].clone(), resize_images=False, return_lpips=True)
            loss_terms[f'{m}_lpips_loss'] = w_lpips * (tfeat[m] - feat).square().sum()
        reg = 0.0
        for b in bufs:
            n = b[None, None]
            while True:
                reg = reg + (n * n.roll(1, 3)).mean() ** 2 + (n * n.roll(1, 2)).mean() ** 2
                if n.shape[2] <= 8:
                    break
                n = F.avg_pool2d(n, 2)
        loss = reg * reg_weight
        for m in modalities:
            loss = loss + loss_terms[f'{m}_lpips_loss'] + loss_terms[f'{m}_pix_loss']
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 0:
            out['grad0/w'] = w_opt.grad.numpy().astype(np.float64)
            for i, b in enumerate(bufs):
                out[f'grad0/noise/{i}'] = b.grad.numpy().astype(np.float64)
        opt.step()
        rows['lr'].append(lr)
        rows['w_noise_scale'].append(scale)
        rows['reg_loss'].append(reg.item() * reg_weight)
        rows['tot_loss'].append(loss.item())
        for k, v in loss_terms.items():
            rows[k].append(v.item())
        w_out.append(w_opt.detach()[0, 0].numpy().astype(np.float64))
        with torch.no_grad():
            for b in bufs:
                b -= b.mean()
                b *= b.square().mean().rsqrt()
    out.update({k: np.asarray(v, np.float64) for k, v in rows.items()})
    out['w_out'] = np.stack(w_out)
    for i, b in enumerate(bufs):
        out[f'noise/{i}'] = b.detach().numpy().astype(np.float64)
    out['best_step'] = np.int64(int(np.argmin(rows['tot_loss'])))
    return out


# ---- the fixture ----

JUDGED = ('reg_loss', 'tot_loss', 'w_out_last', 'grad0/w') + tuple(f'{m}_{t}_loss' for m in MODALITIES
                                                                   for t in ('lpips', 'pix'))


def load_fixture(path):
    with np.load(path, allow_pickle=False) as z:
        z = {k: z[k] for k in z.files}
    fix = {'G': {k[2:]: v for k, v in z.items() if k.startswith('G/')},
           'det': {k[4:]: v for k, v in z.items() if k.startswith('det/')}, 'target': z['target']}
    for run in RUNS:
        from rngtape import Tape
        fix[run] = {k[len(run) + 1:]: v for k, v in z.items() if k.startswith(run + '/') and '/tape' not in k
                    and not k.startswith(run + '/r32_')}
        fix[run]['tape'] = Tape.from_npz({k[len(run) + 1:]: v for k, v in z.items() if k.startswith(run + '/tape')}, 'tape')
        names = sorted({k.split('/')[1] for k in z if k.startswith(run + '/r32_')})
        fix[run]['spread'] = {n: {k[len(run) + len(n) + 2:]: v for k, v in z.items() if k.startswith(f'{run}/{n}/')}
                              for n in names}
    return fix


def rel(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def quantities(run):
    """The judged quantities of a run's dict (project()'s, the fixture's or the product's)."""
    q = {k: run[k] for k in run if k in JUDGED or k.startswith('grad0/noise/')}
    q['w_out_last'] = np.asarray(run['w_out'])[-1]
    return q


def bounds(ref_run):
    """{quantity: max(FLOOR, FACTOR x the reference's own f32 spread on it)}: the spread is the largest relative L2
    distance of a re-evaluation of the reference (one thread; states nudged by half an ulp) from the reference run."""
    base = quantities(ref_run)
    out = {}
    for k, v in base.items():
        r = max([rel(quantities(s)[k], v) for s in ref_run['spread'].values()], default=0.0)
        out[k] = (max(FLOOR, FACTOR * r), r)
    return out


def judge(got, ref_run, what, grads_tight=False, check=True):
    """Every judged quantity of `got` within its bound of the reference run; grads_tight: the step-0 gradients held
    to FLOOR itself.  Prints each figure; -> {quantity: (error, bound)}."""
    base, bnd, res, bad = quantities(ref_run), bounds(ref_run), {}, []
    gq = quantities(got)
    for k in sorted(base):
        b = FLOOR if grads_tight and k.startswith('grad0/') else bnd[k][0]
        e = rel(gq[k], base[k])
        res[k] = (e, b)
        print(f'{what} {k}: rel L2 {e:.3g} (bound {b:.3g}, reference spread {bnd[k][1]:.3g})')
        if not e <= b:
            bad.append(f'{k}: {e:.3g} > {b:.3g}')
    assert not check or not bad, f'{what}: ' + '; '.join(bad)
    return res
