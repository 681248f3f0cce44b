"""Perceptual path length (Karras et al. 2019), per modality: SG3/metrics/perceptual_path_length.py, arithmetic
restated.

One sampler call draws B latent pairs, interpolates each at t and at t + epsilon (linearly in W, spherically in Z),
renders the 2B images in float32 with freshly drawn constant noise, and divides the squared LPIPS distance of every
pair by epsilon^2.  The metric is the mean of those values between their 1st and 99th percentile.

The fused path (the default on ROCm; SG2_PPL_FUSED=0 selects the reference's composition) keeps all noise buffers
of the private generator copy in one flat float32 tensor refilled by ONE torch.randn, builds the detector's input in
one HIP pass (sg2_ppl_prep) and the pair distances in one read of the LPIPS features (sg2_lpips_pair_dist):
torch_utils/ops/ppl.py.  The two paths draw differently (the composition draws `rand`, `randn`, then one
`randn_like` per buffer, as the reference does); PPLSampler.forward(draws=...) runs either path on given draws.

Differences from the reference by design:
  * per modality: with `mode_dict`, channel `mode_idx` of the generated image is the image, repeated to three
    channels (metric_utils._select_mode's rule); the reference's sampler cannot run on a 2-channel generator;
  * the VGG16 network is supplied offline (SG2_PR_DETECTOR or metric_utils.register_detector), never downloaded;
  * ranks exchange their distances with one all_gather after the loop, not one broadcast per rank and call;
  * on ROCm the images are rendered in the kernels' deterministic mode (sg2hip.deterministic), so the same seed
    gives the same value.
"""
import contextlib
import copy
import os

import numpy as np
import torch

import sg2hip as _hip
from torch_utils.ops import noise_reg
from torch_utils.ops import ppl as ppl_ops
from . import metric_utils
from . import precision_recall

DETECTOR_URL = precision_recall.DETECTOR_URL        # .../metrics/vgg16.pkl: the network pr50k3 uses


def fused_default():
    return os.environ.get('SG2_PPL_FUSED', '1') != '0'


def slerp(a, b, t):
    """Spherical interpolation of batches of vectors [B, D] at t [B, 1]; the result has unit length."""
    a = a / a.norm(dim=-1, keepdim=True)
    b = b / b.norm(dim=-1, keepdim=True)
    cos_ab = (a * b).sum(dim=-1, keepdim=True)
    angle = t * torch.acos(cos_ab)
    ortho = b - cos_ab * a
    ortho = ortho / ortho.norm(dim=-1, keepdim=True)
    out = a * torch.cos(angle) + ortho * torch.sin(angle)
    return out / out.norm(dim=-1, keepdim=True)


def lpips_features(detector, img):
    try:
        return detector(img, resize_images=False, return_lpips=True)
    except (RuntimeError, TypeError) as err:
        names = ' / '.join(metric_utils.detector_env_vars(DETECTOR_URL))
        raise RuntimeError(f'the VGG16 detector refused (img, resize_images=False, return_lpips=True): {names} must '
                           f'name NVIDIA\'s scripted VGG16 with the LPIPS head, or a module with that signature must be '
                           f'registered with metrics.metric_utils.register_detector ({err})') from err


class PPLSampler(torch.nn.Module):
    def __init__(self, G, G_kwargs, epsilon, space, sampling, crop, vgg16, mode_dict=None):
        assert space in ['z', 'w']
        assert sampling in ['full', 'end']
        super().__init__()
        self.G = copy.deepcopy(G)
        self.G_kwargs = G_kwargs
        self.epsilon = epsilon
        self.space = space
        self.sampling = sampling
        self.crop = crop
        self.vgg16 = copy.deepcopy(vgg16)
        self.mode_dict = mode_dict
        self.__dict__['_flat'] = None       # (flat noise tensor, table, views): built on the first fused call
        self.__dict__['last_fused'] = None

    def _noise_owners(self):
        names = [name for name, _ in self.G.named_buffers() if name.endswith('.noise_const')]
        return [self.G.get_submodule(name.rsplit('.', 1)[0]) for name in names]

    def _flat_noise(self, owners, device):
        """All noise buffers as views of one flat tensor (None if the layout is not one noise_reg takes)."""
        shapes = [tuple(o._buffers['noise_const'].shape) for o in owners]
        if not owners or any(len(s) != 2 or s[0] != s[1] for s in shapes):
            return None
        table, total = noise_reg.make_table(0, [s[0] for s in shapes])
        if not noise_reg.supported(table):
            return None
        state = self._flat
        if state is None or state[0].device != device or state[1] != table or \
                any(o._buffers['noise_const'] is not v for o, v in zip(owners, state[2])):
            flat = torch.empty([total], dtype=torch.float32, device=device)
            _, views = noise_reg.unflatten(flat, table, head=0)
            for o, v in zip(owners, views):
                v.copy_(o._buffers['noise_const'])
                o._buffers['noise_const'] = v
            state = self.__dict__['_flat'] = (flat, table, views)
        return state

    def _channel(self, channels):
        if self.mode_dict is not None:
            return int(self.mode_dict['mode_idx'])
        if channels not in (1, 3):
            raise RuntimeError(f'the perceptual path length of a {channels}-channel generator is taken per modality: '
                               f'pass mode_dict (mode_name, mode_idx) to name the channel')
        return None

    @torch.no_grad()
    def forward(self, c, draws=None, return_draws=False):
        """c [B, c_dim] -> dist [B].  draws = (t [B], z [2B, z_dim], [one tensor per noise_const buffer, in
        named_buffers order]) takes the place of the sampler's own draws; return_draws: -> (dist, draws used)."""
        batch, dev = c.shape[0], c.device
        owners = self._noise_owners()
        fused = fused_default() and dev.type == 'cuda'
        flat = self._flat_noise(owners, dev) if fused else None
        fused = fused and flat is not None
        self.__dict__['last_fused'] = fused

        # the draws: interpolation points, latent pairs, noise
        if draws is None:
            t = torch.rand([batch], device=dev)
            z = torch.randn([batch * 2, self.G.z_dim], device=dev)
            if fused:
                torch.randn(flat[0].shape, out=flat[0])
            else:
                for o in owners:
                    buf = o._buffers['noise_const']
                    buf.copy_(torch.randn_like(buf))
        else:
            t, z, noise = draws
            t, z = t.to(dev), z.to(dev)
            assert len(noise) == len(owners), 'one noise draw per noise_const buffer'
            for o, n in zip(owners, noise):
                o._buffers['noise_const'].copy_(n)
        if return_draws:
            used = (t.clone(), z.clone(), [o._buffers['noise_const'].clone() for o in owners])
        t = t * (1 if self.sampling == 'full' else 0)
        z0, z1 = z.chunk(2)
        cc = torch.cat([c, c])

        if self.space == 'w':       # (torch.lerp as the reference: at epsilon = 1e-4 the formula matters)
            w0, w1 = self.G.mapping(z=torch.cat([z0, z1]), c=cc).chunk(2)
            wt0 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2))
            wt1 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2) + self.epsilon)
        else:
            zt0 = slerp(z0, z1, t.unsqueeze(1))
            zt1 = slerp(z0, z1, t.unsqueeze(1) + self.epsilon)
            wt0, wt1 = self.G.mapping(z=torch.cat([zt0, zt1]), c=cc).chunk(2)

        # (on ROCm in the kernels' fixed-order reductions: at epsilon = 1e-4 a float atomic's arrival order in a
        # split-K convolution would show in the fourth digit of a distance, and the metric would not repeat)
        with _hip.deterministic(device=dev) if dev.type == 'cuda' else contextlib.nullcontext():
            img = self.G.synthesis(ws=torch.cat([wt0, wt1]), noise_mode='const', force_fp32=True, **self.G_kwargs)
        channel = self._channel(img.shape[1])
        factor = self.G.img_resolution // 256       # (0 and 1: no down-sampling)
        if fused:
            img = ppl_ops.prep_images(img.float(), channel=channel, crop=self.crop, factor=factor)
            dist = ppl_ops.pair_distances(lpips_features(self.vgg16, img).float(), self.epsilon)
        else:
            img = ppl_ops.prep_images_ref(img, channel=channel, crop=self.crop, factor=factor)
            dist = ppl_ops.pair_distances_ref(lpips_features(self.vgg16, img), self.epsilon)
        return (dist, used) if return_draws else dist


def ppl_from_distances(dist):
    """Mean of the values between the 1st percentile (taken downwards) and the 99th (taken upwards), ends included."""
    dist = np.asarray(dist)
    try:
        lo, hi = np.percentile(dist, 1, method='lower'), np.percentile(dist, 99, method='higher')
    except TypeError:       # numpy < 1.22
        lo, hi = np.percentile(dist, 1, interpolation='lower'), np.percentile(dist, 99, interpolation='higher')
    return float(np.extract(np.logical_and(dist >= lo, dist <= hi), dist).mean())


def gather_distances(local, num_samples, num_gpus):
    """local [iters, B], this rank's distances -> [num_samples] in the reference's order: call by call, within a
    call rank by rank, within a rank the batch (the order its per-call broadcasts append in)."""
    if num_gpus > 1:
        parts = [torch.empty_like(local) for _ in range(num_gpus)]
        torch.distributed.all_gather(parts, local.contiguous())
        local = torch.stack(parts, dim=1)
    return local.reshape(-1)[:num_samples]


def compute_ppl(opts, num_samples, epsilon, space, sampling, crop, batch_size, draws_out=None):
    """The reference's signature and return value (nan on ranks other than 0).  draws_out: a list that receives
    (c, draws, dist) of every sampler call of this rank."""
    vgg16 = metric_utils.get_feature_detector(DETECTOR_URL, device=opts.device, num_gpus=opts.num_gpus, rank=opts.rank,
                                              verbose=opts.progress.verbose)
    sampler = PPLSampler(G=opts.G, G_kwargs=opts.G_kwargs, epsilon=epsilon, space=space, sampling=sampling, crop=crop,
                         vgg16=vgg16, mode_dict=opts.mode_dict)
    sampler.eval().requires_grad_(False).to(opts.device)
    c_iter = metric_utils.iterate_random_labels(opts=opts, batch_size=batch_size)

    per_call = batch_size * opts.num_gpus
    calls = (num_samples + per_call - 1) // per_call
    progress = opts.progress.sub(tag='ppl sampling', num_items=num_samples)
    dist = []
    for i in range(calls):
        progress.update(i * per_call)
        c = next(c_iter)
        if draws_out is None:
            dist.append(sampler(c))
        else:
            d, draws = sampler(c, return_draws=True)
            draws_out.append((c, draws, d))
            dist.append(d)
    progress.update(num_samples)
    dist = gather_distances(torch.stack(dist), num_samples, opts.num_gpus)
    if opts.rank != 0:
        return float('nan')
    return ppl_from_distances(dist.cpu().numpy())
