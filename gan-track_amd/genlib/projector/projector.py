"""Projection of one image into the W space of a trained StyleGAN2-ADA generator (GAN inversion): the reference's
SG3/genlib/projector/projector.py `StyleGAN2Projector`, arithmetic restated.

One projection optimises a single w [1, 1, w_dim] (broadcast to every layer) and the generator's noise_const buffers
with Adam against   sum_modality (w_lpips LPIPS + w_pix MSE)  +  regularize_noise_weight * noise regulariser,
adds a decaying Gaussian perturbation to w, renormalises the noise buffers after every step and stops early when
the loss has not improved for `early_stopping` steps.  Returned: w of every step (repeated to num_ws) and the index
of the best step.

The fused path (the default; SG2_PROJ_FUSED=0 selects the reference's composition) keeps w and all noise buffers in
one flat float32 tensor (torch_utils/ops/noise_reg.py): the regulariser is 3 + 1 HIP launches, the Adam step one
sg2_adam_multi launch (training.optim.FlatAdam, torch.optim.Adam's arithmetic) and the renormalisation one launch,
instead of several hundred tiny launches per step.

forward_batch runs B such projections in one loop (the reference has no counterpart): all w and noise buffers of the
batch in one buffer-major flat tensor (noise_reg.make_batched_table), one synthesis and one detector pass at batch B,
per-sample loss sums (torch_utils/ops/proj_loss.py) and per-sample early stopping (optimise_batch).  forward is
untouched by it.

Differences from the reference by design:
  * the snapshot is read by this build's legacy.load_network_pkl (nothing embedded in the pickle is executed);
  * the LPIPS network is supplied offline (metrics.metric_utils: SG2_LPIPS_DETECTOR, else SG2_PR_DETECTOR, or
    register_detector) instead of being downloaded;
  * imageio is imported only when a video is asked for; `snap_video` / `snap_optimization_history` of False mean
    "never" (the reference divides by them);
  * the loss plots cover the modalities of the run (the reference hard-codes the Claro / Pelvis column names);
  * Adam's gradient passes sg2_adam_multi's sanitation (nan_to_num) on the fused path.
"""
import copy
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

import legacy
from genlib.utils import util_general
from metrics import metric_utils
from torch_utils.ops import noise_reg, proj_loss

LPIPS_URL = 'https://nvlabs-fi-cdn.nvidia.com/stylegan2-ada-pytorch/pretrained/metrics/vgg16.pt'


def fused_default():
    return os.environ.get('SG2_PROJ_FUSED', '1') != '0'


def split_modalities(img, modalities):
    """[N, C, H, W] -> {modality: [N, 3, H, W]}: one channel is repeated to 3 under the first name, three channels
    are one RGB image under the first name, any other count is one grey image per modality name."""
    channels = img.shape[1]
    if channels == 1:
        return {modalities[0]: img.repeat([1, 3, 1, 1])}
    if channels == 3:
        return {modalities[0]: img}
    return {mode: img[:, i, :, :].unsqueeze(dim=1).repeat([1, 3, 1, 1]) for i, mode in enumerate(modalities)}


def schedule(step, num_steps, w_std, initial_learning_rate=0.1, initial_noise_factor=0.05, lr_rampdown_length=0.25,
             lr_rampup_length=0.05, noise_ramp_length=0.75):
    """(lr, w_noise_scale) of a step, in host float64: cosine ramp-down over the last quarter, linear ramp-up over the
    first 5 %, and a quadratic decay of the perturbation of w over the first 75 %."""
    t = step / num_steps
    w_noise_scale = w_std * initial_noise_factor * max(0.0, 1.0 - t / noise_ramp_length) ** 2
    ramp = min(1.0, (1.0 - t) / lr_rampdown_length)
    ramp = 0.5 - 0.5 * np.cos(ramp * np.pi)
    ramp = ramp * min(1.0, t / lr_rampup_length)
    return initial_learning_rate * ramp, w_noise_scale


def optimise(num_steps, early_stopping, step_fn):
    """Run step_fn(step) -> loss (float) for step = 0 .. num_steps - 1; stop once `early_stopping` steps in a row
    did not improve on the best loss.  Returns (best_step, best_loss); best_step = num_steps if no loss was ever
    below +inf (the reference's initial value)."""
    best_loss, best_step, stale = np.inf, num_steps, 0
    for step in range(num_steps):
        loss = step_fn(step)
        if loss < best_loss:
            best_step, best_loss, stale = step, loss, 0
        else:
            stale += 1
            if stale >= early_stopping:
                print(f'\nEarly Stopping! Total steps: {step}')
                break
    return best_step, best_loss


def optimise_batch(num_steps, early_stopping, step_fn):
    """`optimise` for B independent columns at once: step_fn(step) -> B losses.  Returns (best_steps, best_losses,
    stop_steps), three lists of length B; per column the best step and loss are exactly what `optimise` returns on
    that column's losses, and stop_step is the last step `optimise` would have run (num_steps - 1 if it never stops
    early).  A stopped column keeps being computed while others run, but its later losses are discarded: its best is
    frozen.  The loop ends when every column has stopped, so step_fn runs max(stop_steps) + 1 times."""
    best_loss = best_step = stale = stop = None
    for step in range(num_steps):
        losses = [float(v) for v in step_fn(step)]
        if best_loss is None:
            B = len(losses)
            best_loss, best_step, stale, stop = [np.inf] * B, [num_steps] * B, [0] * B, [num_steps - 1] * B
            running = [True] * B
        for b, loss in enumerate(losses):
            if not running[b]:
                continue
            if loss < best_loss[b]:
                best_step[b], best_loss[b], stale[b] = step, loss, 0
            else:
                stale[b] += 1
                if stale[b] >= early_stopping:
                    print(f'\nEarly Stopping! Sample {b}, total steps: {step}')
                    running[b], stop[b] = False, step
        if not any(running):
            break
    if best_loss is None:
        return [], [], []
    return best_step, best_loss, stop


def w_statistics(G, w_avg_samples, device):
    """Mean [1, 1, C] (float32 numpy) and scalar spread of w over `w_avg_samples` mapped latents of RandomState(123).
    The latents are float64, as in the reference: the mapping network casts."""
    z = np.random.RandomState(123).randn(w_avg_samples, G.z_dim)
    w = G.mapping(torch.from_numpy(z).to(device), None)
    w = w[:, :1, :].cpu().numpy().astype(np.float32)
    w_avg = np.mean(w, axis=0, keepdims=True)
    w_std = (np.sum((w - w_avg) ** 2) / w_avg_samples) ** 0.5
    return w_avg, w_std


def lpips_features(detector, img):
    try:
        return detector(img, resize_images=False, return_lpips=True)
    except (RuntimeError, TypeError) as err:
        names = ' / '.join(metric_utils.detector_env_vars(LPIPS_URL))
        raise RuntimeError(f'the LPIPS detector refused (img, resize_images=False, return_lpips=True): {names} must '
                           f'name NVIDIA\'s scripted VGG16 with the LPIPS head (vgg16.pt), or a module with that '
                           f'signature must be registered with metrics.metric_utils.register_detector ({err})') from err


def _to_uint8_hw(img, idx_mode):
    """channel idx_mode of [1, C, H, W] -> uint8 numpy [H, W, 1]"""
    return img[:, idx_mode, :, :].unsqueeze(0).permute(0, 2, 3, 1).clamp(0, 255).to(torch.uint8)[0].cpu().numpy()


def plot_training(history, plot_training_dir, columns_to_plot=None, **plot_args):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    columns = [c for c in (columns_to_plot or list(history.keys())) if c in history]
    cmap = plt.get_cmap('hsv', len(columns) + 1)
    fig = plt.figure(figsize=(8, 6))
    for i, key in enumerate(columns):
        plt.plot(history[key], label=key, c=cmap(i))
    plt.title(plot_args['title'])
    plt.xlabel(plot_args['xlab'])
    plt.ylabel(plot_args['ylab'])
    plt.legend()
    plt.savefig(os.path.join(plot_training_dir, f"{plot_args['title']}.png"), dpi=400, format='png')
    plt.close(fig)


class StyleGAN2Projector(torch.nn.Module):
    def __init__(self, outdir, device, modalities, dtype, outdir_model, w_lpips=1.0, w_pix=1e-4, w_avg_samples=10000,
                 initial_learning_rate=0.1, initial_noise_factor=0.05, lr_rampdown_length=0.25, lr_rampup_length=0.05,
                 noise_ramp_length=0.75, regularize_noise_weight=1e5, save_final_projection=True, snap_video=False,
                 snap_optimization_history=False, **kwargs):
        """outdir_model: the snapshot file (network-snapshot-*.pkl).  kwargs: the rest of the CLI's projector_kwargs
        (ignored, as in the reference), and `G`: an already loaded G_ema that takes the place of the file."""
        super().__init__()
        self.outdir = outdir
        self.outdir_model = outdir_model
        self.device = device
        self.dtype = dtype
        self.modalities = list(modalities)
        self.w_lpips = w_lpips
        self.w_pix = w_pix
        self.w_avg_samples = w_avg_samples
        self.initial_learning_rate = initial_learning_rate
        self.initial_noise_factor = initial_noise_factor
        self.lr_rampdown_length = lr_rampdown_length
        self.lr_rampup_length = lr_rampup_length
        self.noise_ramp_length = noise_ramp_length
        self.regularize_noise_weight = regularize_noise_weight
        self.save_final_projection = save_final_projection
        self.snap_video = snap_video
        self.snap_optimization_history = snap_optimization_history
        G = kwargs.get('G')
        if G is None:
            print('Loading networks from "%s"...' % self.outdir_model)
            with open(self.outdir_model, 'rb') as f:
                G = legacy.load_network_pkl(f)['G_ema']
        self.G = G.requires_grad_(False).to(self.device)
        self.__dict__['last'] = None       # what the last forward() left: private G, loss history, step-0 gradients

    def _schedule(self, step, num_steps, w_std):
        return schedule(step, num_steps, w_std, self.initial_learning_rate, self.initial_noise_factor,
                        self.lr_rampdown_length, self.lr_rampup_length, self.noise_ramp_length)

    def forward(self, id_patient, id_slice, target, num_steps, early_stopping, w_init=None, verbose=False,
                verbose_logger=True):
        """target [1, C, H, W] float32 in [0, 255] at the generator's resolution -> (w of every step
        [num_steps, num_ws, w_dim], best_step)."""
        def logprint(*args):
            if verbose_logger:
                print(*args)

        G0 = self.G
        assert target.detach().cpu().numpy().dtype == self.dtype
        assert target.min().item() >= 0.0
        assert target.max().item() > 1.0
        assert target.max().item() <= 255.0
        assert target.shape == (1, G0.img_channels, G0.img_resolution, G0.img_resolution)
        since = time.time()
        dev = self.device
        target_modalities = {m: t.to(dev).to(torch.float32) for m, t in split_modalities(target, self.modalities).items()}

        G = copy.deepcopy(G0).eval().requires_grad_(False).to(dev)
        num_ws = G.mapping.num_ws

        if w_init is not None:      # warm start: w_init [num_ws, w_dim] is the mean, its own spread the scale
            w_avg = torch.unsqueeze(w_init, dim=0)[:, :1, :]
            w_std = torch.std(w_avg).item()
            w_avg = w_avg.detach().cpu().numpy()
        else:
            logprint(f'Computing W midpoint and stddev using {self.w_avg_samples} samples...')
            w_avg, w_std = w_statistics(G, self.w_avg_samples, dev)

        noise_names = [name for name, _ in G.synthesis.named_buffers() if 'noise_const' in name]
        owners = [G.synthesis.get_submodule(name.rsplit('.', 1)[0]) if '.' in name else G.synthesis
                  for name in noise_names]

        detector = metric_utils.get_feature_detector(LPIPS_URL, device=dev)

        def features(img):      # (the network normalises its input in place: hand it a copy)
            img = img.clone()
            if img.shape[2] > 256:
                img = F.interpolate(img, size=(256, 256), mode='area')
            return lpips_features(detector, img)

        with torch.no_grad():
            target_features = {m: features(target_modalities[m]) for m in self.modalities}

        w_first = torch.tensor(w_avg, dtype=torch.float32, device=dev)      # [1, 1, C]
        w_dim = w_first.shape[-1]
        w_out = torch.zeros([num_steps, 1, w_dim], dtype=torch.float32, device=dev)
        noise_init = [torch.randn_like(o._buffers['noise_const']) for o in owners]
        sizes = [tuple(n.shape) for n in noise_init]
        table, total = noise_reg.make_table(w_dim, [s[0] for s in sizes])
        fused = fused_default() and torch.device(dev).type == 'cuda' and all(s[0] == s[1] for s in sizes) and \
            noise_reg.supported(table)

        if fused:
            from training.optim import FlatAdam
            flat = torch.zeros([total], dtype=torch.float32, device=dev)
            flat[:w_dim] = w_first.reshape(-1)
            for (off, r), n in zip(table, noise_init):
                flat[off:off + r * r] = n.reshape(-1)
            flat.requires_grad_(True)
            optimizer = FlatAdam([flat], betas=(0.9, 0.999), lr=self.initial_learning_rate)
        else:
            w_opt = w_first.clone().requires_grad_(True)
            noise_bufs = []
            for o, n in zip(owners, noise_init):
                buf = o._buffers['noise_const']
                buf[:] = n
                buf.requires_grad = True
                noise_bufs.append(buf)
            optimizer = torch.optim.Adam([w_opt] + noise_bufs, betas=(0.9, 0.999), lr=self.initial_learning_rate)

        history = util_general.list_dict()
        first_grads, schedules = {}, []
        print(f'Early stopping set to {early_stopping}')

        def step_fn(step):
            lr, w_noise_scale = self._schedule(step, num_steps, w_std)
            for group in optimizer.param_groups:
                group['lr'] = lr
            if fused:
                head, views = noise_reg.unflatten(flat, table, head=w_dim)
                w = head.view(1, 1, w_dim)
                for o, v in zip(owners, views):
                    o._buffers['noise_const'] = v
            else:
                w, views = w_opt, noise_bufs

            w_noise = torch.randn_like(w) * w_noise_scale
            ws = (w + w_noise).repeat([1, num_ws, 1])
            synth = G.synthesis(ws, noise_mode='const')
            synth = (synth + 1) * (255 / 2)
            synth_modalities = split_modalities(synth, self.modalities)

            pix_loss, dist = {}, {}
            for m in self.modalities:
                s = synth_modalities[m]
                pix_loss[m] = self.w_pix * torch.mean((target_modalities[m].float() - s.float()) ** 2)
                dist[m] = self.w_lpips * (target_features[m] - features(s)).square().sum()

            reg_loss = noise_reg.noise_regularizer(flat, table) if fused else noise_reg.noise_regularizer_ref(views)
            loss = reg_loss * self.regularize_noise_weight
            terms = [reg_loss.detach()]
            for m in self.modalities:
                loss = loss + dist[m] + pix_loss[m]
                terms += [dist[m].detach(), pix_loss[m].detach()]
            terms = torch.stack(terms + [loss.detach()]).tolist()       # one host read per step
            history['reg_loss'].append(terms[0] * self.regularize_noise_weight)
            for i, m in enumerate(self.modalities):
                history[f'{m}_lpips_loss'].append(terms[1 + 2 * i])
                history[f'{m}_pix_loss'].append(terms[2 + 2 * i])
            history['tot_loss'].append(terms[-1])
            schedules.append((lr, w_noise_scale))

            if fused:
                flat.grad = None
                loss.backward()
                if step == 0:
                    first_grads['w'] = flat.grad[:w_dim].detach().clone().view(1, 1, w_dim)
                    first_grads['noise'] = [flat.grad[o:o + r * r].detach().clone().view(r, r) for o, r in table]
                optimizer.step_flat(flat.grad, [0], [0], write_grad=False)
                w_out[step] = flat.detach()[:w_dim].view(1, w_dim)
                noise_reg.normalize_noise_(flat, table)
            else:
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if step == 0:
                    first_grads['w'] = w_opt.grad.detach().clone()
                    first_grads['noise'] = [b.grad.detach().clone() for b in noise_bufs]
                optimizer.step()
                w_out[step] = w_opt.detach()[0]
                noise_reg.normalize_noise_ref_(noise_bufs)

            desc = ''.join(f'dist_{m} {terms[1 + 2 * i]:<4.2f}--pix_loss_{m} {terms[2 + 2 * i]:<4.2f} '
                           for i, m in enumerate(self.modalities))
            logprint(f'step {step + 1:>4d}/{num_steps}, lr: {lr}: {desc} loss {terms[-1]:<5.2f}')
            return terms[-1]

        best_step, best_loss = optimise(num_steps, early_stopping, step_fn)

        if fused:       # leave the optimised noise in the private copy as ordinary buffers
            for o, (off, r) in zip(owners, table):
                o._buffers['noise_const'] = flat.detach()[off:off + r * r].view(r, r).clone()
        else:
            for b in noise_bufs:
                b.requires_grad = False
        elapsed = time.time() - since
        print('Optimization completed in {:.0f}m {:.0f}s'.format(elapsed // 60, elapsed % 60))
        print('Best step: {:0f}'.format(best_step))
        print('Best loss: {:4f}'.format(best_loss))

        projected_w_steps = w_out.repeat([1, num_ws, 1])
        self.__dict__['last'] = dict(G=G, history=dict(history), first_grads=first_grads, schedules=schedules, w_avg=w_avg, w_std=w_std,
                                     fused=fused, best_loss=best_loss)

        if self.save_final_projection:
            log_dir = os.path.join(self.outdir, id_patient, 'projections')
            util_general.create_dir(log_dir)
            projected_w = projected_w_steps[best_step]
            np.savez(os.path.join(log_dir, f'w_{id_slice:05d}-best_step_{best_step}.npz'),
                     w=projected_w.unsqueeze(0).cpu().numpy())
            with torch.no_grad():       # (rendered with the generator's own noise, as the reference does)
                synth_image = (self.G.synthesis(projected_w.unsqueeze(0), noise_mode='const') + 1) * (255 / 2)
            import PIL.Image
            for idx_mode, mode in enumerate(self.modalities):
                log_dir = os.path.join(self.outdir, id_patient, mode, 'image_log')
                util_general.create_dir(log_dir)
                pair = np.concatenate([_to_uint8_hw(target, idx_mode), _to_uint8_hw(synth_image, idx_mode)], axis=1)
                PIL.Image.fromarray(pair.squeeze(-1)).save(
                    os.path.join(log_dir, f'img_{id_slice:05d}-best_step_{best_step}.png'))

        if verbose:
            import pandas as pd
            frame = pd.DataFrame.from_dict(dict(history), orient='index').transpose()
            self.logs(id_patient=id_patient, id_slice=id_slice, target=target, history=frame,
                      projected_w_steps=projected_w_steps)
        return projected_w_steps, best_step

    def forward_batch(self, ids, targets, num_steps, early_stopping, w_init=None, verbose=False, verbose_logger=True):
        """B independent projections in one optimisation loop.  ids: B (id_patient, id_slice) pairs; targets
        [B, C, H, W] float32 in [0, 255]; w_init: None (cold: one w_avg and w_std for all), [num_ws, w_dim], or
        [B, num_ws, w_dim] (per-sample mean, its own spread the scale, as forward's warm start) ->
        (w of every step [B, num_steps, num_ws, w_dim], best_steps: B ints).

        Samples share no variable: sample b's loss is  reg_b * regularize_noise_weight + sum_m (w_lpips dist[b, m] +
        w_pix pix[b, m]),  the backward runs on the sum over b, and Adam is elementwise, so every sample is optimised as
        forward() optimises it alone -- with one synthesis, one detector pass and a fixed number of small launches per
        step whatever B is.  Early stopping is per sample (optimise_batch): a stopped sample is still computed while
        others run, but its later steps are discarded (rows of the result left zero, as at batch 1).

        Random draws: the initial noise per sample, then per buffer (torch.randn_like(noise_const), sample-major: at
        B = 1 forward's sequence); then one torch.randn([B, 1, w_dim]) per step."""
        def logprint(*args):
            if verbose_logger:
                print(*args)

        G0 = self.G
        B = len(ids)
        if not 1 <= B <= noise_reg.MAX_BATCH:
            raise RuntimeError(f'forward_batch: the batch must hold 1..{noise_reg.MAX_BATCH} projections; got {B}')
        assert targets.detach().cpu().numpy().dtype == self.dtype
        assert targets.min().item() >= 0.0
        assert targets.max().item() <= 255.0
        assert all(t.max().item() > 1.0 for t in targets)
        assert targets.shape == (B, G0.img_channels, G0.img_resolution, G0.img_resolution)
        since = time.time()
        dev = self.device
        targets = targets.to(dev).to(torch.float32).contiguous()
        M = proj_loss.num_modalities(targets.shape[1])
        modalities = self.modalities[:M]

        G = copy.deepcopy(G0).eval().requires_grad_(False).to(dev)
        num_ws = G.mapping.num_ws

        if w_init is not None:      # warm start per sample: the mean is w_init[b]'s first row, its spread the scale
            w_init = torch.as_tensor(w_init)
            if w_init.ndim == 2:
                w_init = w_init.unsqueeze(0).expand(B, -1, -1)
            assert w_init.shape[0] == B
            w_avgs, w_stds = [], []
            for b in range(B):
                w_avg = torch.unsqueeze(w_init[b], dim=0)[:, :1, :]
                w_stds.append(torch.std(w_avg).item())
                w_avgs.append(w_avg.detach().cpu().numpy())
        else:
            logprint(f'Computing W midpoint and stddev using {self.w_avg_samples} samples...')
            w_avg, w_std = w_statistics(G, self.w_avg_samples, dev)
            w_avgs, w_stds = [w_avg] * B, [w_std] * B

        noise_names = [name for name, _ in G.synthesis.named_buffers() if 'noise_const' in name]
        owners = [G.synthesis.get_submodule(name.rsplit('.', 1)[0]) if '.' in name else G.synthesis
                  for name in noise_names]
        detector = metric_utils.get_feature_detector(LPIPS_URL, device=dev)

        def features(img):      # (the network normalises its input in place: hand it a copy)
            return lpips_features(detector, img.clone())

        with torch.no_grad():   # the target features [M B, F], row m B + b, once
            t_rows = proj_loss.split_rows(targets)
            if t_rows.shape[2] > 256:
                t_rows = F.interpolate(t_rows, size=(256, 256), mode='area')
            target_features = features(t_rows).to(torch.float32).contiguous()

        w_first = torch.tensor(np.concatenate(w_avgs, axis=0), dtype=torch.float32, device=dev)     # [B, 1, C]
        w_dim = w_first.shape[-1]
        w_out = torch.zeros([B, num_steps, w_dim], dtype=torch.float32, device=dev)
        noise_init = [[torch.randn_like(o._buffers['noise_const']) for o in owners] for _ in range(B)]
        sizes = [tuple(n.shape) for n in noise_init[0]]
        noise_init = [torch.stack([noise_init[b][k] for b in range(B)]).unsqueeze(1) for k in range(len(owners))]
        table, total = noise_reg.make_batched_table(B, w_dim, [s[0] for s in sizes])
        fused = fused_default() and torch.device(dev).type == 'cuda' and all(s[0] == s[1] for s in sizes) and \
            noise_reg.supported(table)

        if fused:
            from training.optim import FlatAdam
            wp = table[0][0] // B
            flat = torch.zeros([total], dtype=torch.float32, device=dev)
            flat[:B * wp].view(B, wp)[:, :w_dim] = w_first.view(B, w_dim)
            for (off, r), n in zip(table, noise_init):
                flat[off:off + B * r * r] = n.reshape(-1)
            flat.requires_grad_(True)
            optimizer = FlatAdam([flat], betas=(0.9, 0.999), lr=self.initial_learning_rate)
        else:
            w_opt = w_first.clone().requires_grad_(True)
            noise_bufs = [n.clone().requires_grad_(True) for n in noise_init]       # [B, 1, R, R] leaves
            for o, buf in zip(owners, noise_bufs):
                o._buffers['noise_const'] = buf
            optimizer = torch.optim.Adam([w_opt] + noise_bufs, betas=(0.9, 0.999), lr=self.initial_learning_rate)

        histories = [util_general.list_dict() for _ in range(B)]
        first_grads, schedules = [{} for _ in range(B)], []
        print(f'Early stopping set to {early_stopping}')

        def step_fn(step):
            scheds = [self._schedule(step, num_steps, s) for s in w_stds]
            lr, scales = scheds[0][0], [s[1] for s in scheds]       # (the learning rate does not depend on w_std)
            for group in optimizer.param_groups:
                group['lr'] = lr
            if fused:
                w, views = noise_reg.unflatten_batched(flat, table, B, w_dim)
                for o, v in zip(owners, views):
                    o._buffers['noise_const'] = v
            else:
                w, views = w_opt, noise_bufs

            scale_t = torch.tensor([float(s) for s in scales], dtype=torch.float32).view(B, 1, 1).to(dev)
            w_noise = torch.randn([B, 1, w_dim], device=dev) * scale_t
            ws = (w + w_noise).repeat([1, num_ws, 1])
            synth = G.synthesis(ws, noise_mode='const')
            if fused:
                det_in, pix = proj_loss.prep(synth, targets)                # [M B, 3, Hd, Hd], [B, M]
                dist = proj_loss.sqdist_rows(features(det_in).to(torch.float32), target_features).view(M, B).t()
                reg = noise_reg.noise_regularizer_batched(flat, table, B)   # [B]
            else:
                det_in, pix = proj_loss.prep_ref(synth, targets)
                dist = proj_loss.sqdist_rows_ref(features(det_in), target_features).view(M, B).t()
                reg = noise_reg.noise_regularizer_batched_ref(views)

            loss = reg * self.regularize_noise_weight
            cols = [reg.detach()]
            for m in range(M):
                d, p = self.w_lpips * dist[:, m], self.w_pix * pix[:, m]
                loss = loss + d + p
                cols += [d.detach(), p.detach()]
            terms = torch.stack(cols + [loss.detach()], dim=1).tolist()     # [B, 2 M + 2]: one host read per step
            for b in range(B):
                histories[b]['reg_loss'].append(terms[b][0] * self.regularize_noise_weight)
                for i, m in enumerate(modalities):
                    histories[b][f'{m}_lpips_loss'].append(terms[b][1 + 2 * i])
                    histories[b][f'{m}_pix_loss'].append(terms[b][2 + 2 * i])
                histories[b]['tot_loss'].append(terms[b][-1])
            schedules.append((lr, tuple(scales)))

            if fused:
                flat.grad = None
                loss.sum().backward()
                if step == 0:
                    gw, gviews = noise_reg.unflatten_batched(flat.grad.detach(), table, B, w_dim)
                    for b in range(B):
                        first_grads[b]['w'] = gw[b].clone().view(1, 1, w_dim)
                        first_grads[b]['noise'] = [v[b, 0].clone() for v in gviews]
                optimizer.step_flat(flat.grad, [0], [0], write_grad=False)
                w_out[:, step] = noise_reg.unflatten_batched(flat.detach(), table, B, w_dim)[0][:, 0]
                noise_reg.normalize_noise_batched_(flat, table, B)
            else:
                optimizer.zero_grad(set_to_none=True)
                loss.sum().backward()
                if step == 0:
                    for b in range(B):
                        first_grads[b]['w'] = w_opt.grad[b].detach().clone().view(1, 1, w_dim)
                        first_grads[b]['noise'] = [buf.grad[b, 0].detach().clone() for buf in noise_bufs]
                optimizer.step()
                w_out[:, step] = w_opt.detach()[:, 0]
                noise_reg.normalize_noise_batched_ref_(noise_bufs)

            losses = [t[-1] for t in terms]
            logprint(f'step {step + 1:>4d}/{num_steps}, lr: {lr}: loss ' + ' '.join(f'{v:<5.2f}' for v in losses))
            return losses

        best_steps, best_losses, stop_steps = optimise_batch(num_steps, early_stopping, step_fn)

        # a stopped sample's later steps are discarded: rows left zero and the history cut, as forward() leaves them
        for b in range(B):
            w_out[b, stop_steps[b] + 1:] = 0
            histories[b] = {k: v[:stop_steps[b] + 1] for k, v in histories[b].items()}
        with torch.no_grad():
            if fused:
                final = [flat.detach()[off:off + B * r * r].view(B, r, r).clone() for off, r in table]
            else:
                final = [buf.detach()[:, 0].clone() for buf in noise_bufs]
        elapsed = time.time() - since
        print('Optimization completed in {:.0f}m {:.0f}s'.format(elapsed // 60, elapsed % 60))
        print('Best steps: ' + ' '.join(str(s) for s in best_steps))
        print('Best losses: ' + ' '.join('{:4f}'.format(v) for v in best_losses))

        projected_w_steps = w_out.unsqueeze(2).repeat([1, 1, num_ws, 1])        # [B, num_steps, num_ws, w_dim]
        self.__dict__['last'] = dict(
            batch=B, fused=fused, schedules=schedules,
            samples=[dict(history=histories[b], first_grads=first_grads[b], best_loss=best_losses[b],
                          best_step=best_steps[b], stop_step=stop_steps[b], w_avg=w_avgs[b], w_std=w_stds[b],
                          noise=[n[b] for n in final]) for b in range(B)])

        if self.save_final_projection:
            projected_w = torch.stack([projected_w_steps[b, best_steps[b]] for b in range(B)])     # [B, num_ws, w_dim]
            with torch.no_grad():       # (rendered with the generator's own noise, as the reference does): one synthesis
                synth_images = (self.G.synthesis(projected_w, noise_mode='const') + 1) * (255 / 2)
            import PIL.Image
            for b, (id_patient, id_slice) in enumerate(ids):
                id_slice = int(id_slice)
                log_dir = os.path.join(self.outdir, id_patient, 'projections')
                util_general.create_dir(log_dir)
                np.savez(os.path.join(log_dir, f'w_{id_slice:05d}-best_step_{best_steps[b]}.npz'),
                         w=projected_w[b].unsqueeze(0).cpu().numpy())
                for idx_mode, mode in enumerate(self.modalities):
                    log_dir = os.path.join(self.outdir, id_patient, mode, 'image_log')
                    util_general.create_dir(log_dir)
                    pair = np.concatenate([_to_uint8_hw(targets[b:b + 1], idx_mode),
                                           _to_uint8_hw(synth_images[b:b + 1], idx_mode)], axis=1)
                    PIL.Image.fromarray(pair.squeeze(-1)).save(
                        os.path.join(log_dir, f'img_{id_slice:05d}-best_step_{best_steps[b]}.png'))

        if verbose:
            import pandas as pd
            for b, (id_patient, id_slice) in enumerate(ids):
                frame = pd.DataFrame.from_dict(dict(histories[b]), orient='index').transpose()
                self.logs(id_patient=id_patient, id_slice=int(id_slice), target=targets[b:b + 1], history=frame,
                          projected_w_steps=projected_w_steps[b])
        return projected_w_steps, best_steps

    def logs(self, id_patient, id_slice, target, history, projected_w_steps):
        """The loss table and plots of one projection, and the video of its steps."""
        log_dir = os.path.join(self.outdir, id_patient, 'loss')
        util_general.create_dir(log_dir)
        infix = '' if len(self.modalities) == 1 else 'modalities_'
        if self.snap_optimization_history and id_slice % self.snap_optimization_history == 0:
            for kind in ('lpips', 'pix'):
                plot_training(history=history, plot_training_dir=log_dir,
                              columns_to_plot=[f'{m}_{kind}_loss' for m in self.modalities],
                              title=f'{kind}_loss_{infix}{id_slice:05d}', xlab='Step', ylab='Loss')
            history.to_csv(os.path.join(log_dir, f'opt_loss_{id_slice:05d}.csv'))

        if self.snap_video and id_slice % self.snap_video == 0:
            try:
                import imageio
            except ImportError as err:
                raise RuntimeError('the projection video (snap_video with verbose) needs the imageio package, which is '
                                   'not installed; run with --snap_video larger than the slice count or '
                                   '--verbose False') from err
            with torch.no_grad():
                frames = [(self.G.synthesis(w.unsqueeze(0), noise_mode='const') + 1) * (255 / 2)
                          for w in projected_w_steps]
            for idx_mode, mode in enumerate(self.modalities):
                log_dir = os.path.join(self.outdir, id_patient, mode, 'video_log')
                util_general.create_dir(log_dir)
                video = imageio.get_writer(os.path.join(log_dir, f'movie_{id_slice:05d}.mp4'), mode='I', fps=10,
                                           codec='libx264', bitrate='16M')
                print(f'Saving optimization progress video for slice {id_slice:05d}.mp4 of patient {id_patient}')
                left = _to_uint8_hw(target, idx_mode)
                for frame in frames:
                    video.append_data(np.concatenate([left, _to_uint8_hw(frame, idx_mode)], axis=1))
                video.close()
