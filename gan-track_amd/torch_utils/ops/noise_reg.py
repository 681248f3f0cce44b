"""The small-tensor part of a latent projection step as a handful of HIP launches (csrc/noise_reg.hip).

The reference's projector (SG3/genlib/projector/projector.py:259-268, :294-298) walks the generator's noise buffers
one by one: a pyramid of average pools with two rolled products, means and squares per level, and after the optimiser
step a mean / second-moment renormalisation per buffer -- hundreds of tiny launches per step at batch 1.  Here every
noise buffer of a generator, and the latent in front of them, lives in ONE flat float32 tensor:

    flat = [ head (the latent w, padded to a multiple of 4 floats) | buf 0 (R0 x R0) | buf 1 | ... ]
    table = ((offset, R), ...)        one row per noise buffer, offsets in floats into flat

noise_regularizer(flat, table)   the regulariser, 3 launches forward and 1 backward (first order only)
normalize_noise_(flat, table)    the renormalisation of every buffer in place, 1 launch
unflatten(flat, table)           (head, [R x R views]) whose backward assembles ONE flat gradient in one pass

make_batched_table / unflatten_batched / noise_regularizer_batched / normalize_noise_batched_ are the same for B
independent projections in one flat tensor (buffer-major, see below): the same launch counts whatever B is.

ROCm tensors only.  The `*_ref` functions are the reference's composition on any device: the SG2_PROJ_FUSED=0 path of
the projector and the cross-check of the kernels.
"""
import ctypes

import torch
import torch.nn.functional as F

import sg2hip as _hip

MIN_R, MAX_R, MAX_BUFS = 4, 1024, 32


def make_table(head, sizes):
    """Layout of a flat buffer: `head` floats (rounded up to a multiple of 4) followed by square buffers of the
    given sides.  Returns (table, total floats)."""
    off = (int(head) + 3) // 4 * 4
    table = []
    for r in sizes:
        table.append((off, int(r)))
        off += int(r) * int(r)
    return tuple(table), off


def supported(table):
    """Whether the HIP kernels take this table (square power-of-two buffers of 4..1024, 4-float aligned offsets)."""
    return 1 <= len(table) <= MAX_BUFS and all(
        MIN_R <= r <= MAX_R and r & (r - 1) == 0 and off >= 0 and off % 4 == 0 for off, r in table)


def num_levels(r):
    n = 1
    while r > 8:
        r //= 2
        n += 1
    return n


_ctables = {}


def _ctable(table):
    table = tuple((int(o), int(r)) for o, r in table)
    c = _ctables.get(table)
    if c is None:
        c = _ctables[table] = _hip.i64arr([v for row in table for v in row])
    return c, len(table)


def _check_flat(flat, table, what):
    _hip.require_device(flat)
    if flat.dtype != torch.float32 or flat.ndim != 1 or not flat.is_contiguous():
        raise RuntimeError(f'{what}: flat must be a contiguous 1-D float32 tensor')
    if max(o + r * r for o, r in table) > flat.numel():
        raise RuntimeError(f'{what}: the table reaches past the end of flat ({flat.numel()} floats)')


def _gaps(table, numel):
    """The ranges of flat that no buffer covers (the head, padding)."""
    gaps, pos = [], 0
    for off, r in sorted(table):
        if off > pos:
            gaps.append((pos, off))
        pos = max(pos, off + r * r)
    if pos < numel:
        gaps.append((pos, numel))
    return gaps


class _NoiseReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, table):
        _check_flat(flat, table, 'noise_regularizer')
        ct, nbuf = _ctable(table)
        L = _hip.lib()
        nbytes = ctypes.c_int64(0)
        _hip.check(L.sg2_noise_reg_scratch_bytes(ctypes.byref(nbytes), ct, nbuf), 'sg2_noise_reg_scratch_bytes')
        with torch.cuda.device(flat.device):
            scratch = torch.empty([nbytes.value // 4], dtype=torch.float32, device=flat.device)
            means = torch.empty([sum(num_levels(r) for _, r in table), 2], dtype=torch.float32, device=flat.device)
            reg = torch.empty([], dtype=torch.float32, device=flat.device)
            _hip.check(L.sg2_noise_reg_fwd(_hip.ptr(reg), _hip.ptr(means), _hip.ptr(flat), ct, nbuf, _hip.ptr(scratch),
                                           _hip.stream_ptr(flat.device)), 'sg2_noise_reg_fwd')
        ctx.save_for_backward(flat, means, scratch)
        ctx.table = table
        ctx.mark_non_differentiable(means)
        return reg, means

    @staticmethod
    def backward(ctx, greg, _gmeans):
        if torch.is_grad_enabled():
            raise RuntimeError('noise_regularizer is first order only: its backward cannot be differentiated '
                               '(create_graph=True)')
        flat, means, scratch = ctx.saved_tensors
        ct, nbuf = _ctable(ctx.table)
        greg = greg.to(torch.float32).contiguous()
        with torch.cuda.device(flat.device):
            gflat = torch.empty_like(flat)
            for a, b in _gaps(ctx.table, flat.numel()):
                gflat[a:b].fill_(0)
            _hip.check(_hip.lib().sg2_noise_reg_bwd(_hip.ptr(gflat), _hip.ptr(greg), _hip.ptr(means), _hip.ptr(flat), ct,
                                                    nbuf, _hip.ptr(scratch), 0, _hip.stream_ptr(flat.device)),
                       'sg2_noise_reg_bwd')
        return gflat, None


def noise_regularizer(flat, table, return_means=False):
    """sum over buffers and pyramid levels of mean(n * roll_x n)^2 + mean(n * roll_y n)^2, a 0-d tensor.
    return_means: also the [levels, 2] per-level means (buffers in table order, finest level first)."""
    reg, means = _NoiseReg.apply(flat, tuple(table))
    return (reg, means) if return_means else reg


def noise_regularizer_backward(gflat, greg, flat, means, scratch, table, accumulate):
    """The raw backward launch (tests, and callers that own the flat gradient): gflat (+)= greg * d reg / d flat."""
    ct, nbuf = _ctable(table)
    _hip.check(_hip.lib().sg2_noise_reg_bwd(_hip.ptr(gflat), _hip.ptr(greg), _hip.ptr(means), _hip.ptr(flat), ct, nbuf,
                                            _hip.ptr(scratch), int(accumulate), _hip.stream_ptr(flat.device)),
               'sg2_noise_reg_bwd')
    return gflat


def normalize_noise_(flat, table):
    """Per buffer, in place: x -= x.mean(); x *= x.square().mean().rsqrt().  One launch for all buffers."""
    _check_flat(flat, table, 'normalize_noise_')
    ct, nbuf = _ctable(table)
    with torch.no_grad(), torch.cuda.device(flat.device):
        _hip.check(_hip.lib().sg2_noise_normalize_multi(_hip.ptr(flat), ct, nbuf, _hip.stream_ptr(flat.device)),
                   'sg2_noise_normalize_multi')
    return flat


class _Unflatten(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, table, head):
        ctx.table, ctx.head, ctx.numel = table, head, flat.numel()
        outs = [flat[:head]] + [flat[o:o + r * r].view(r, r) for o, r in table]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        # one torch.cat (a single pass over the flat gradient) instead of a zero-padded add per view
        ref = next(g for g in grads if g is not None)
        pieces, pos = [], 0
        spans = [(0, ctx.head)] + [(o, o + r * r) for o, r in ctx.table]
        for (a, b), g in zip(spans, grads):
            if a > pos:
                pieces.append(ref.new_zeros([a - pos]))
            pieces.append(ref.new_zeros([b - a]) if g is None else g.reshape(-1))
            pos = b
        if pos < ctx.numel:
            pieces.append(ref.new_zeros([ctx.numel - pos]))
        return torch.cat(pieces), None, None


def unflatten(flat, table, head=None):
    """(head, [views]): flat[:head] (default: everything in front of the first buffer) and one [R, R] view per table
    row.  The views share flat's memory; the backward writes all incoming gradients into one flat gradient."""
    table = tuple(table)
    if head is None:
        head = min(o for o, _ in table)
    if any(a[0] + a[1] ** 2 > b[0] for a, b in zip(table, table[1:])) or head > table[0][0]:
        raise RuntimeError('unflatten: the table must list non-overlapping buffers in increasing order behind the head')
    outs = _Unflatten.apply(flat, table, int(head))
    return outs[0], list(outs[1:])


# ---- B projections at once: the buffer-major layout and its kernels (the sample is a grid dimension) ----
#
#     flat = [ w: B rows x Wp floats (Wp = w_dim rounded up to a multiple of 4) | buf 0: B x R0 x R0 | buf 1: ... ]
#
# so every [B, 1, R, R] noise view is contiguous.  Per sample the kernels run the batch-1 code: sample b's results are
# bitwise those of noise_regularizer / normalize_noise_ on that sample's buffers alone.

MAX_BATCH = 64


def make_batched_table(B, w_dim, sizes):
    """Layout of B projections in one flat buffer: B latent rows of w_dim floats (each padded to a multiple of 4), then
    per noise buffer its B samples one after another.  Returns (table of (off_k, R_k), total floats); sample b of
    buffer k starts at off_k + b * R_k^2.  At B = 1 this is make_table(w_dim, sizes)."""
    B = int(B)
    if B < 1:
        raise RuntimeError('make_batched_table: B must be at least 1')
    off = B * ((int(w_dim) + 3) // 4 * 4)
    table = []
    for r in sizes:
        table.append((off, int(r)))
        off += B * int(r) * int(r)
    return tuple(table), off


def _check_flat_batched(flat, table, B, what):
    _hip.require_device(flat)
    if flat.dtype != torch.float32 or flat.ndim != 1 or not flat.is_contiguous():
        raise RuntimeError(f'{what}: flat must be a contiguous 1-D float32 tensor')
    if max(o + B * r * r for o, r in table) > flat.numel():
        raise RuntimeError(f'{what}: the table reaches past the end of flat ({flat.numel()} floats)')


def _gaps_batched(table, B, numel):
    """The ranges of flat that no buffer covers (the latent rows, padding)."""
    gaps, pos = [], 0
    for off, r in sorted(table):
        if off > pos:
            gaps.append((pos, off))
        pos = max(pos, off + B * r * r)
    if pos < numel:
        gaps.append((pos, numel))
    return gaps


class _NoiseRegBatched(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, table, B):
        _check_flat_batched(flat, table, B, 'noise_regularizer_batched')
        ct, nbuf = _ctable(table)
        L = _hip.lib()
        nbytes = ctypes.c_int64(0)
        _hip.check(L.sg2_noise_reg_batched_scratch_bytes(ctypes.byref(nbytes), ct, nbuf, B),
                   'sg2_noise_reg_batched_scratch_bytes')
        with torch.cuda.device(flat.device):
            scratch = torch.empty([nbytes.value // 4], dtype=torch.float32, device=flat.device)
            means = torch.empty([B, sum(num_levels(r) for _, r in table), 2], dtype=torch.float32, device=flat.device)
            reg = torch.empty([B], dtype=torch.float32, device=flat.device)
            _hip.check(L.sg2_noise_reg_fwd_batched(_hip.ptr(reg), _hip.ptr(means), _hip.ptr(flat), ct, nbuf, B,
                                                   _hip.ptr(scratch), _hip.stream_ptr(flat.device)),
                       'sg2_noise_reg_fwd_batched')
        ctx.save_for_backward(flat, means, scratch)
        ctx.table, ctx.B = table, B
        ctx.mark_non_differentiable(means)
        return reg, means

    @staticmethod
    def backward(ctx, greg, _gmeans):
        if torch.is_grad_enabled():
            raise RuntimeError('noise_regularizer_batched is first order only: its backward cannot be differentiated '
                               '(create_graph=True)')
        flat, means, scratch = ctx.saved_tensors
        greg = greg.to(torch.float32).contiguous()
        with torch.cuda.device(flat.device):
            gflat = torch.empty_like(flat)
            for a, b in _gaps_batched(ctx.table, ctx.B, flat.numel()):
                gflat[a:b].fill_(0)
            noise_regularizer_batched_backward(gflat, greg, flat, means, scratch, ctx.table, ctx.B, accumulate=0)
        return gflat, None, None


def noise_regularizer_batched(flat, table, B, return_means=False):
    """The regulariser of each of B projections laid out by make_batched_table: a [B] tensor (3 launches forward, 1
    backward, whatever B is; first order only).  return_means: also the [B, levels, 2] per-level means."""
    B = int(B)
    if not 1 <= B <= MAX_BATCH:
        raise RuntimeError(f'noise_regularizer_batched: B must be in 1..{MAX_BATCH}')
    reg, means = _NoiseRegBatched.apply(flat, tuple(table), B)
    return (reg, means) if return_means else reg


def noise_regularizer_batched_backward(gflat, greg, flat, means, scratch, table, B, accumulate):
    """The raw backward launch: gflat (+)= greg[b] * d reg[b] / d flat over every sample of every buffer."""
    ct, nbuf = _ctable(table)
    _hip.check(_hip.lib().sg2_noise_reg_bwd_batched(_hip.ptr(gflat), _hip.ptr(greg), _hip.ptr(means), _hip.ptr(flat), ct,
                                                    nbuf, int(B), _hip.ptr(scratch), int(accumulate),
                                                    _hip.stream_ptr(flat.device)), 'sg2_noise_reg_bwd_batched')
    return gflat


def normalize_noise_batched_(flat, table, B):
    """Per sample and buffer, in place: x -= x.mean(); x *= x.square().mean().rsqrt().  One launch."""
    B = int(B)
    if not 1 <= B <= MAX_BATCH:
        raise RuntimeError(f'normalize_noise_batched_: B must be in 1..{MAX_BATCH}')
    _check_flat_batched(flat, table, B, 'normalize_noise_batched_')
    ct, nbuf = _ctable(table)
    with torch.no_grad(), torch.cuda.device(flat.device):
        _hip.check(_hip.lib().sg2_noise_normalize_batched(_hip.ptr(flat), ct, nbuf, B, _hip.stream_ptr(flat.device)),
                   'sg2_noise_normalize_batched')
    return flat


class _UnflattenBatched(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, table, B, w_dim):
        wp = (w_dim + 3) // 4 * 4
        ctx.table, ctx.B, ctx.w_dim, ctx.wp, ctx.numel = table, B, w_dim, wp, flat.numel()
        w = flat[:B * wp].view(B, 1, wp)[:, :, :w_dim]
        return (w,) + tuple(flat[o:o + B * r * r].view(B, 1, r, r) for o, r in table)

    @staticmethod
    def backward(ctx, *grads):
        # one torch.cat (a single pass over the flat gradient), as _Unflatten
        ref = next(g for g in grads if g is not None)
        B, pad = ctx.B, ctx.wp - ctx.w_dim
        if grads[0] is None:
            head = ref.new_zeros([B * ctx.wp])
        else:
            head = grads[0].reshape(B, ctx.w_dim)
            head = (F.pad(head, (0, pad)) if pad else head).reshape(-1)
        pieces, pos = [head], B * ctx.wp
        for (o, r), g in zip(ctx.table, grads[1:]):
            if o > pos:
                pieces.append(ref.new_zeros([o - pos]))
            pieces.append(ref.new_zeros([B * r * r]) if g is None else g.reshape(-1))
            pos = o + B * r * r
        if pos < ctx.numel:
            pieces.append(ref.new_zeros([ctx.numel - pos]))
        return torch.cat(pieces), None, None, None


def unflatten_batched(flat, table, B, w_dim):
    """(w [B, 1, w_dim], [one contiguous [B, 1, R, R] view per table row]) of a make_batched_table layout.  The views
    share flat's memory; the backward writes all incoming gradients into one flat gradient in one pass."""
    table, B, w_dim = tuple(table), int(B), int(w_dim)
    wp = (w_dim + 3) // 4 * 4
    if any(a[0] + B * a[1] ** 2 > b[0] for a, b in zip(table, table[1:])) or B * wp > table[0][0]:
        raise RuntimeError('unflatten_batched: the table must list non-overlapping buffers of B samples in increasing '
                           'order behind the B latent rows')
    if table[-1][0] + B * table[-1][1] ** 2 > flat.numel():
        raise RuntimeError(f'unflatten_batched: the table reaches past the end of flat ({flat.numel()} floats)')
    outs = _UnflattenBatched.apply(flat, table, B, w_dim)
    return outs[0], list(outs[1:])


# ---- the reference's composition (any device) ----

def noise_regularizer_ref(bufs):
    """SG3/genlib/projector/projector.py:259-268 over a list of [R, R] tensors."""
    total = 0.0
    for buf in bufs:
        level = buf.reshape(1, 1, *buf.shape)
        for l in range(num_levels(buf.shape[-1])):
            if l:
                level = F.avg_pool2d(level, kernel_size=2)
            for axis in (3, 2):         # x first, then y: the reference's order of additions
                total = total + (level * level.roll(1, axis)).mean() ** 2
    return total


def normalize_noise_ref_(bufs):
    """SG3/genlib/projector/projector.py:294-298 over a list of tensors, in place."""
    with torch.no_grad():
        for buf in bufs:
            buf.sub_(buf.mean())
            buf.mul_(buf.square().mean().rsqrt())


def noise_regularizer_batched_ref(bufs):
    """noise_regularizer_ref per sample over a list of [B, 1, R, R] tensors: a [B] tensor."""
    total = 0.0
    for buf in bufs:
        level = buf
        for l in range(num_levels(buf.shape[-1])):
            if l:
                level = F.avg_pool2d(level, kernel_size=2)
            for axis in (3, 2):
                total = total + (level * level.roll(1, axis)).mean(dim=(1, 2, 3)) ** 2
    return total


def normalize_noise_batched_ref_(bufs):
    """normalize_noise_ref_ per sample over a list of [B, 1, R, R] tensors, in place."""
    with torch.no_grad():
        for buf in bufs:
            buf.sub_(buf.mean(dim=(1, 2, 3), keepdim=True))
            buf.mul_(buf.square().mean(dim=(1, 2, 3), keepdim=True).rsqrt())
