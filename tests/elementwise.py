"""Elementwise parity of a 16-bit kernel output against a float64 reference (test infrastructure).

rel_err (golden_util) is one number per tensor; a correct MFMA kernel sits 12-25 x under its tolerance in norm, so a
fault confined to a tile corner, a halo row or one channel fits inside.  Here every element is held to

    |got - ref| <= u |ref| + (1 + u) slack + tiny

u:     the unit roundoff of the output type (2^-11 fp16, 2^-8 bf16, 0 for an f32 output): the one final rounding;
slack: the absolute error the kernel may carry BEFORE that rounding (a float64 tensor the test derives from the
       kernel's arithmetic, below), which the final rounding can stretch by (1 + u);
tiny:  half the smallest subnormal spacing of fp16 (2^-25); 0 otherwise (bf16 and f32 share f32's exponent range).

No element is exempt.  The bound only holds when `ref` rounds where the kernel rounds, so the builders below mirror
the documented rounding points (conv3x3.hip), and a test names the ONE model its route uses.

`ref` is always CPU float64 torch of the rounded operands: never a kernel or a product wrapper of this project.
"""
import torch
import torch.nn.functional as F

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0, torch.float32: 0.0}
EPS32 = 2.0 ** -24          # unit roundoff of an f32 operation


def _f64(t):
    return t.detach().double().cpu()


def ratios(got, ref, slack, out_dtype):
    """|got - ref| / bound per element (float64)."""
    got, ref = _f64(got), _f64(ref)
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    u = U[out_dtype]
    slack = torch.as_tensor(slack, dtype=torch.float64)
    bound = u * ref.abs() + (1 + u) * slack + TINY[out_dtype]
    err = (got - ref).abs()
    # 0 / 0 (an exact element with a zero bound, e.g. an f32 zero) is no violation; x / 0 is one
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isnan(got), torch.full_like(r, float('inf')), r)


def assert_elementwise(got, ref, slack, out_dtype, what):
    """Every element of `got` within the bound of `ref` -> the worst error / bound ratio (<= 1)."""
    r = ratios(got, ref, slack, out_dtype)
    bad = r > 1
    nbad = int(bad.sum())
    if nbad:
        got, ref = _f64(got), _f64(ref)
        idx = bad.nonzero()
        lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
        worst = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape)) if r.dim() else ()
        raise AssertionError(
            f'{what}: {nbad} of {r.numel()} elements outside the elementwise bound; worst at {worst}: '
            f'got {got[worst].item():.9g}, ref {ref[worst].item():.9g}, error / bound {r[worst].item():.4g}; '
            f'violators span {tuple(lo)} .. {tuple(hi)} (inclusive, index order of shape {tuple(r.shape)})')
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------ slack builders
def accumulation_slack(K, A):
    """An f32 accumulation of K products of 16-bit values: 2 K 2^-24 A, A the same convolution / correlation / FIR of
    the operands' absolute values in float64.  The products are exact in f32 (11 + 11 or 8 + 8 significand bits); each
    of the at most K additions errs by one f32 rounding of a partial sum that |.| bounds by A; the factor 2 covers an
    accumulator that truncates instead of rounding to nearest (the 16-bit MFMAs' mode is not documented)."""
    return 2.0 * K * EPS32 * A


def epilogue_slack(slack_c, c, d=1.0, noise_g=0.0, b=0.0, gain=1.0, alpha=1.0, f32_ops=8):
    """clamp(lrelu(c d + noise g + b) gain) after an accumulation c with slack slack_c.  lrelu, the gain and the clamp
    are Lipschitz with gain max(1, alpha) together; the handful of f32 operations (two multiply-adds, the lrelu
    product, the gain -- or the persistent kernels' folded gain and max(v, alpha v)) get `f32_ops` roundings in total
    of a value no larger than |c d| + |noise g| + |b|, whatever their order."""
    d = torch.as_tensor(d, dtype=torch.float64)
    mag = (c * d).abs() + torch.as_tensor(noise_g, dtype=torch.float64).abs() + torch.as_tensor(b, dtype=torch.float64).abs()
    return gain * max(1.0, alpha) * (d.abs() * slack_c + f32_ops * EPS32 * mag)


# ------------------------------------------------------------------ references that round where the routes round
def rnd(t, dtype):
    """One rounding of an f32-exact value to `dtype`, as float64."""
    return t.float().to(dtype).double()


def mod_x(x, s, dtype):
    """x-side modulation round(x round(s)) (networks_stylegan2.py:69; conv3x3.hip: the register-staged halo kernel,
    its LDS-DMA form, the persistent c64p kernel, the stride-2 halo kernel, up2).  The product of two 16-bit values is
    exact in f32, so this is one rounding."""
    return (x.to(dtype).float() * s.to(dtype).float()[:, :, None, None]).to(dtype).double()


def mod_x_f32(x, s, dtype):
    """The LDS-DMA scaled wgrad: x stays 16-bit, s stays f32 and multiplies the f32 partial sums ('the
    product here stays in f32') -> the exact x s in float64 (wgrad_ref's f32_ops carries the factor's roundings)."""
    return x.to(dtype).double() * s.float().double()[:, :, None, None]


def mod_w(w, s, dtype):
    """Weight-side modulation round(W round(s)) per sample (the C = 64 ring forms and the C = 32 ring):
    [N, Cout, Cin, kh, kw] float64."""
    return (w.to(dtype).float()[None] * s.to(dtype).float()[:, None, :, None, None]).to(dtype).double()


def conv_per_sample(x, wn, **kw):
    """F.conv2d with one weight set per sample (wn [N, Cout, Cin, kh, kw]) as a grouped convolution."""
    N, Cout = wn.shape[:2]
    y = F.conv2d(x.reshape(1, -1, *x.shape[2:]), wn.reshape(-1, *wn.shape[2:]), groups=N, **kw)
    return y.reshape(N, Cout, *y.shape[2:])


def bias_rounded(b, dtype):
    """The bias rounded to the activation type (conv3x3.hip: `(float)(T)a.bias[oc]`) as [1, C, 1, 1] float64."""
    return rnd(b, dtype)[None, :, None, None]


def add_residual(v, slack_v, residual, dtype):
    """round(round(v) + residual), the stride-2 routes' resnet add -> (ref, slack).  Two roundings: the last one is
    the check's own u |ref| term; the first one, round(v), cannot be replayed in float64 (a kernel value within
    slack_v of a tie may fall either way, a whole 16-bit ulp apart), so it is carried as slack around the unrounded
    v: u |v| + (1 + u) slack_v + tiny, plus one f32 rounding of the sum."""
    u = U[dtype]
    ref = v + residual.to(dtype).double()
    return ref, u * v.abs() + (1 + u) * slack_v + TINY[dtype] + EPS32 * ref.abs()


def mod_x_f32s(x, s, dtype):
    """round(x s) with the scale left in f32: conv.hip's kernels (`(T)(v * in_scale)`) and the register-staged weight
    gradients (wgrad3x3.hip scale8).  The f32 product is rounded to f32 and then to the 16-bit type; replayed here
    operation for operation.  Callers that want the reference's x * s.to(x.dtype) pass a rounded s."""
    return (x.to(dtype).float() * s.float()[:, :, None, None]).to(dtype).double()


def wgrad_ref(g, x, wshape, f32_ops=0, **kw):
    """(dw, slack) of the weight gradient sum_{n,y,x} g x in float64 (operands already rounded, float64):
    K = N OH OW products per element, accumulated in f32 (over MFMAs, workgroup partial sums and their final adds);
    `f32_ops` further f32 roundings of the sum (a scale factor applied to the partial sums)."""
    dw = torch.nn.grad.conv2d_weight(x, wshape, g, **kw)
    K = g.shape[0] * g.shape[2] * g.shape[3]
    A = torch.nn.grad.conv2d_weight(x.abs(), wshape, g.abs(), **kw)
    return dw, accumulation_slack(K, A) + f32_ops * EPS32 * A


def min_dropped_term_ratio(g, x_tap, bound):
    """The weight gradient's slack grows as K^2 while one term stays O(1), so at a large N OH OW the bound would let a
    kernel drop a whole pixel.  For one tap: g [N, A, OH, OW] and x_tap [N, B, OH, OW] (the x sample each g pixel meets
    at that tap), bound [A, B] -> over all (n, y, x), the smallest of max_{a,b} |g x| / bound: above 1, dropping any
    single (n, y, x) term pushes at least one element over the bound."""
    worst = float('inf')
    for n in range(g.shape[0]):
        ga = g[n].abs().flatten(1).t()                 # [P, A]
        xa = x_tap[n].abs().flatten(1).t()             # [P, B]
        for p in range(0, ga.shape[0], 64):
            r = (ga[p:p + 64, :, None] * xa[p:p + 64, None, :] / bound[None]).flatten(1).max(1).values
            worst = min(worst, float(r.min()))
    return worst


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _upfirdn(x, f, up, down, padding, flip_filter):
    """up / down: one factor for both axes, or (x, y) as the separable passes of a 1-D filter need them."""
    N, C, H, W = x.shape
    (upx, upy), (downx, downy) = _pair(up), _pair(down)
    px0, px1, py0, py1 = [padding] * 4 if isinstance(padding, int) else padding
    x = F.pad(x.reshape(N, C, H, 1, W, 1), [0, upx - 1, 0, 0, 0, upy - 1]).reshape(N, C, H * upy, W * upx)
    x = F.pad(x, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    x = x[:, :, max(-py0, 0):x.shape[2] - max(-py1, 0), max(-px0, 0):x.shape[3] - max(-px1, 0)]
    f = f if flip_filter else f.flip([0, 1])
    return F.conv2d(x, f[None, None].repeat(C, 1, 1, 1), groups=C)[:, :, ::downy, ::downx]


def fir_ref(x, f, dtype, up=1, down=1, padding=0, flip_filter=False, gain=1):
    """(ref, slack) of a 2-D FIR (zero-stuff by `up`, pad, correlate with the flipped filter, keep every `down`-th) in
    float64.  upfirdn2d.hip folds the gain into the f32 taps (`f * gain`, replayed in f32 here) and runs one pass over
    a 2-D filter, so nothing rounds between passes; a tap is an f32 value, so each of the K = taps products rounds once
    (an FMA), which the accumulation slack's factor 2 covers in place of a truncating accumulator (VALU f32 FMAs round
    to nearest)."""
    assert f.ndim == 2
    fg = (f.float() * torch.tensor(gain, dtype=torch.float32)).double()
    xd = x.to(dtype).double()
    kw = dict(up=up, down=down, padding=padding, flip_filter=flip_filter)
    return _upfirdn(xd, fg, **kw), accumulation_slack(f.numel(), _upfirdn(xd.abs(), fg.abs(), **kw))


# ------------------------------------------------------------------ the ADA geometric kernels (test_ada_geom_gpu.py)
def assert_regions(got, computed, band, what, ref=None, slack=None, out_dtype=torch.float32, exact=False):
    """The three regions of a buffer that is partial by contract (got [N, C, H, W], poisoned with NaN before the
    kernel ran): rows < computed[0] and cols < computed[1] hold `ref` (bitwise when `exact`, else within the
    elementwise bound); the rest of rows < band[0], cols < band[1] is exactly 0.0; everything else is still NaN,
    i.e. was never stored.  Extents beyond the buffer clamp to it.  -> the worst error / bound ratio."""
    g = got.detach().cpu()
    H, W = g.shape[2:]
    cy, cx, by, bx = min(computed[0], H), min(computed[1], W), min(band[0], H), min(band[1], W)
    rows, cols = torch.arange(H)[:, None], torch.arange(W)[None]
    in_c = (rows < cy) & (cols < cx)
    in_b = (rows < by) & (cols < bx) & ~in_c
    rest = ~(in_c | in_b)
    nz = int((g[:, :, in_b] != 0).sum())            # NaN != 0 is true: a NaN left in the band counts
    assert nz == 0, f'{what}: {nz} of {g[:, :, in_b].numel()} zero-band elements (out to {by} x {bx}) are not 0.0'
    nw = int((~torch.isnan(g[:, :, rest])).sum())
    assert nw == 0, f'{what}: {nw} elements beyond the band ({by} x {bx} of {H} x {W}) were stored'
    sub = g[:, :, :cy, :cx]
    if exact:
        r = _f64(ref)[:, :, :cy, :cx]
        nd = int((sub.double() != r).sum())
        assert nd == 0, f'{what}: {nd} of {sub.numel()} elements of the computed region differ (bitwise)'
        return 0.0
    return assert_elementwise(sub, _f64(ref)[:, :, :cy, :cx], torch.as_tensor(slack)[:, :, :cy, :cx], out_dtype, what)


def reflect_pad_adjoint_ref(gy, hw, margins):
    """(ref, slack) of the adjoint of F.pad(x, reflect) for gy [N, C, Hd, Wd] float64 (the padded image's gradient,
    cropped): the float64 autograd gradient.  A source pixel sums at most 3 x 3 padded positions in f32: at most 8
    additions (9 with the accumulator's zero), each rounding a partial sum that the same adjoint of |gy| bounds."""
    mx0, my0, mx1, my1 = margins
    x = torch.zeros([*gy.shape[:2], *hw], dtype=torch.float64, requires_grad=True)
    y = F.pad(x, (mx0, mx1, my0, my1), mode='reflect')
    assert y.shape == gy.shape, (y.shape, gy.shape)
    ref, = torch.autograd.grad(y, [x], gy, retain_graph=True)
    mag, = torch.autograd.grad(y, [x], gy.abs())
    return ref, 8 * EPS32 * mag


AFFINE_F32_OPS = 8      # roundings of t0 bx + t1 by + t2 and of base_coord, per unit of |t0| + |t1| + |t2| (below)


def grid_sample_ref(x, grid, theta=None):
    """(ref, slack) of the bilinear sample (zeros padding, align_corners = False) of x [N, C, H, W] float64 (the
    rounded operands) at grid [N, Ho, Wo, 2] float64 (the f32 grid the kernel reads, or affine_grid of the f32 theta
    in float64).  grid_sample.hip corners_g forms ix = ((g + 1) W - 1) / 2 in f32: an add, a product and a
    subtraction (the halving is exact), each rounding a value <= (|g| + 1) W, and the weight differences ix - fx,
    (fx + 1) - ix one more: 4 roundings, dix = 4 2^-24 (|gx| + 1) W, diy likewise with H.  With `theta` (the
    in-kernel affine grid) g itself is rounded: base_coord (a division and a subtraction of values <= 2, 3 2^-24
    absolute), two products and two sums of values <= |t0| + |t1| + |t2|: under AFFINE_F32_OPS = 8 roundings of
    that sum, times W / 2 in ix.  A coordinate error d moves a bilinear value by at most d times the largest
    difference of neighbouring pixels, <= 2 M with M the largest |x| in the 5 x 5 pixels around floor(ix, iy) (zero
    outside the image; two pixels each way cover a floor that d moved across a boundary).  The four products and
    three additions of the f32 sum: 8 2^-24 S, S the same sample of |x|.  The output type's rounding is
    assert_elementwise's own u |ref| term."""
    N, C, H, W = x.shape
    Ho, Wo = grid.shape[1:3]
    kw = dict(mode='bilinear', padding_mode='zeros', align_corners=False)
    ref = F.grid_sample(x, grid, **kw)
    S = F.grid_sample(x.abs(), grid, **kw)
    gx, gy = grid[..., 0], grid[..., 1]
    dx = 4 * EPS32 * (gx.abs() + 1) * W
    dy = 4 * EPS32 * (gy.abs() + 1) * H
    if theta is not None:
        t = theta.double().abs().sum(2)                            # [N, 2]
        dx = dx + AFFINE_F32_OPS * EPS32 * t[:, 0, None, None] * W / 2
        dy = dy + AFFINE_F32_OPS * EPS32 * t[:, 1, None, None] * H / 2
    x0 = (((gx + 1) * W - 1) / 2).floor().clamp(-3, W + 2).long() + 3
    y0 = (((gy + 1) * H - 1) / 2).floor().clamp(-3, H + 2).long() + 3
    m = F.max_pool2d(F.pad(x.abs(), [3, 3, 3, 3]), 5, 1, 2)        # [N, C, H + 6, W + 6]: max |x| over 5 x 5
    idx = (y0 * (W + 6) + x0).view(N, 1, -1).expand(N, C, -1)
    M = m.flatten(2).gather(2, idx).view(N, C, Ho, Wo)
    return ref, 2 * (dx + dy)[:, None] * M + 8 * EPS32 * S


def grid_sample_grad_ref(x_shape, grid, dy):
    """(ref, tol) of grid_sample's input gradient for dy [N, C, Ho, Wo] float64: the float64 autograd gradient and
    the bound of test_det_gather_matches_scatter_ada_maps, 2^-11 (the same gradient of |dy| + max |dy|)."""
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    y = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    ref, = torch.autograd.grad(y, [x], dy, retain_graph=True)
    mag, = torch.autograd.grad(y, [x], dy.abs())
    return ref, 2.0 ** -11 * (mag + float(dy.abs().max()))


def fir_chain_ref(x, passes, dtype=torch.float32):
    """(ref, slack) of FIR passes run one after the other (a separable filter's horizontal and vertical launch), each
    a dict(f=2-D filter, up, down, padding, flip_filter, gain) as fir_ref takes them.  The reference is the float64
    chain; a pass's slack is the previous slack pushed through its |taps| plus its own accumulation slack on the
    operand it really meets (|previous reference| + previous slack).  Nothing rounds between f32 passes."""
    ref = x if x.dtype == torch.float64 else x.to(dtype).double()     # (float64: taken as already rounded)
    slack = torch.zeros_like(ref)
    for p in passes:
        fg = (p['f'].float() * torch.tensor(p.get('gain', 1), dtype=torch.float32)).double()
        kw = dict(up=p.get('up', 1), down=p.get('down', 1), padding=p.get('padding', 0),
                  flip_filter=p.get('flip_filter', False))
        slack = _upfirdn(slack, fg.abs(), **kw) + accumulation_slack(fg.numel(), _upfirdn(ref.abs() + slack, fg.abs(), **kw))
        ref = _upfirdn(ref, fg, **kw)
    return ref, slack


# ------------------------------------------------------------------ the layer-backward kernels (test_layer_bwd_gpu.py)
# layer_bwd.hip: sg2_layer_bwd, sg2_dot_hw and sg2_vjp_axpy share one lane layout.  A lane owns 8 channels of a pixel,
# LP = C / 8 lanes cover a pixel, PPP = 256 // LP pixels are in flight per pass (threads beyond LP PPP idle), and a
# workgroup owns min(HW, passes PPP) pixels: passes = 16 in layer_bwd and vjp_axpy, 32 in dot_hw.
LB_CS = (8, 24, 64, 96, 512, 520, 1024, 2048)       # LP 1, 3, 8, 12, 64, 65, 128, 256: every path of the layout
LB_BOUND_CS = (24, 64, 1024)                        # the three noise routes: LDS (no power of two), shuffle, LDS (> 64)
LB_NS = (1, 3)
LB_EXACT = dict(alpha=0.25, gain=2.0, clamp=2.5)    # powers of two (and a clamp on the y grid): every product exact
LB_QUANTUM = 0.5                                    # every term of every reduction of the exact fixture is k / 2


def f32(v):
    """A Python scalar as the kernel receives it (a float argument)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def gamma(k):
    """k f32 roundings in a row: (1 + 2^-24)^k - 1 <= k 2^-24 / (1 - k 2^-24)."""
    return k * EPS32 / (1 - k * EPS32)


def lb_layout(C, passes=16):
    """(LP, PPP, pixels per workgroup at HW -> infinity)."""
    LP = C // 8
    PPP = 256 // LP
    return LP, PPP, passes * PPP


def lb_hws(C, passes=16):
    """One pixel; a second pass of one pixel; exactly one workgroup; a second workgroup of one pixel; several
    workgroups with a tail that is no multiple of the 4 PPP pixels a lane keeps in flight."""
    _, PPP, ppb = lb_layout(C, passes)
    return [1, PPP + 1, ppb, ppb + 1, 37 * PPP + 5]


def lb_exact_operands(N, C, HW):
    """Operands (float64 [N, C, HW, 1] and [N, C]) whose every product and partial sum in the three kernels is exact
    in f32 and whose every elementwise result is a bf16 (hence fp16, f32) value: small integers, halves for y (so
    y == 0 and |y| == clamp are frequent), powers of two for the per-(sample, channel) factors.  A dropped, doubled or
    misrouted term then is a bitwise mismatch in any summation order.  lb_assert_exact checks the precondition."""
    g = torch.Generator().manual_seed(1000003 * C + 101 * HW + N)
    shape = (N, C, HW, 1)

    def ints(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, generator=g).double()

    def pow2(*s):
        return 2.0 ** ints(-1, 2, *s)
    op = dict(dy=ints(-8, 8, *shape), c=ints(-8, 8, *shape), y=ints(-6, 6, *shape) / 2, a=ints(-8, 8, *shape),
              b=ints(-8, 8, *shape), e=ints(-8, 8, *shape), d=pow2(N, C), sa=pow2(N, C))
    op['sb'] = pow2(N, C) * (ints(0, 1, N, C) * 2 - 1)
    return op


def lb_random_operands(N, C, HW, dtype, seed=0):
    """Random normal operands rounded to `dtype` (float64 values): y scaled by 2 so that a clamp of 2.5 masks some."""
    g = torch.Generator().manual_seed(7919 * C + 13 * HW + N + seed)
    shape = (N, C, HW, 1)
    op = {k: rnd(torch.randn(shape, generator=g), dtype) for k in ('dy', 'c', 'a', 'b', 'e')}
    op['y'] = rnd(torch.randn(shape, generator=g) * 2, dtype)
    op['d'] = (torch.rand(N, C, generator=g) + 0.5).float().double()
    op['sa'] = (torch.rand(N, C, generator=g) + 0.5).float().double()
    op['sb'] = torch.randn(N, C, generator=g).float().double()
    return op


def _act_grad(v, y, act, alpha, gain, clamp):
    """bias_act's first-order gradient factor as the kernels apply it: v gain [alpha where not y > 0] and then
    ASSIGNED 0 where not -clamp < y < clamp (strict; a NaN y fails both comparisons, so it takes alpha and, with a
    clamp, gives exactly 0 whatever v holds).  -> (value, |value| with the same mask)."""
    alpha, gain, clamp = f32(alpha), f32(gain), f32(clamp)
    v, m = v * gain, v.abs() * abs(gain)
    if act == 1:
        pos = y > 0
        v, m = torch.where(pos, v, v * alpha), torch.where(pos, m, m * abs(alpha))
    if clamp >= 0:
        keep = (y > -clamp) & (y < clamp)
        v, m = torch.where(keep, v, torch.zeros_like(v)), torch.where(keep, m, torch.zeros_like(m))
    return v, m


def layer_bwd_ref(dy, y, c=None, d=None, act=1, alpha=0.2, gain=1.0, clamp=-1.0):
    """sg2_layer_bwd in float64 (operands float64 [N, C, H, W], d [N, C]): dz = act'(dy; y), dc = dz d, db = sum_{n,p}
    dz, dd = sum_p dz c, dnoise = sum_c dz, and under 'A_*' the same reductions of |terms|."""
    dz, mz = _act_grad(dy, y, act, alpha, gain, clamp)
    r = dict(dz=dz, dc=dz * d[:, :, None, None] if d is not None else dz, db=dz.sum([0, 2, 3]), A_db=mz.sum([0, 2, 3]),
             dnoise=dz.sum(1, keepdim=True), A_dnoise=mz.sum(1, keepdim=True))
    if c is not None:
        r['dd'], r['A_dd'] = (dz * c).sum([2, 3]), (mz * c.abs()).sum([2, 3])
    return r


def vjp_axpy_ref(a, sa=None, b=None, sb=None, y=None, act=0, alpha=0.2, gain=1.0, clamp=-1.0, e=None):
    """sg2_vjp_axpy in float64: out = act'(a sa + b sb; y) (act' only with y), dot = sum_p a e; 'mag' is the same
    expression of the operands' absolute values (what the f32 roundings before the output's own are relative to),
    'A_dot' the sum of |a e|."""
    v = a * (sa[:, :, None, None] if sa is not None else 1.0)
    m = v.abs()
    if b is not None:
        t = b * (sb[:, :, None, None] if sb is not None else 1.0)
        v, m = v + t, m + t.abs()
    if y is not None:
        v, _ = _act_grad(v, y, act, alpha, gain, clamp)
        m, _ = _act_grad(m, y, act, abs(alpha), abs(gain), clamp)
    r = dict(out=v, mag=m)
    if e is not None:
        r['dot'], r['A_dot'] = (a * e).sum([2, 3]), (a * e).abs().sum([2, 3])
    return r


def dot_hw_ref(a, b, dtype):
    """sg2_dot_hw in float64: sum_p round(a b), the product rounded to the operands' type as torch's `a * b` does
    (exact in f32 for 16-bit operands, so one rounding) -> (dot, the same sum of |terms|)."""
    t = (a.float() * b.float()).to(dtype).double()
    return t.sum([2, 3]), t.abs().sum([2, 3])


def det_sum_depth(S, n, G=1):
    """The longest chain of f32 additions through det.hip's det_sum over S slots of n outputs (G groups): four lane
    rows sum every fourth slot in order, ceil(S / 4) additions, the rows are added in order (4 with the zero start);
    few outputs over a long sum go through K chunks first (the same form twice).  The sequential form it takes at
    S <= 16 over many outputs is S additions.  One more for the final add into the output."""
    cdiv = lambda p, q: -(-p // q)      # noqa: E731
    bx = cdiv(n, 64)
    K = 1
    if bx * G < 512 and S > 64:
        K = min(cdiv(S, 64), 1024, cdiv(512, bx * G))
    if K > 1:
        chunk = cdiv(S, K)
        K = cdiv(S, chunk)
        return cdiv(chunk, 4) + 4 + cdiv(K, 4) + 4 + 1
    return max(cdiv(S, 4) + 4, S if S <= 16 else 0) + 1


def lb_depths(C, HW, N, det, passes=16):
    """The longest chain of f32 additions any contribution passes through, per output, read from layer_bwd.hip:

    per thread   a lane adds the pixels p0 + pl + k PPP of its workgroup into a register, k < passes: `passes` adds
                 (16 in layer_bwd_kernel and vjp_axpy_kernel, 32 in dot_hw_kernel; the U = 4 unroll keeps the order);
    workgroup    atomic mode: the PPP lanes of a channel atomicAdd into the LDS cell: PPP additions in any order;
                 deterministic mode: det_rows_sum adds the PPP rows in order: PPP additions;
    grid         db: one contribution per workgroup, gridDim.x N of them; dd and dot: gridDim.x per sample.  Atomic
                 mode: that many global atomicAdds (plus the memset's zero: no rounding); deterministic mode: det_sum
                 over that many slots (det_sum_depth), which also covers the add into a caller's accumulator;
    dnoise       never leaves the workgroup: 8 additions for the lane's channels, then log2 LP shuffle steps (LP a
                 power of two <= 64), else LP LDS atomicAdds, or LP ordered additions of the dn_part partials."""
    LP, PPP, ppb = lb_layout(C, passes)
    grid = -(-HW // min(HW, ppb))
    step = (lambda S, n: det_sum_depth(S, n)) if det else (lambda S, n: S + 1)
    shfl = LP & (LP - 1) == 0 and LP <= 64
    return dict(db=passes + PPP + step(grid * N, C), dd=passes + PPP + step(grid, N * C),
                dot=passes + PPP + step(grid, N * C), dnoise=8 + (LP.bit_length() - 1 if shfl else LP))


def layer_bwd_slack(ref, C, HW, N, det):
    """Judge 2 of sg2_layer_bwd -> slack per output.  dz = (dy gain) alpha: 2 f32 roundings; dc = dz d: a third, and
    that is all before the output's own rounding (for an f32 output the third IS the output's): gamma(3) |dc|.
    The reductions are f32 outputs: a term carries t roundings (dz: 2; dz c: 3, or 2 where the compiler contracts
    the product into an FMA) and then passes through `depth` additions (lb_depths), each rounding a partial sum that
    the same reduction of |terms|, A, bounds: gamma(t + depth) A."""
    dep = lb_depths(C, HW, N, det)
    s = dict(dc=gamma(3) * ref['dc'].abs(), db=gamma(2 + dep['db']) * ref['A_db'],
             dnoise=gamma(2 + dep['dnoise']) * ref['A_dnoise'])
    if 'dd' in ref:
        s['dd'] = gamma(3 + dep['dd']) * ref['A_dd']
    return s


def vjp_axpy_slack(ref, C, HW, N, det):
    """Judge 2 of sg2_vjp_axpy.  out: v = a sa (1 rounding), fmaf(b, sb, v) (1), v gain (1), v alpha (1): 4 f32
    roundings, each of a value that 'mag' (the expression of the absolute values) bounds, before the one rounding to
    the output type -- gamma(4) mag (for an f32 output the cast rounds nothing, so the four are all there is).
    dot: acc = fmaf(a, e, acc) -- the product is not rounded (t = 0), every addition is: gamma(depth) A."""
    s = dict(out=gamma(4) * ref['mag'])
    if 'dot' in ref:
        s['dot'] = gamma(lb_depths(C, HW, N, det)['dot']) * ref['A_dot']
    return s


def dot_hw_slack(A, C, HW, N, det):
    """Judge 2 of sg2_dot_hw: the terms are the rounded products (in the reference too: t = 0); 32 passes a lane."""
    return gamma(lb_depths(C, HW, N, det, passes=32)['dot']) * A


def lb_assert_exact(sums, elementwise):
    """The precondition of Judge 1, on the reference alone: sums = [(name, A)] with A the float64 sum of |terms| of a
    reduction -- A / quantum below 2^24, so every partial sum in any order is an f32 value; elementwise = [(name,
    float64 tensor)] -- every value survives a round trip through bf16 and fp16."""
    for name, A in sums:
        assert float(A.max()) / LB_QUANTUM < 2 ** 24, (name, float(A.max()))
        assert torch.equal(A / LB_QUANTUM, (A / LB_QUANTUM).round()), f'{name}: a term off the {LB_QUANTUM} grid'
    for name, v in elementwise:
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(v.to(dt).double(), v), f'{name}: not exact in {dt}'


def lb_judge_exact(got, ref, what):
    """Judge 1: every output of `got` (name -> tensor, any device / dtype) bitwise the float64 reference.  NaN never
    equals, so an element that was not stored fails too."""
    for k, v in got.items():
        g, r = _f64(v), ref[k]
        assert tuple(g.shape) == tuple(r.shape), (what, k, tuple(g.shape), tuple(r.shape))
        if not torch.equal(g, r):
            bad = (g != r).nonzero()
            at = tuple(bad[0].tolist())
            raise AssertionError(f'{what} {k}: {bad.shape[0]} of {g.numel()} elements differ from the exact reference, '
                                 f'first at {at}: got {g[at].item()!r}, ref {r[at].item()!r}; last at '
                                 f'{tuple(bad[-1].tolist())} (index order of shape {tuple(g.shape)})')


def lb_judge_bound(got, ref, slack, dtype, what):
    """Judge 2: every element of every output within its derived bound -> {name: worst error / bound}.  The
    elementwise outputs ('dc', 'out') are `dtype` values, the reductions f32."""
    return {k: assert_elementwise(v, ref[k], slack[k], dtype if k in ('dc', 'out') else torch.float32, f'{what} {k}')
            for k, v in got.items()}
