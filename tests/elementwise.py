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


# ------------------------------------------------------------------ the f32 conv routes (test_conv_f32_gpu.py)
# conv.hip runs an f32 convolution by default as a three-way bf16 split: x = h + m + l (split3 / split3x4: bf16
# round-to-nearest-even residuals), and the GEMM takes six of the nine plane products in mfma_s3's order, in-loop
# ('s3') or on planes sg2_split3 made once ('p3'); SG2_F32_EXACT=1 ('exact') takes the f32-input MFMA instead.
S3_ORDER = ('lh', 'hl', 'mm', 'mh', 'hm', 'hh')     # (plane of the A operand, plane of the B operand), as mfma_s3
S3_DROPPED = ('ml', 'lm', 'll')                      # never formed: below 2.02 2^-24 of a product together
_PLANE = dict(h=0, m=1, l=2)
CF_FORMS = ('s3', 'p3', 'exact')
CF_WS_LIMIT = 1 << 23                                 # conv2d_gradfix._WS_LIMIT: split-K only below it
CF_EXACT = dict(noise_gain=0.5, act=1, alpha=0.25, gain=2.0, clamp=64.0)      # the integer fixture's epilogue
CF_RANDOM = dict(noise_gain=0.3, act=1, alpha=0.2, gain=2.0 ** 0.5, clamp=2.5)
CF_WGRAD_ALPHA = dict(exact=0.25, random=0.7)
SK_ITERS = 16                                         # conv1x1_smallk_dot: pixel passes per workgroup


def cdiv(p, q):
    return -(-p // q)


def s3_split(x):
    """(h, m, l) as f32 tensors: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), every conversion
    round-to-nearest-even and every residual an exact f32 subtraction: what split3 / split3x4 do.  h + m + l == x
    for every normal f32 whose last bit is a normal bf16 value (|x| >= 2^-102)."""
    x = x.float()
    h = x.bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    r = r - m
    return h, m, r.bfloat16().float()


def s3_products(xs, ws, drop=None):
    """The plane products of mfma_s3 in its order (small terms first) as (name, A plane, B plane); `drop` leaves
    one out: the mutant that gives the plane fixtures teeth."""
    assert drop is None or drop in S3_ORDER, drop
    return [(n, xs[_PLANE[n[0]]], ws[_PLANE[n[1]]]) for n in S3_ORDER if n != drop]


def s3_matmul_emulated(X, W, drop=None, bk=32):
    """X [M, K] @ W [K, N] as the split kernels form it: per `bk`-deep K stage the six products in order, each
    one MFMA whose 32 bf16 products (exact in f32) are summed in float64 here and added to the f32 accumulator
    with one rounding.  (How an MFMA rounds inside is not documented; on the plane fixtures nothing rounds.)"""
    xs, ws = s3_split(X), s3_split(W)
    acc = torch.zeros(X.shape[0], W.shape[1], dtype=torch.float32)
    for k0 in range(0, X.shape[1], bk):
        for _, a, b in s3_products([p[:, k0:k0 + bk] for p in xs], [p[k0:k0 + bk] for p in ws], drop):
            acc = (acc.double() + a.double() @ b.double()).float()
    return acc


def cf_out_hw(k, stride, pad, transposed, H, W):
    if transposed:
        return (H - 1) * stride - 2 * pad + k, (W - 1) * stride - 2 * pad + k
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def conv_fwd_plan(k, stride, pad, transposed, N, Cin, H, W, Cout, form='s3', workspace=True, dot=False):
    """The host dispatch of sg2_conv2d_fused / launch_fwd for an f32 call, read from conv.hip (default
    SG2_CONV_SPLIT_WGS = 512; 16-byte aligned operands).  `workspace`: whether the wrapper passes one (it does below
    _WS_LIMIT output elements).  -> dict: family ('smallk', 'smallk_dot', 'generic'), OH, OW and, for the generic
    implicit GEMM, BM, BN, BK, vec, nck, live_last (channels of the last K stage that are < Cin), phases [(M, ntaps,
    nk)], splits, kper, grid, split_steps [phase][split] (K steps each split runs), empty [(phase, split)],
    early_return [(phase, M tile)], dot_depth(det) (the longest chain of f32 additions of the dot reduction)."""
    assert form in CF_FORMS
    OH, OW = cf_out_hw(k, stride, pad, transposed, H, W)
    P = OH * OW
    plan = dict(OH=OH, OW=OW, K=k * k * Cin, splits=1)
    if form != 'p3' and k == 1 and stride == 1 and pad == 0 and Cin <= 4 and Cout % 8 == 0 and 256 % (Cout // 8) == 0:
        OG = Cout // 8
        if dot:
            ppi = 256 // OG
            gx = cdiv(H * W, SK_ITERS * ppi)
            plan.update(family='smallk_dot', grid=(gx, N), ppi=ppi, last_wg_pixels=H * W - (gx - 1) * SK_ITERS * ppi,
                        dot_depth=lambda det: SK_ITERS + ppi + (det_sum_depth(gx, N * Cout) if det else gx + 1))
        else:
            plan.update(family='smallk', grid=(min(cdiv(N * H * W * OG, 256), 256 * 64),), items=N * H * W * OG)
        return plan
    # (conv1x1_smallo, the toRGB kernel, is 16-bit only: an f32 Cout <= 4 takes the implicit GEMM)
    BK = 16 if form == 'exact' else 32
    BM, BN = 128, 128 if Cout > 64 else 64
    nck = cdiv(Cin, BK)
    phases = []
    if not transposed:
        phases.append((N * OH * OW, k * k, k * k * nck))
    else:
        for py in range(stride):
            for px in range(stride):
                QH, QW = (OH - py + stride - 1) // stride, (OW - px + stride - 1) // stride
                if QH <= 0 or QW <= 0:
                    continue
                nt = sum(1 for ky in range(k) if (py + pad - ky) % stride == 0) * \
                    sum(1 for kx in range(k) if (px + pad - kx) % stride == 0)
                phases.append((N * QH * QW, nt, nt * nck))
    assert len(phases) <= 4, 'more than kMaxPhases: several launches (not modelled)'
    blocks = sum(cdiv(M, 128) * cdiv(Cout, BN) for M, _, _ in phases)
    maxnk = max([1] + [nk for _, _, nk in phases])
    splits = 1
    if blocks < 512 and workspace and N * P * Cout <= CF_WS_LIMIT:
        splits = max(1, min(cdiv(512, blocks), maxnk // 4))
    kper = cdiv(maxnk, splits)
    maxM = max(M for M, _, _ in phases)
    steps = [[max(0, min(nk, (s + 1) * kper) - s * kper) for s in range(splits)] for _, _, nk in phases]
    plan.update(family='generic', BM=BM, BN=BN, BK=BK, vec=form == 'p3' or Cin % 4 == 0, nck=nck,
                live_last=Cin - (nck - 1) * BK, phases=phases, splits=splits, kper=kper,
                grid=(cdiv(maxM, BM), cdiv(Cout, BN), len(phases) * splits), split_steps=steps,
                empty=[(p, s) for p in range(len(phases)) for s in range(splits) if steps[p][s] == 0],
                early_return=[(p, t) for p, (M, _, _) in enumerate(phases) for t in range(cdiv(maxM, BM))
                              if t * BM >= M],
                dot_depth=lambda det: (det_sum_depth(P, Cout, N) if det else P) + 1)
    return plan


def conv_wgrad_plan(A, B, k, stride, pad, N, OH, OW, form='s3'):
    """The host dispatch of conv2d_wgrad_impl / launch_wgrad for an f32 call (default SG2_CWGRAD_WGS = 1024; the
    halo weight gradient is 16-bit only) -> dict: family ('smallb', 'smalla', 'generic'), K = N OH OW; generic: BM,
    BN, BK, vec, tiles (mt, nt), chunks, splits, kper (pixels per split), split_pixels, grid; small forms: grid,
    rows (deterministic slots), lanes (lanes a workgroup adds into one LDS cell).  depth(det, oikk): the additions
    that follow a workgroup's own partial sum (atomics: one per split; det_sum / det_sum_oikk over the slots)."""
    assert form in CF_FORMS
    M = N * OH * OW
    plan = dict(K=M)
    one = k == 1 and stride == 1 and pad == 0
    for fam, small, wide in (('smallb', B, A), ('smalla', A, B)):
        if form != 'p3' and one and small <= 4 and wide % 8 == 0 and 256 % (wide // 8) == 0 and A * B <= 2048:
            OG = wide // 8
            g = min(cdiv(M * OG, 256), 1024)
            rows = g * 256 // OG
            plan.update(family=fam, grid=(g,), rows=rows, lanes=256 // OG, items=M * OG, splits=g,
                        depth=lambda det, oikk=False: det_sum_depth(rows, A * B) if det else 256 // OG + g + 1)
            return plan
    BK = 16 if form == 'exact' else 32
    BM, BN = 128 if A > 64 else 64, 128 if B > 64 else 64
    mt, nt, KK = cdiv(A, BM), cdiv(B, BN), k * k
    chunks = cdiv(M, BK)
    splits = max(1, min(chunks // 8, cdiv(1024, mt * nt * KK)))
    kper = cdiv(chunks, splits) * BK
    splits = cdiv(M, kper)
    nel = A * KK * B
    plan.update(family='generic', BM=BM, BN=BN, BK=BK, vec=form == 'p3' or (A % 4 == 0 and B % 4 == 0),
                tiles=(mt, nt), chunks=chunks, splits=splits, kper=kper, grid=(mt, nt, KK * splits),
                split_pixels=[min(M, (s + 1) * kper) - s * kper for s in range(splits)],
                depth=lambda det, oikk=False: (splits if oikk else det_sum_depth(splits, nel)) if det else splits + 1)
    return plan


# the case tables: the smallest shapes that reach each edge (test_conv_f32_host.py asserts that they do)
CF_FWD_CASES = {        # name -> k, stride, pad, transposed, N, Cin, H, W, Cout
    'f3': (3, 1, 1, False, 3, 40, 7, 7, 40),
    'f3w': (3, 1, 1, False, 2, 8, 5, 6, 136),
    'f1': (1, 1, 0, False, 3, 72, 7, 7, 24),
    'f1d': (1, 1, 0, False, 2, 264, 4, 4, 72),
    'fd': (3, 2, 0, False, 2, 16, 9, 9, 24),
    'fu': (3, 2, 0, True, 4, 64, 5, 6, 24),
    'f1t': (1, 1, 0, True, 2, 24, 6, 6, 40),
    'fn': (3, 1, 1, False, 2, 13, 5, 5, 20),
    'frgb1': (1, 1, 0, False, 2, 64, 6, 6, 1),
    'frgb3': (1, 1, 0, False, 2, 64, 6, 6, 3),
    'fk1_8': (1, 1, 0, False, 3, 1, 7, 7, 8),
    'fk1_64': (1, 1, 0, False, 3, 1, 7, 7, 64),
    'fk3_8': (1, 1, 0, False, 3, 3, 7, 7, 8),
    'fk3_64': (1, 1, 0, False, 3, 3, 7, 7, 64),
    'fk40': (1, 1, 0, False, 3, 3, 7, 7, 40),
}
CF_WGRAD_CASES = {      # name -> A, B, k, stride, pad, N, OH, OW
    'w3': (40, 40, 3, 1, 1, 3, 7, 7),
    'wA': (136, 8, 3, 1, 1, 2, 14, 20),
    'wB': (8, 136, 3, 1, 1, 2, 14, 20),
    'wAB': (72, 72, 3, 1, 1, 2, 6, 6),
    'wd': (24, 16, 3, 2, 0, 2, 4, 4),
    'w1': (24, 72, 1, 1, 0, 3, 7, 7),
    'wn': (20, 13, 3, 1, 1, 2, 5, 5),
    'wsb8_1': (8, 1, 1, 1, 0, 3, 7, 7),
    'wsb64_1': (64, 1, 1, 1, 0, 3, 7, 7),
    'wsb8_3': (8, 3, 1, 1, 0, 3, 7, 7),
    'wsb64_3': (64, 3, 1, 1, 0, 3, 7, 7),
    'wsa1_8': (1, 8, 1, 1, 0, 3, 7, 7),
    'wsa1_64': (1, 64, 1, 1, 0, 3, 7, 7),
    'wsa3_8': (3, 8, 1, 1, 0, 3, 7, 7),
    'wsa3_64': (3, 64, 1, 1, 0, 3, 7, 7),
}
CF_PLANE_FWD, CF_PLANE_WGRAD = ('f1', 'f3'), ('w1', 'w3')
CF_PLANE_FIXTURES = {'x24': ('lh', 'mh', 'hh'), 'w24': ('hl', 'hm', 'hh'), 'mm': ('mm', 'mh', 'hm', 'hh')}


def cf_forms(cin_or_ab, wgrad_1x1_small=False):
    """The arithmetic forms a case admits: 'p3' where conv2d_gradfix._p3 holds (every channel count % 8 == 0, and
    for dw not the 1x1 small-depth kernels)."""
    cs = cin_or_ab if isinstance(cin_or_ab, tuple) else (cin_or_ab,)
    p3 = all(c % 8 == 0 for c in cs) and not wgrad_1x1_small
    return ('s3', 'p3', 'exact') if p3 else ('s3', 'exact')


def cf_wgrad_x_hw(k, stride, pad, OH, OW):
    """The smallest input that gives an OH x OW gradient."""
    return (OH - 1) * stride + k - 2 * pad, (OW - 1) * stride + k - 2 * pad


def cf_pack(w, transposed):
    """The packed weight [Cout][kh][kw][Cin] of w [Cout, Cin, kh, kw] (transposed: [Cin, Cout, kh, kw]) as a torch
    permutation (conv2d_gradfix._pack_conv / _pack_convT without the pack kernel)."""
    return (w.permute(1, 2, 3, 0) if transposed else w.permute(0, 2, 3, 1)).contiguous()


def _cf_gen(name, *ints):
    seed = sum((j + 1) * 7919 ** j * (int(v) + 3) for j, v in enumerate(ints))
    return torch.Generator().manual_seed((seed + sum(map(ord, name)) * 104729) % (2 ** 31 - 1))


def _ints(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).double()


def _pow2(g, lo, hi, *s):
    return 2.0 ** _ints(g, lo, hi, *s)


def _wshape(k, transposed, Cin, Cout):
    return (Cin, Cout, k, k) if transposed else (Cout, Cin, k, k)


def cf_fwd_operands(case, kind):
    """Operands of a forward case as float64 (every value an f32 value).  kind 'exact': the integer fixture --
    |x|, |w| <= 4, scales 2^-1..2^1, integer bias / noise / residual / dot_src (with CF_EXACT: noise_gain 0.5, alpha
    0.25, gain 2, a clamp on the value grid) -- every product and partial sum is a multiple of 1/16 far below 2^24
    quanta (cf_fwd_exact_refs asserts it), so all three arithmetic forms are exact in any order.  kind 'random': seeded
    normals, w scaled by K^-1/2, scales in [0.5, 1.5)."""
    k, stride, pad, tr, N, Cin, H, W, Cout = case
    OH, OW = cf_out_hw(k, stride, pad, tr, H, W)
    g = _cf_gen(kind, *[int(v) for v in case])
    out = (N, Cout, OH, OW)
    if kind == 'exact':
        return dict(x=_ints(g, -4, 4, N, Cin, H, W), w=_ints(g, -4, 4, *_wshape(k, tr, Cin, Cout)),
                    in_scale=_pow2(g, -1, 1, N, Cin), out_scale=_pow2(g, -1, 1, N, Cout),
                    noise=_ints(g, -8, 8, N, 1, OH, OW), bias=_ints(g, -8, 8, Cout), residual=_ints(g, -8, 8, *out),
                    dot_src=_ints(g, -4, 4, *out))

    def rn(*s):
        return torch.randn(*s, generator=g).float().double()
    w = (torch.randn(*_wshape(k, tr, Cin, Cout), generator=g) / (k * k * Cin) ** 0.5).float().double()
    return dict(x=rn(N, Cin, H, W), w=w,
                in_scale=(torch.rand(N, Cin, generator=g) + 0.5).float().double(),
                out_scale=(torch.rand(N, Cout, generator=g) + 0.5).float().double(),
                noise=rn(N, 1, OH, OW), bias=rn(Cout), residual=rn(*out), dot_src=rn(*out))


def _cf_conv(x, w, case):
    k, stride, pad, tr = case[:4]
    return (F.conv_transpose2d if tr else F.conv2d)(x, w, stride=stride, padding=pad)


def conv_f32_slack(form, K, S, A):
    """The absolute error an f32 conv route may carry in a sum of K products whose |.| sum is A (float64), reduced
    over S further additions (split-K atomics or slots, det_sum's chain).
    s3 / p3: (3 + 2 (6 K + S + 1)) 2^-24 A.  The 3: the three plane products that are never formed, m l' + l m' +
    l l' with |m| <= 2^-8 |x| and |l| <= 2^-16 |x|: below 2.02 2^-24 per product.  6 K: one f32 addition per plane
    product that is formed (the bf16 products themselves are exact in f32), S + 1 the additions after the
    workgroup's own sum; the factor 2 is accumulation_slack's allowance for an MFMA accumulator that truncates.
    exact: 2 (K + S + 1) 2^-24 A: one rounding per f32 product-and-add.
    A modulated operand is rounded where the kernel rounds it (__fmul_rn in sstore and in split3_kernel) by the
    reference itself, so it carries no slack."""
    n = 3 + 2 * (6 * K + S + 1) if form in ('s3', 'p3') else 2 * (K + S + 1)
    return n * EPS32 * A


def cf_fwd_ref(case, op, form, S, dot_depth, epi=None, in_scale=False, out_scale=False, noise=False, bias=False,
               residual=False, aux_mode=0, dot=False):
    """sg2_conv2d_fused in float64 with its Judge 2 slack -> dict(c, A, y, aux, dot and slack_*).  c = conv(x *
    in_scale, w) with the product rounded to f32 as the kernels stage it; v = clamp(lrelu(c out_scale + noise g +
    bias) gain) through epilogue_slack; y = v + residual is one more f32 rounding; aux = c (mode 1) or v (mode 2);
    dot[n, o] = sum_p c src: |src| slack_c plus one rounding of each product and `dot_depth` additions."""
    x = op['x']
    if in_scale:
        x = (x.float() * op['in_scale'].float()[:, :, None, None]).double()
    c, A = _cf_conv(x, op['w'], case), _cf_conv(x.abs(), op['w'].abs(), case)
    sc = conv_f32_slack(form, case[0] * case[0] * case[5], S, A)
    r = dict(c=c, A=A, slack_c=sc, y=c, slack_y=sc)
    if epi is not None:
        d = op['out_scale'][:, :, None, None] if out_scale else torch.ones(())
        ng = op['noise'] * f32(epi['noise_gain']) if noise else torch.zeros(())
        b = op['bias'][None, :, None, None] if bias else torch.zeros(())
        al, gn, cl = f32(epi['alpha']) if epi['act'] == 1 else 1.0, f32(epi['gain']), f32(epi['clamp'])
        v = c * d + ng + b
        v = torch.where(v > 0, v, v * al) * gn
        if cl >= 0:
            v = v.clamp(-cl, cl)
        sv = epilogue_slack(sc, c, d, ng, b, abs(gn), abs(al))
        r.update(v=v, slack_v=sv, y=v, slack_y=sv)
        if residual:
            r['y'] = v + op['residual']
            r['slack_y'] = sv + EPS32 * r['y'].abs()
        if aux_mode:
            r['aux'], r['slack_aux'] = (c, sc) if aux_mode == 1 else (v, sv)
    if dot:
        src = op['dot_src']
        r['dot'] = (c * src).sum([2, 3])
        r['A_dot'] = (A * src.abs()).sum([2, 3])
        r['slack_dot'] = (sc * src.abs()).sum([2, 3]) + gamma(1 + dot_depth) * ((c.abs() + sc) * src.abs()).sum([2, 3])
    return r


def cf_assert_exact(sums, quantum=1.0 / 16):
    """The precondition of Judge 1 on the reference alone (as lb_assert_exact): sums = [(name, A, values)], A the
    float64 sum of |terms| -- below 2^24 quanta, so every partial sum in any order and in any of the three
    arithmetic forms is an f32 value -- and `values` (the outputs) on the quantum's grid."""
    for name, A, v in sums:
        assert float(A.max()) / quantum < 2 ** 24, (name, float(A.max()))
        assert torch.equal(v / quantum, (v / quantum).round()), f'{name}: a value off the {quantum} grid'
        assert torch.equal(v.float().double(), v), name


def cf_fwd_exact_refs(case):
    """The integer fixture's references for a forward case: plain, the full epilogue with aux_mode 2, and (aux_mode
    1) with the dot -- with the precondition asserted.  Every bound that matters is on a sum of |terms|: the conv
    sum A (quantum 1/2), the epilogue value (|c d| + |noise g| + |b|) gain + |residual| (quantum 1/16) and the dot's
    sum_p A |src|."""
    op = cf_fwd_operands(case, 'exact')
    full = dict(epi=CF_EXACT, in_scale=True, out_scale=True, noise=True, bias=True, residual=True)
    refs = dict(plain=cf_fwd_ref(case, op, 's3', 1, 1), full=cf_fwd_ref(case, op, 's3', 1, 1, aux_mode=2, **full),
                dot=cf_fwd_ref(case, op, 's3', 1, 1, aux_mode=1, dot=True, **full))     # (the slacks go unused)
    for name, r in refs.items():
        sums = [(f'{name} c', r['A'], r['c']), (f'{name} y', r['y'].abs(), r['y'])]
        if 'v' in r:
            mag = (r['A'] * op['out_scale'][:, :, None, None] + (op['noise'] * CF_EXACT['noise_gain']).abs() +
                   op['bias'].abs()[None, :, None, None]) * CF_EXACT['gain'] + op['residual'].abs()
            sums.append((f'{name} v', mag, r['v']))
        if 'dot' in r:
            sums.append((f'{name} dot', r['A_dot'], r['dot']))
        cf_assert_exact(sums)
    return op, refs


def cf_wgrad_operands(case, kind):
    """g [N, A, OH, OW], x [N, B, H, W], g_scale [N, A], x_scale [N, B] as float64; 'exact': integers |.| <= 4 and
    scales 2^-1..2^1 (alpha 0.25: every term a multiple of 1/16), 'random': normals, scales in [0.5, 1.5)."""
    A, B, k, stride, pad, N, OH, OW = case
    H, W = cf_wgrad_x_hw(k, stride, pad, OH, OW)
    g = _cf_gen('w' + kind, *case)
    if kind == 'exact':
        return dict(g=_ints(g, -4, 4, N, A, OH, OW), x=_ints(g, -4, 4, N, B, H, W), g_scale=_pow2(g, -1, 1, N, A),
                    x_scale=_pow2(g, -1, 1, N, B))
    return dict(g=torch.randn(N, A, OH, OW, generator=g).float().double(),
                x=torch.randn(N, B, H, W, generator=g).float().double(),
                g_scale=(torch.rand(N, A, generator=g) + 0.5).float().double(),
                x_scale=(torch.rand(N, B, generator=g) + 0.5).float().double())


def cf_wgrad_ref(case, op, form, S, scaled, alpha):
    """sg2_conv2d_wgrad in float64 -> (dw [A, B, k, k], sum of |terms|, slack): both operands modulated with the
    product rounded to f32 (as the kernels' sstore and split3_kernel), K = N OH OW products per element through
    conv_f32_slack, and alpha applied to each workgroup's partial sum: one more f32 rounding of values whose |.|
    sums to at most |alpha| A."""
    A, B, k, stride, pad, N, OH, OW = case
    g, x = op['g'], op['x']
    if scaled:
        g = (g.float() * op['g_scale'].float()[:, :, None, None]).double()
        x = (x.float() * op['x_scale'].float()[:, :, None, None]).double()
    al = f32(alpha)
    kw = dict(stride=stride, padding=pad)
    dw = torch.nn.grad.conv2d_weight(x, (A, B, k, k), g, **kw) * al
    mag = torch.nn.grad.conv2d_weight(x.abs(), (A, B, k, k), g.abs(), **kw) * abs(al)
    return dw, mag, conv_f32_slack(form, N * OH * OW, S, mag) + (EPS32 * mag if al != 1.0 else 0.0)


def cf_wgrad_exact_refs(case):
    """The integer fixture's dw references, with both scales and alpha and with none; the precondition asserted."""
    op = cf_wgrad_operands(case, 'exact')
    refs = {}
    for name, scaled, alpha in (('scaled', True, CF_WGRAD_ALPHA['exact']), ('plain', False, 1.0)):
        dw, mag, _ = cf_wgrad_ref(case, op, 's3', 1, scaled, alpha)
        cf_assert_exact([(f'dw {name}', mag / min(alpha, 1.0), dw)])      # (the partial sums before alpha)
        refs[name] = dw
    return op, refs


# ---- the plane fixtures: every output has at most one nonzero product and the float64 result is an f32 value, so
# the six-product scheme is exact and every product class a fixture needs is load-bearing
def cf_plane_values(kind, role, g, *s):
    """role 'a' (the GEMM's A operand: x of a forward conv, g of a weight gradient) or 'b' (w; x of a dw)."""
    n = 1
    for v in s:
        n *= v
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    if kind == 'mm':        # 1 + q 2^-11, q odd <= 15: h + m with l = 0; a product is a multiple of 2^-22 below 2
        v = 1 + (torch.randint(0, 8, (n,), generator=g) * 2 + 1).double() * 2.0 ** -11
    elif (kind == 'x24') == (role == 'a'):      # 24 significant bits (the last one set), random sign
        v = sign * ((torch.randint(0, 2 ** 22, (n,), generator=g) * 2 + 1).double() * 2.0 ** -23 + 1)
    else:                   # +-2^k: one plane, so the partner's h, m and l each meet it once
        v = sign * 2.0 ** torch.randint(-3, 4, (n,), generator=g).double()
    return v.view(*s)


def cf_plane_fwd_operands(case, kind, sparse):
    """(x, w) of a plane fixture for a forward case (float64).  sparse 'a': x nonzero in one channel per pixel (1x1)
    or on an every-third-pixel lattice, one channel per lattice point (3x3, stride 1), against a dense w; sparse
    'b': w a one-hot (c, ky, kx) per output channel against a dense x."""
    k, stride, pad, tr, N, Cin, H, W, Cout = case
    assert stride == 1 and not tr and k in (1, 3)
    g = _cf_gen(kind + sparse, *[int(v) for v in case])
    x = cf_plane_values(kind, 'a', g, N, Cin, H, W)
    w = cf_plane_values(kind, 'b', g, Cout, Cin, k, k)
    if sparse == 'a':
        keep = torch.zeros(N, Cin, H, W, dtype=torch.bool)
        ch = torch.randint(0, Cin, (N, H, W), generator=g)
        keep.scatter_(1, ch[:, None], True)
        if k == 3:
            lat = torch.zeros(H, W, dtype=torch.bool)
            lat[1::3, 1::3] = True
            keep &= lat
        x = x * keep
    else:
        keep = torch.zeros(Cout, Cin * k * k, dtype=torch.bool)
        keep.scatter_(1, torch.randint(0, Cin * k * k, (Cout, 1), generator=g), True)
        w = w * keep.view(Cout, Cin, k, k)
    return x, w


def cf_plane_wgrad_operands(case, kind, sparse):
    """(g, x) of a plane fixture for a weight-gradient case: the sparse operand ('a': g, 'b': x) is nonzero at one
    pixel of one sample per channel, the other one dense."""
    A, B, k, stride, pad, N, OH, OW = case
    H, W = cf_wgrad_x_hw(k, stride, pad, OH, OW)
    rng = _cf_gen('w' + kind + sparse, *case)
    g = cf_plane_values(kind, 'a', rng, N, A, OH, OW)
    x = cf_plane_values(kind, 'b', rng, N, B, H, W)
    t, C, hw = (g, A, OH * OW) if sparse == 'a' else (x, B, H * W)
    keep = torch.zeros(C, N * hw, dtype=torch.bool)
    keep.scatter_(1, torch.randint(0, N * hw, (C, 1), generator=rng), True)
    keep = keep.view(C, N, *t.shape[2:]).transpose(0, 1)
    return (g * keep, x) if sparse == 'a' else (g, x * keep)


def cf_plane_assert_one_term(terms, ref, what):
    """terms: the number of nonzero products per output (the same operation on the operands' nonzero masks); ref:
    the float64 result -- at most one product each, every result an f32 value, and a fair share of the outputs nonzero."""
    assert float(terms.max()) <= 1, (what, float(terms.max()))
    assert torch.equal(ref.float().double(), ref), what
    assert float((ref != 0).double().mean()) > 0.05, what


# ------------------------------------------------------------------ bias_act (test_bias_act_gpu.py, test_bias_act_host.py)
# csrc/bias_act.hip: one flat index over the dense tensor, a 16-byte vector (V elements) per lane per trip, a masked
# tail vector when numel % V != 0, a grid capped at 256 * 16 workgroups of 256 lanes (BA_SWEEP vectors a sweep), the
# bias at ((base + j) / step_b) % size_b.  The arithmetic is f32 throughout and rounds once, at the store.
BA_V = {torch.float32: 4, torch.float16: 8, torch.bfloat16: 8}
BA_SWEEP = 256 * 16 * 256                   # vectors per sweep of the capped grid: 1,048,576
BA_SPEC = {     # name -> (default alpha, default gain, what the gradient is expressed through, has a 2nd-order term)
    'linear': (0.0, 1.0, '', False), 'relu': (0.0, 2.0 ** 0.5, 'y', False), 'lrelu': (0.2, 2.0 ** 0.5, 'y', False),
    'tanh': (0.0, 1.0, 'y', True), 'sigmoid': (0.0, 1.0, 'y', True), 'elu': (0.0, 1.0, 'y', True),
    'selu': (0.0, 1.0, 'y', True), 'softplus': (0.0, 1.0, 'y', True), 'swish': (0.0, 2.0 ** 0.5, 'x', True),
}
BA_SELU_SCALE = f32(1.0507009873554804934193349852946)
BA_SELU_ALPHA = f32(1.6732632423543772848170429916717)
BA_SELU_SA = float(torch.tensor(BA_SELU_SCALE, dtype=torch.float32) * torch.tensor(BA_SELU_ALPHA, dtype=torch.float32))
BA_EXP_HW_ULPS = 4          # (2 |x| + 4) 2^-24: twice the documented 1 ulp (2 2^-24) of the hardware exp2
BA_TANH_ULPS = 5            # OCML tanh, OpenCL full profile; 1 ulp = 2^-23 relative
BA_LOG1P_ULPS = 2           # OCML log1p, OpenCL full profile
BA_EXACT = dict(alpha=0.25, gain=2.0, clamp=2.5)


def _c(v):
    """A constant as a (value, error) pair."""
    return torch.as_tensor(v, dtype=torch.float64), torch.zeros((), dtype=torch.float64)


def _z(t):
    """An operand (exact) as a (value, error) pair."""
    return t, torch.zeros_like(t)


def _ba_neg(a):
    return -a[0], a[1]


def _ba_add(a, b):
    """fl(a + b): the operands' errors, and one rounding of a sum that the TERMS' magnitudes bound (so the bound
    stays absolute where the sum cancels: exp(v) - 1, 1 - exp(-yy), 1 - yy yy)."""
    (va, ea), (vb, eb) = a, b
    return va + vb, ea + eb + EPS32 * (va.abs() + vb.abs() + ea + eb)


def _ba_mul(a, b):
    (va, ea), (vb, eb) = a, b
    v = va * vb
    p = va.abs() * eb + vb.abs() * ea + ea * eb
    return v, p + EPS32 * (v.abs() + p)


def _ba_div(a, b):
    """fl(a / b), correctly rounded (the kernel's divisions compile to the IEEE sequence, not to a bare reciprocal):
    |a' / b' - a / b| <= (ea + |a / b| eb) / |b'| with |b'| >= |b| - eb."""
    (va, ea), (vb, eb) = a, b
    v = va / vb
    p = (ea + v.abs() * eb) / (vb.abs() - eb)
    return v, p + EPS32 * (v.abs() + p)


def _ba_exp(a):
    """__expf(x) = exp2(fl(log2e_f32 x)) on the hardware: the rounded product and the rounded constant each move
    the argument by up to 2^-24 |x log2e|, i.e. 2 2^-24 |x| relative in the result, the instruction is specified to
    1 ulp = 2 2^-24 and is allowed twice that here (BA_EXP_HW_ULPS): (2 |x| + 4) 2^-24 relative, plus 2^-126 for a
    result flushed from the denormal range; an argument error ea stretches the value by exp(ea) - 1."""
    v = torch.exp(a[0])
    p = v * torch.expm1(a[1])
    return v, p + (2 * a[0].abs() + BA_EXP_HW_ULPS) * EPS32 * (v + p) + 2.0 ** -126


def _ba_where(c, a, b):
    return torch.where(c, a[0], b[0]), torch.where(c, a[1], b[1])


def _ba_cut(v, cut, hi, lo, ge=False):
    """A branch on a COMPUTED value v = (value, error) at `cut`: float64's side, and where v is within its error of
    the cut -- where the kernel's f32 value may fall on the other side -- both sides' errors plus their distance."""
    c = (v[0] >= cut) if ge else (v[0] > cut)
    r = _ba_where(c, hi, lo)
    near = (v[0] - cut).abs() <= v[1]
    return r[0], torch.where(near, hi[1] + lo[1] + (hi[0] - lo[0]).abs(), r[1])


def _ba_act(act, v, alpha):
    """act_fwd<ACT> on a (value, error) pair."""
    one = _c(1.0)
    if act == 'linear':
        return v
    if act == 'relu':
        return _ba_cut(v, 0.0, v, _c(0.0))
    if act == 'lrelu':
        return _ba_cut(v, 0.0, v, _ba_mul(v, _c(alpha)))
    if act == 'tanh':       # 1-Lipschitz, then the library's own error
        t = torch.tanh(v[0])
        return t, v[1] + BA_TANH_ULPS * 2 * EPS32 * t.abs()
    if act == 'sigmoid':
        return _ba_div(one, _ba_add(one, _ba_exp(_ba_neg(v))))
    if act == 'elu':
        return _ba_cut(v, 0.0, v, _ba_add(_ba_exp(v), _c(-1.0)), ge=True)
    if act == 'selu':
        return _ba_cut(v, 0.0, _ba_mul(_c(BA_SELU_SCALE), v),
                       _ba_mul(_c(BA_SELU_SA), _ba_add(_ba_exp(v), _c(-1.0))), ge=True)
    if act == 'softplus':   # log1p is 1 / (1 + t)-Lipschitz at t >= 0, then the library's own error
        t = _ba_exp(v)
        lg = torch.log1p(t[0])
        lo = lg, t[1] / (1 + (t[0] - t[1]).clamp(min=0)) + BA_LOG1P_ULPS * 2 * EPS32 * lg.abs()
        return _ba_cut(v, 20.0, v, lo)
    assert act == 'swish', act
    return _ba_div(v, _ba_add(one, _ba_exp(_ba_neg(v))))


def _ba_d1(act, g, yy, xs, alpha):
    """act_d1<ACT>: the branches on yy take yy's SIGN, which is the stored yref's (one exact-sign product)."""
    one = _c(1.0)
    pos, nn = yy[0] > 0, yy[0] >= 0             # a NaN yy fails both, as in the kernel
    if act == 'linear':
        return g
    if act == 'relu':
        return _ba_where(pos, g, _c(0.0))
    if act == 'lrelu':
        return _ba_where(pos, g, _ba_mul(g, _c(alpha)))
    if act == 'tanh':
        return _ba_mul(g, _ba_add(one, _ba_neg(_ba_mul(yy, yy))))
    if act == 'sigmoid':
        return _ba_mul(_ba_mul(g, yy), _ba_add(one, _ba_neg(yy)))
    if act == 'elu':
        return _ba_where(nn, g, _ba_mul(g, _ba_add(yy, one)))
    if act == 'selu':
        return _ba_where(nn, _ba_mul(g, _c(BA_SELU_SCALE)), _ba_mul(g, _ba_add(yy, _c(BA_SELU_SA))))
    if act == 'softplus':
        return _ba_mul(g, _ba_add(one, _ba_neg(_ba_exp(_ba_neg(yy)))))
    assert act == 'swish', act
    e = _ba_exp(xs)
    d = _ba_add(e, one)
    return _ba_cut(xs, 40.0, g, _ba_div(_ba_mul(_ba_mul(g, e), _ba_add(xs, d)), _ba_mul(d, d)))


def _ba_d2(act, g, yy, xs):
    """act_d2<ACT>."""
    one, two, zero = _c(1.0), _c(2.0), _c(0.0)
    nn = yy[0] >= 0
    if act == 'tanh':
        return _ba_mul(_ba_mul(g, _ba_add(one, _ba_neg(_ba_mul(yy, yy)))), _ba_mul(_c(-2.0), yy))
    if act == 'sigmoid':
        return _ba_mul(_ba_mul(_ba_mul(g, yy), _ba_add(one, _ba_neg(yy))), _ba_add(one, _ba_neg(_ba_mul(two, yy))))
    if act == 'elu':
        return _ba_where(nn, zero, _ba_mul(g, _ba_add(yy, one)))
    if act == 'selu':
        return _ba_where(nn, zero, _ba_mul(g, _ba_add(yy, _c(BA_SELU_SA))))
    if act == 'softplus':
        e = _ba_exp(_ba_neg(yy))
        return _ba_mul(_ba_mul(g, e), _ba_add(one, _ba_neg(e)))
    if act == 'swish':
        e = _ba_exp(xs)
        d = _ba_add(e, one)
        num = _ba_add(_ba_mul(xs, _ba_add(two, _ba_neg(d))), _ba_mul(two, d))
        return _ba_cut(xs, 40.0, zero, _ba_div(_ba_mul(_ba_mul(g, e), num), _ba_mul(_ba_mul(d, d), d)))
    return _ba_where(nn, zero, zero)            # linear, relu, lrelu: 0 of yy's shape


def ba_bias(b, x, dim):
    """The bias as it meets x: a 1-D b along `dim`, or (the host mutants' misindexed bias) one value per element."""
    if b is None or b.dim() == x.dim():
        return b
    shape = [1] * x.dim()
    shape[dim] = -1
    return b.reshape(shape)


def bias_act_ref(grad, act, x, b=None, xref=None, yref=None, dy=None, dim=1, alpha=None, gain=None, clamp=None,
                 dtype=torch.float32):
    """bias_act_kernel<T, ACT, GRAD> in float64 -> (ref, slack).  Operands: float64 tensors holding `dtype` values,
    named as the KERNEL names them (at grad 1 `x` is the incoming gradient and `xref`, `yref` the saved forward
    tensors; at grad 2 `x` is the gradient of dx and `dy` the first-order incoming gradient); alpha, gain and clamp
    are taken at their f32 values; clamp None or negative: no clamp.  Never autograd, never a product wrapper.

    Mirrored from the kernel: v = x + b at grad 0 and xs = xref + b at the gradients (a missing operand is 0 there
    and dy is 1); yy = yref inv_gain with inv_gain = fl(1 / gain), 0 for gain 0; for swish yref is RECOMPUTED from xs
    (act_fwd<9>(xs) gain) and the stored one ignored; the derivative formulas as written (tanh, sigmoid, elu, selu,
    softplus through yy; swish through xs with its cut-offs at 40; softplus' forward cut-off at 20); then gain, then
    dy; the clamp mask is ASSIGNED last, strict (-clamp < yref < clamp) and false for a NaN yref; the forward clamp
    is fmin(fmax(r, -clamp), clamp), which sends NaN to -clamp.  The one rounding to `dtype` at the store is
    assert_elementwise's own u |ref| term.

    slack is the absolute f32 error before that rounding, carried through the kernel's operations one by one as
    (value, error) pairs: an f32 add, product or division rounds once, 2^-24 of a magnitude that the operands'
    absolute values (plus their errors) bound -- k operations in a row give gamma(k) of the expression of absolute
    values -- so a difference that cancels keeps an ABSOLUTE bound of the size of its terms; an intermediate's
    error passes on at the next step's Lipschitz factor (|other factor| through a product, 1 / |denominator| through
    a division, exp(e) - 1 through exp, <= 1 through tanh and log1p, and through a clamp that it cannot leave: 0);
    __expf per _ba_exp, tanhf BA_TANH_ULPS and log1pf BA_LOG1P_ULPS ulp of 2^-23.  A product the compiler contracts
    into an FMA rounds less, never more.  A branch on a computed value (v > 0, v > 20, xs > 40) takes float64's
    side and, where the value is within its own error of the cut, both sides' errors plus their distance (_ba_cut);
    a branch on yy takes the sign of the stored yref and cannot flip.  None of the constants is fitted to a run."""
    spec = BA_SPEC[act]
    alpha = f32(spec[0] if alpha is None else alpha)
    gain = f32(spec[1] if gain is None else gain)
    clamp = f32(clamp) if clamp is not None and clamp >= 0 else None
    if dtype != torch.float64 and x.numel() < (1 << 20):    # (float64: the host's comparison with autograd)
        for t in (x, b, xref, yref, dy):
            assert t is None or torch.equal(rnd(t, dtype).nan_to_num(0.5), t.nan_to_num(0.5)), 'operand not rounded'
    bb = ba_bias(b, x, dim)
    if grad == 0:
        v = _ba_add(_z(x), _z(bb)) if bb is not None else _z(x)
        r = _ba_mul(_ba_act(act, v, alpha), _c(gain))
        if clamp is not None:
            nan = r[0].isnan()
            val = torch.where(nan, torch.full_like(r[0], -clamp), r[0].clamp(-clamp, clamp))
            r = val, torch.where(nan | (r[0].abs() - r[1] > clamp), torch.zeros_like(r[1]), r[1])
        return r
    assert grad in (1, 2), grad
    one32 = torch.tensor(1.0, dtype=torch.float32)
    inv_gain = float(one32 / torch.tensor(gain, dtype=torch.float32)) if gain != 0 else 0.0
    zero = torch.zeros_like(x)
    if xref is not None and bb is not None:
        xs = _ba_add(_z(xref), _z(bb.expand_as(x) if bb.dim() == x.dim() else bb))
    else:
        xs = _z(xref if xref is not None else (bb + zero if bb is not None else zero))
    if act == 'swish':
        yr = _ba_mul(_ba_act('swish', xs, 0.0), _c(gain))
    else:
        yr = _z(yref if yref is not None else zero)
    yy = _ba_mul(yr, _c(inv_gain))
    r = _ba_d1(act, _z(x), yy, xs, alpha) if grad == 1 else _ba_d2(act, _z(x), yy, xs)
    r = _ba_mul(r, _c(gain))
    if dy is not None:
        r = _ba_mul(r, _z(dy))
    r = r[0] + zero, r[1] + zero
    if clamp is not None:
        keep = (yr[0] > -clamp) & (yr[0] < clamp)
        r = _ba_where(keep, r, _z(zero))
    return r


# ---- the case families of test_bias_act_gpu.py (test_bias_act_host.py gives each mutant its teeth on every one)
BA_CASES = {    # name -> (shape, dim, channels_last, bias, view); V = 4 (f32) or 8 (16-bit)
    'lt_v': ((1, 3), 1, False, True, None),                     # numel < V: the tail vector alone
    'tail_nchw': ((1, 5, 3, 1), 1, False, True, None),          # 15: full vectors and a tail of V - 1, C coprime to V
    'tail_w13': ((2, 3, 1, 13), 1, False, True, None),          # 78: a tail of 2 (f32) or 6
    'tail_cl': ((2, 5, 3, 3), 1, True, True, None),             # 90: a tail of 2
    'tail_cl15': ((1, 5, 3, 1), 1, True, True, None),
    'full': ((2, 8, 4, 4), 1, False, True, None),               # no tail
    'full_cl': ((2, 8, 4, 4), 1, True, True, None),
    'dim0': ((3, 5, 2, 7), 0, False, True, None), 'dim0_cl': ((3, 5, 2, 7), 0, True, True, None),
    'dim2': ((3, 5, 2, 7), 2, False, True, None), 'dim2_cl': ((3, 5, 2, 7), 2, True, True, None),
    'dim3': ((3, 5, 2, 7), 3, False, True, None), 'dim3_cl': ((3, 5, 2, 7), 3, True, True, None),
    'nd2': ((3, 5), 1, False, True, None), 'nd3': ((2, 5, 3), 1, False, True, None),
    'nd5': ((2, 3, 2, 2, 3), 1, False, True, None),
    'c1': ((2, 1, 3, 5), 1, False, True, None), 'nc11': ((3, 5, 1, 1), 1, False, True, None),
    'no_bias': ((2, 5, 3, 3), 1, False, False, None),
    'mis_x': ((2, 5, 3, 3), 1, False, True, 'mis_x'), 'mis_dy': ((2, 5, 3, 3), 1, False, True, 'mis_dy'),
    'mis_y': ((2, 5, 3, 3), 1, False, True, 'mis_y'),
    'strided_x': ((2, 5, 3, 3), 1, False, True, 'strided_x'),   # x = base[:, :, ::2]
    'expanded_dy': ((2, 5, 3, 3), 1, False, True, 'expanded_dy'),       # dy = ones(()).expand(shape): stride 0
    'bound': ((3, 5, 3, 7), 1, False, True, None), 'bound_cl': ((3, 5, 3, 7), 1, True, True, None),   # Judge 2's: 315
}
BA_GAINS, BA_CLAMPS = (None, 0.7), (None, 0.9, 256.0)


def ba_sweep_shape(dtype, extra):
    """The 2-D [R, C] of a second-sweep case: numel = BA_SWEEP V + extra when some odd C in 3..63 divides it, else
    the next product above it that keeps a ragged tail."""
    V = BA_V[dtype]
    n = BA_SWEEP * V + extra
    for C in range(3, 65, 2):
        if n % C == 0:
            return n // C, C
    R = cdiv(n, 5)
    while (R * 5) % V == 0:
        R += 1
    return R, 5


def ba_sweep_extras(dtype):
    V = BA_V[dtype]
    return 3 * 256 * V + (V - 1), 1


def ba_flat(t, channels_last):
    """A logical tensor in the order of the kernel's flat index (a copy)."""
    return (t.permute(0, 2, 3, 1) if channels_last else t).reshape(-1).clone()


def ba_unflat(flat, shape, channels_last):
    if channels_last:
        N, C, H, W = shape
        return flat.view(N, H, W, C).permute(0, 3, 1, 2)
    return flat.view(shape)


def ba_step(shape, dim, channels_last):
    """step_b: the dense tensor's stride along `dim`."""
    t = torch.empty(shape)
    return (t.contiguous(memory_format=torch.channels_last) if channels_last else t).stride(dim)


def ba_neighbours(c, dtype):
    """The `dtype` value nearest c and its two neighbours (one ulp below and above), as floats."""
    t = torch.tensor([c], dtype=torch.float32).to(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    return [float((t.view(it) + k).view(dtype)[0]) for k in (-1, 0, 1)]


def ba_plants(act, clamp, dtype):
    """The values planted into a supplied y: 0, -0, and with a clamp NaN and both signs of the `dtype` values at and
    one ulp either side of the clamp (for 256 only where the gradient is piecewise linear in y: exp(256) is no f32)."""
    vals = []
    if clamp is not None:
        if clamp <= 4 or act in ('linear', 'relu', 'lrelu'):
            lo, at, hi = ba_neighbours(clamp, dtype)
            vals += [at, -at, lo, -lo, hi, -hi]
        vals.append(float('nan'))
    return vals + [0.0, -0.0]


def ba_fixture(shape, dim, bias, dtype, act, gain=None, clamp=None, alpha=None, seed=0, exact=False, plant=True):
    """The operands of one case, float64 holding `dtype` values: x, b, dy, v (the gradient of dx), and y = the
    rounded float64 forward with ba_plants written over its first and last elements in index order (so the tail
    vector holds some).  exact: Judge 1's grid -- x and b halves in [-3, 3], dy and v integers in [-8, 8]."""
    if act == 'swish' and clamp is not None and not exact and seed < 64:
        # the strict mask is taken on an f32 RECOMPUTATION of y: the first seed (from the one asked for) at which no
        # element's recomputed |y| is within the forward slack of the clamp, so float64 and f32 mask alike
        op = ba_fixture(shape, dim, bias, dtype, act, gain, clamp, alpha, seed + 64, exact, plant)
        y, s = bias_act_ref(0, act, op['x'], op['b'], **dict(op['kw'], clamp=None))
        if float(((y.abs() - f32(clamp)).abs() - s).min()) > 0:
            return op
        return ba_fixture(shape, dim, bias, dtype, act, gain, clamp, alpha, seed + 1, exact, plant)
    seed %= 64
    g = torch.Generator().manual_seed(seed * 1000003 + sum((i + 2) * s for i, s in enumerate(shape)) * 131 + dim)
    C = shape[dim]
    if exact:
        x = torch.randint(-6, 7, shape, generator=g).double() / 2
        b = torch.randint(-6, 7, (C,), generator=g).double() / 2
        dy, v = (torch.randint(-8, 9, shape, generator=g).double() for _ in range(2))
    else:
        x, dy, v = (rnd(torch.randn(shape, generator=g), dtype) for _ in range(3))
        b = rnd(torch.randn(C, generator=g), dtype)
    op = dict(x=x, b=b if bias else None, dy=dy, v=v, shape=tuple(shape), dim=dim, dtype=dtype, act=act,
              kw=dict(dim=dim, alpha=alpha, gain=gain, clamp=clamp, dtype=dtype))
    y = rnd(bias_act_ref(0, act, x, op['b'], **op['kw'])[0], dtype)
    if plant:
        vals = torch.tensor(ba_plants(act, clamp, dtype), dtype=torch.float64)
        flat = y.reshape(-1).clone()
        n = min(len(vals), flat.numel())
        flat[:n] = vals[:n]
        if flat.numel() >= 2 * len(vals):
            flat[-len(vals):] = vals.flip(0)
        y = flat.view(shape)
    op['y'] = y
    return op


def ba_ref(op, grad, **over):
    """(ref, slack) of a fixture at `grad`, with the operands the drivers of test_bias_act_gpu.py hand the kernel:
    grad 1 of an activation expressed through y (or through nothing) gets y alone -- bias_act_grad(dy, y) -- swish
    gets x and b; grad 2 gets everything.  `over`: operands or options replaced (the host mutants)."""
    o = dict(op, **{k: v for k, v in over.items() if k in ('x', 'b', 'dy', 'v', 'y')})
    kw = dict(op['kw'], **{k: v for k, v in over.items() if k in ('alpha', 'gain', 'clamp')})
    if grad == 0:
        return bias_act_ref(0, op['act'], o['x'], o['b'], **kw)
    if grad == 1:
        if BA_SPEC[op['act']][2] == 'x':
            return bias_act_ref(1, op['act'], o['dy'], o['b'], o['x'], o['y'], None, **kw)
        return bias_act_ref(1, op['act'], o['dy'], None, None, o['y'], None, **kw)
    return bias_act_ref(2, op['act'], o['v'], o['b'], o['x'], o['y'], o['dy'], **kw)


def ba_report(table):
    """{(act, grad, dtype name): worst ratio} as the lines the first GPU run prints."""
    return '\n'.join(f'bias_act worst error / bound: {a:8s} grad {g} {d:4s} {r:.3g}' for (a, g, d), r in sorted(table.items()))


# ---- the autograd-wiring fixtures: sums of one sign and no stored element near a rounding tie
BA_WIRING = (('tanh', None), ('swish', 0.9))     # the second-order cases; relu, lrelu and linear run the exact grid
BA_WIRING_SHAPE = (2, 5, 4, 4)


def ba_near_tie(ref, slack, dtype):
    """Where a value within `slack` of ref may round to `dtype` either way (never for an f32 store)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref, dtype=torch.bool)
    return rnd(ref - slack, dtype) != rnd(ref + slack, dtype)


def ba_wiring_fixture(act, clamp, dtype, dim):
    """x in [0.1, 1.6), b in [0, 0.3), dy and v in [0.5, 1.5): on that range tanh' and swish' are positive and tanh''
    negative, swish'' positive (it changes sign at 2.4), so every term of a bias gradient has one sign; the first
    seed for which no element of the forward, dx or the second-order dx is within its slack of a rounding tie, so the
    device's stored values ARE the rounded reference (test_bias_act_host.py asserts both)."""
    shape = BA_WIRING_SHAPE
    for seed in range(64):
        g = torch.Generator().manual_seed(977 * seed + 31 * dim + len(act))
        x = rnd(0.1 + 1.5 * torch.rand(shape, generator=g), dtype)
        b = rnd(0.3 * torch.rand(shape[dim], generator=g), dtype)
        dy, v = (rnd(0.5 + torch.rand(shape, generator=g), dtype) for _ in range(2))
        kw = dict(dim=dim, alpha=None, gain=None, clamp=clamp, dtype=dtype)
        y, sy = bias_act_ref(0, act, x, b, **kw)
        op = dict(x=x, b=b, dy=dy, v=v, y=rnd(y, dtype), shape=shape, dim=dim, dtype=dtype, act=act, kw=kw, seed=seed)
        if clamp is not None:       # (swish recomputes y for its mask: keep it off the clamp, as ba_fixture does)
            yf, sf = bias_act_ref(0, act, x, b, **dict(kw, clamp=None))
            if float(((yf.abs() - f32(clamp)).abs() - sf).min()) <= 0:
                continue
        if not any(bool(ba_near_tie(r, s, dtype).any()) for r, s in ((y, sy), ba_ref(op, 1), ba_ref(op, 2))):
            return op
    raise AssertionError('no seed below 64 keeps every element off a rounding tie')


def ba_sum_bound(ref_terms, slack_terms, dims, dtype):
    """(ref, bound) of a bias gradient: the float64 sum over `dims` of the reference terms as the kernel STORES them
    (rounded to `dtype`), within u |ref| (the sum's own rounding to `dtype`) + gamma(K) A, K the number of values per
    output (each f32 addition rounds a partial sum that A bounds), A the sum of |terms| plus their slack."""
    t = rnd(ref_terms, dtype) if dtype != torch.float32 else ref_terms
    ref = t.sum(dims)
    K = ref_terms.numel() // ref.numel()
    A = (t.abs() + slack_terms).sum(dims)
    return ref, U[dtype] * ref.abs() + gamma(K) * A + TINY[dtype]


# ---- the contract, written out literally: test_bias_act_host.py holds the reference to it, test_bias_act_gpu.py the
# device
NAN, INF = float('nan'), float('inf')
# lrelu, alpha 0.25, gain 2, clamp 2.5, dy = 1.  y: 0, -0, +clamp, -clamp, one ulp inside (+, -), one ulp outside
# (+, -), NaN -> alpha branch, alpha branch, 0, 0, passed (gain), passed (alpha gain), 0, 0, 0
BA_EDGE_Y = {
    torch.float16: [0.0, -0.0, 2.5, -2.5, 2.498046875, -2.498046875, 2.501953125, -2.501953125, NAN],
    torch.bfloat16: [0.0, -0.0, 2.5, -2.5, 2.484375, -2.484375, 2.515625, -2.515625, NAN],
    torch.float32: [0.0, -0.0, 2.5, -2.5, 2.499999761581421, -2.499999761581421, 2.500000238418579,
                    -2.500000238418579, NAN],
}
BA_EDGE_DX = [0.5, 0.5, 0.0, 0.0, 2.0, 0.5, 0.0, 0.0, 0.0]
BA_EDGE_DX_FREE = [0.5, 0.5, 2.0, 0.5, 2.0, 0.5, 2.0, 0.5, 0.5]       # no clamp: nothing masked, a NaN y takes alpha
BA_EDGE_KW = dict(alpha=0.25, gain=2.0)
# forward of x = NaN, +Inf, -Inf at gain 2: with clamp 2.5, and without (-2 BA_SELU_SA = -3.5161986351013184)
BA_FWD_NONFINITE = {
    'linear': ([-2.5, 2.5, -2.5], [NAN, INF, -INF]),
    'relu': ([0.0, 2.5, 0.0], [0.0, INF, 0.0]),          # relu(NaN): `v > 0 ? v : 0` is 0, clamp or not
    'lrelu': ([-2.5, 2.5, -2.5], [NAN, INF, -INF]),
    'tanh': ([-2.5, 2.0, -2.0], [NAN, 2.0, -2.0]),
    'sigmoid': ([-2.5, 2.0, 0.0], [NAN, 2.0, 0.0]),
    'elu': ([-2.5, 2.5, -2.0], [NAN, INF, -2.0]),
    'selu': ([-2.5, 2.5, -2.5], [NAN, INF, -3.5161986351013184]),
    'softplus': ([-2.5, 2.5, 0.0], [NAN, INF, 0.0]),
    'swish': ([-2.5, 2.5, -2.5], [NAN, INF, NAN]),       # -Inf / (1 + Inf) is NaN, in the reference plugin too
}
