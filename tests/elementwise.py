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


def _upfirdn(x, f, up, down, padding, flip_filter):
    N, C, H, W = x.shape
    px0, px1, py0, py1 = [padding] * 4 if isinstance(padding, int) else padding
    x = F.pad(x.reshape(N, C, H, 1, W, 1), [0, up - 1, 0, 0, 0, up - 1]).reshape(N, C, H * up, W * up)
    x = F.pad(x, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    x = x[:, :, max(-py0, 0):x.shape[2] - max(-py1, 0), max(-px0, 0):x.shape[3] - max(-px1, 0)]
    f = f if flip_filter else f.flip([0, 1])
    return F.conv2d(x, f[None, None].repeat(C, 1, 1, 1), groups=C)[:, :, ::down, ::down]


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
