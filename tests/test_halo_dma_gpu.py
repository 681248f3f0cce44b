"""The LDS-DMA form of the stride-1 halo 3x3 convolution (conv3x3.hip conv3x3_halo_dma_kernel, SG2_HALO_DMA) against
the register-staged halo kernel it stands in for (SG2_HALO_DMA=0) and against float64.

The two routes run the same MFMAs in the same order on the same operands, so y, y_raw and the deterministic dot
must be bitwise equal; the new route must also match float64 at test_conv3x3_halo_direct's tolerances.

(sg2_conv3x3, the stride-1 entry point, has no residual / raw_act argument -- conv3x3_fused asserts residual is None
at stride 1 -- so the D block's form runs as its stride-1 conv does in the network: bias + lrelu + gain + clamp with
the raw output.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise as EW
import poison
from golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@pytest.fixture(autouse=True)
def _poisoned_empties(request, monkeypatch):
    """Every torch.empty / empty_like of the op wrappers comes back NaN-filled (tests/poison.py)."""
    poison.poisoned_empties(monkeypatch, poison.op_modules(request.node.originalname))

# (N, Cin, H, W, Cout): the smallest shapes at which each part of the staging can go wrong
SHAPES = [
    (2, 64, 32, 32, 64),      # two chunks, whole tiles, one channel tile
    (2, 64, 32, 32, 128),     # ... two channel tiles
    (2, 32, 16, 32, 64),      # a single chunk: the prologue is longer than the loop
    (2, 96, 20, 37, 128),     # three chunks (odd slot parity), ragged right / bottom tiles, an image edge inside a DMA
    (1, 256, 33, 40, 192),    # eight chunks, a one-pixel row overhang, Cout % 128 != 0
    (3, 128, 8, 64, 128),     # an image no taller than a tile, several samples: no halo row crosses a sample
    (2, 512, 32, 32, 512),    # the deepest K of the bench
    (2, 40, 16, 24, 64),      # the gate refuses: Cin % 32 != 0, W < 32
    (3, 128, 16, 16, 64),     # the gate refuses: W < 32
]


def _run_forms(cg, sg2hip, t):
    """The four forms on the route the environment selects -> dict of outputs."""
    out = {}
    out['plain'] = cg.conv3x3_fused(t['x'], t['wp'], t['cout'])[0]
    out['dblock'] = cg.conv3x3_fused(t['x'], t['wp'], t['cout'], bias=t['b'], act=1, alpha=0.2, gain=np.sqrt(2), clamp=1.5,
                                     want_raw=True)
    out['glayer'] = cg.conv3x3_fused(t['x'], t['wp'], t['cout'], in_scale=t['s'], out_scale=t['d'], noise=t['noise'],
                                     noise_gain=0.3, bias=t['b'], act=1, alpha=0.2, gain=np.sqrt(2), clamp=1.5,
                                     want_raw=True)
    with sg2hip.deterministic(False, device=DEV):
        out['dgrad_atomic'] = cg.conv3x3_fused(t['x'], t['wp'], t['cout'], out_scale=t['d'], dot_src=t['src'])
    with sg2hip.deterministic(True, device=DEV):
        out['dgrad_det'] = cg.conv3x3_fused(t['x'], t['wp'], t['cout'], out_scale=t['d'], dot_src=t['src'])
        out['dgrad_det2'] = cg.conv3x3_fused(t['x'], t['wp'], t['cout'], out_scale=t['d'], dot_src=t['src'])
    return out


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', SHAPES)
def test_halo_dma_matches_register_route_and_float64(shape, dtype, monkeypatch):
    import sg2hip
    from torch_utils.ops import conv2d_gradfix as cg
    monkeypatch.setenv('SG2_C64_RING', '0')
    monkeypatch.setenv('SG2_HALO_PERSIST', '0')
    N, Cin, H, W, Cout = shape
    torch.manual_seed(17)
    x = torch.randn(N, Cin, H, W)
    w = torch.randn(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)
    s = torch.rand(N, Cin) + 0.5
    d = torch.rand(N, Cout) + 0.5
    noise = torch.randn(N, 1, H, W)
    b = torch.randn(Cout) * 0.1
    src = torch.randn(N, Cout, H, W).to(dtype)
    t = dict(cout=Cout, x=x.to(DEV, dtype).contiguous(memory_format=torch.channels_last),
             wp=cg._pack_conv(w.to(DEV, dtype)), s=s.to(DEV), d=d.to(DEV), b=b.to(DEV),
             noise=noise.to(DEV, dtype).reshape(N, H, W).contiguous(),
             src=src.to(DEV).contiguous(memory_format=torch.channels_last))

    monkeypatch.setenv('SG2_HALO_DMA', '0')
    old = _run_forms(cg, sg2hip, t)
    monkeypatch.setenv('SG2_HALO_DMA', '1')
    new = _run_forms(cg, sg2hip, t)

    # 1. y and y_raw bitwise equal between the routes; 2. the deterministic dot bitwise equal, and run to run
    assert torch.equal(new['plain'], old['plain'])
    for form in ('dblock', 'glayer'):
        assert torch.equal(new[form][0], old[form][0]), form
        assert torch.equal(new[form][1], old[form][1]), form
    for form in ('dgrad_atomic', 'dgrad_det'):
        assert torch.equal(new[form][0], old[form][0]), form
    assert torch.equal(new['dgrad_det'][2], old['dgrad_det'][2])
    assert torch.equal(new['dgrad_det'][2], new['dgrad_det2'][2])
    assert torch.equal(new['dgrad_det'][0], new['dgrad_det2'][0])

    # 3. the new route against float64
    tol = 5e-3 if dtype == torch.float16 else 2e-2
    wd = w.to(dtype).double()
    c0 = F.conv2d(x.to(dtype).double(), wd, padding=1)
    xs = (x.to(dtype).float() * s[:, :, None, None]).to(dtype).double()
    cm = F.conv2d(xs, wd, padding=1)
    bd = b.to(dtype).double()[None, :, None, None]

    def epi(z):
        return (F.leaky_relu(z, 0.2) * np.sqrt(2)).clamp(-1.5, 1.5)

    def check(got, ref, what):
        assert rel_err(got.float(), ref) < tol, what
        for n in range(N):
            assert rel_err(got[n].float(), ref[n]) < 2 * tol, (what, n)

    check(new['plain'], c0, 'plain')
    check(new['dblock'][0], epi(c0 + bd), 'dblock y')
    check(new['dblock'][1], c0, 'dblock raw')
    check(new['glayer'][0], epi(cm * d[:, :, None, None] + noise.to(dtype).double() * 0.3 + bd), 'glayer y')
    check(new['glayer'][1], cm, 'glayer raw')
    dot_ref = (c0.to(dtype).double() * src.double()).sum([2, 3])
    for form in ('dgrad_atomic', 'dgrad_det'):
        check(new[form][0], c0 * d[:, :, None, None], form)
        assert rel_err(new[form][2], dot_ref) < tol, form

    # 4. every element of the new route's outputs (tests/elementwise.py).  Rounding model: round(x round(s)) -- the
    # LDS-DMA form scales the staged halo in place by the style rounded to the activation type, and so does the
    # register-staged kernel that keeps the two shapes the gate refuses; bias rounded to the activation type; y_raw
    # the accumulator rounded once.  (The old route's outputs are bitwise equal to these, by 1.)
    f32 = lambda v: float(np.float32(v))
    K = 9 * Cin
    sl0 = EW.accumulation_slack(K, F.conv2d(x.to(dtype).double().abs(), wd.abs(), padding=1))
    xm = EW.mod_x(x, s, dtype)
    cx = F.conv2d(xm, wd, padding=1)
    slx = EW.accumulation_slack(K, F.conv2d(xm.abs(), wd.abs(), padding=1))
    dd = d[:, :, None, None].double()
    ng = noise.to(dtype).double() * f32(0.3)

    def epi32(z):    # the scalar arguments at the f32 values the kernel receives
        return (F.leaky_relu(z, f32(0.2)) * f32(np.sqrt(2))).clamp(-1.5, 1.5)

    def ew(got, ref, slack, what):
        print(f'elementwise halo_dma {what} {str(dtype)[6:]}: worst error / bound '
              f'{EW.assert_elementwise(got, ref, slack, dtype, what):.3f}')

    ew(new['plain'], c0, sl0, 'plain')
    ew(new['dblock'][0], epi32(c0 + bd), EW.epilogue_slack(sl0, c0, b=bd, gain=f32(np.sqrt(2)), alpha=f32(0.2)), 'dblock y')
    ew(new['dblock'][1], c0, sl0, 'dblock raw')
    ew(new['glayer'][0], epi32(cx * dd + ng + bd),
       EW.epilogue_slack(slx, cx, dd, ng, bd, gain=f32(np.sqrt(2)), alpha=f32(0.2)), 'glayer y')
    ew(new['glayer'][1], cx, slx, 'glayer raw')
    for form in ('dgrad_atomic', 'dgrad_det'):
        ew(new[form][0], c0 * dd, EW.epilogue_slack(sl0, c0, dd), form + ' out_scale')
