"""Deterministic mode (sg2hip.deterministic / sg2_set_deterministic): every kernel that reduces with float atomics
on the fast path -- split-K partial sums, weight-gradient pixel splits, per-(n, c) dot / bias / demodulation
reductions, the grid-sample input-gradient scatter -- is run twice in deterministic mode and must give bitwise
equal results, and must agree with the fast (atomic) path to the rounding of a different summation order.
Then one whole phase-isolated iteration at configuration width (C2) in f32 and fp16: every gradient summary and
statistic bitwise equal between two runs.

Every deterministic run here starts from a NaN-filled scratch and writes into NaN-filled outputs (tests/poison.py):
running twice in one scratch cannot see an element that is never written (the same stale value both times), and a
fresh process' scratch is zero pages, so without the poison what such an element holds depends on test order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise as EW
import poison
import sg2hip
from golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CL = torch.channels_last


@pytest.fixture(autouse=True)
def _poisoned(request, monkeypatch):
    """Every torch.empty / empty_like of the op wrappers comes back NaN-filled, and each deterministic run below
    starts from a NaN-filled scratch (tests/poison.py): an output element that is not assigned, or a slot element that
    is summed without having been written by the same call, fails the comparison.  The scratch is left zeroed, as a
    fresh process sees it."""
    poison.poisoned_empties(monkeypatch, poison.op_modules(request.node.originalname))
    yield
    poison.zero_det_scratch(DEV)


def _nhwc(t, dtype):
    return t.to(DEV).to(dtype).contiguous(memory_format=CL)


def _check(fn, tol):
    """fn() -> list of tensors.  Deterministic twice: bitwise equal; vs the atomic path: within tol (f32
    outputs), or within 1e-3 for 16-bit outputs: a sum that lands next to a rounding boundary of the 16-bit
    result rounds to the neighbouring value (one ulp, 2^-11 / 2^-8 relative) when its order changes."""
    with sg2hip.deterministic():
        poison.poison_det_scratch(DEV)
        a = [t.detach().clone() for t in fn()]
        poison.poison_det_scratch(DEV)
        b = [t.detach().clone() for t in fn()]
    ref = [t.detach().clone() for t in fn()]
    torch.cuda.synchronize()
    for i, (x, y, r) in enumerate(zip(a, b, ref)):
        assert torch.equal(x, y), f'output {i}: deterministic runs differ (max {float((x.float() - y.float()).abs().max()):.3g})'
        t = tol if x.dtype == torch.float32 else max(tol, 1e-3)
        e = rel_err(x.float(), r.double().cpu())
        assert e < t, f'output {i}: deterministic vs atomic path {e:.3g} (tol {t:g})'


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('shape', [(2, 16, 24, 8), (3, 64, 7, 512), (4, 64, 64, 64)])
def test_det_layer_bwd(dtype, shape):
    from torch_utils.ops import conv2d_gradfix as cg
    N, H, W, C = shape
    g = torch.Generator().manual_seed(3)
    y, c, dy = (_nhwc(torch.randn(N, C, H, W, generator=g) * 2, dtype) for _ in range(3))
    d = (torch.rand(N, C, generator=g) + 0.5).to(DEV)
    _check(lambda: cg.layer_bwd(dy, y, c, d, act=1, alpha=0.2, gain=1.5, clamp=2.5), 1e-5)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', [(2, 64, 20, 33, 96), (9, 64, 128, 256, 64), (2, 512, 16, 16, 512)])
def test_det_conv3x3_dot_and_wgrad(dtype, shape):
    """16-bit 3x3: the dot epilogue (generic halo kernel: per-tile slots; the persistent C = 64 shape, 9 samples
    over 256 workgroups so runs cross samples: per-(sample, workgroup, wave) slots) and the LDS-DMA weight
    gradient, plain and scaled."""
    from torch_utils.ops import conv2d_gradfix as cg
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(4)
    x = _nhwc(torch.randn(N, Cin, H, W, generator=g), dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)).to(DEV).to(dtype)
    src = _nhwc(torch.randn(N, Cout, H, W, generator=g), dtype)
    s = (torch.rand(N, Cout, generator=g) + 0.5).to(DEV)
    gr = _nhwc(torch.randn(N, Cout, H, W, generator=g), dtype)
    xs = (torch.rand(N, Cin, generator=g) + 0.5).to(DEV)

    def fn():
        y, raw, dot = cg.conv3x3_fused(x, cg._pack_conv(w), Cout, out_scale=s, dot_src=src)
        return [y, dot, cg._wgrad_raw(gr, x, 3, 3, 1, (1, 1)), cg._wgrad_raw(gr, x, 3, 3, 1, (1, 1), x_scale=xs)]
    _check(fn, 1e-5)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('geom', [(3, 1, 1, False, 2, 512, 8, 8, 512), (3, 1, 1, False, 2, 512, 4, 4, 512),
                                  (3, 2, 0, True, 2, 128, 9, 9, 64), (3, 2, 0, False, 3, 32, 12, 10, 48),
                                  (1, 1, 0, True, 3, 128, 9, 7, 3)])
def test_det_conv_fused_split_k_and_dot(dtype, geom):
    """Implicit-GEMM conv: split-K (the f32 low-resolution 512-channel layers), strided / transposed phases,
    the per-element dot epilogue, the 1x1 small-depth dot kernel; and the generic weight gradient (f32 split
    form, pixel-split slots)."""
    from torch_utils.ops import conv2d_gradfix as cg
    k, stride, pad, transpose, N, Cin, H, W, Cout = geom
    g = torch.Generator().manual_seed(29)
    x = _nhwc(torch.randn(N, Cin, H, W, generator=g), dtype)
    if transpose:
        w = (torch.randn(Cin, Cout, k, k, generator=g) / (Cin * k * k) ** 0.5).to(DEV).to(dtype)
        oh, ow = (H - 1) * stride - 2 * pad + k, (W - 1) * stride - 2 * pad + k
        wp = cg._pack_convT(w)
    else:
        w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).to(DEV).to(dtype)
        oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        wp = cg._pack_conv(w)
    s = (torch.rand(N, Cout, generator=g) + 0.5).to(DEV)
    src = _nhwc(torch.randn(N, Cout, oh, ow, generator=g), dtype)
    gr = _nhwc(torch.randn(N, Cout, oh, ow, generator=g), dtype)

    def fn():
        y, _, dot = cg.conv_fused(x, wp, Cout, oh, ow, k, k, stride, (pad, pad), transpose=transpose, out_scale=s,
                                  dot_src=src)
        out = [y, dot]
        if not transpose:
            out.append(cg._wgrad_raw(gr, x, k, k, stride, (pad, pad)))
        return out
    _check(fn, 1e-5)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('cin,cout', [(1, 64), (3, 16), (64, 1), (128, 3)])
def test_det_wgrad_1x1_small_depth(dtype, cin, cout):
    from torch_utils.ops import conv2d_gradfix as cg
    g = torch.Generator().manual_seed(11)
    n, h, w = 2, 33, 47
    x = _nhwc(torch.randn(n, cin, h, w, generator=g), dtype)
    gr = _nhwc(torch.randn(n, cout, h, w, generator=g), dtype)
    gs, xs = (torch.rand(n, cout, generator=g) + 0.5).to(DEV), (torch.rand(n, cin, generator=g) + 0.5).to(DEV)
    _check(lambda: [cg._wgrad_raw(gr, x, 1, 1, 1, (0, 0), x_scale=xs, g_scale=gs)], 1e-5)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('case', ['s2', 's2_scaled', 'reg16_scaled'])
def test_det_wgrad_halo_phases(dtype, case):
    """Halo weight gradients: the stride-2 one-launch kernel, and the register-staged per-phase kernel (a scaled
    16^2 layer whose workgroups span several samples): slots summed in order."""
    from torch_utils.ops import conv2d_gradfix as cg
    g = torch.Generator().manual_seed(31)
    if case.startswith('s2'):
        N, Ci, Co = 3, 64, 72
        x = _nhwc(torch.randn(N, Ci, 67, 65, generator=g), dtype)
        gr = _nhwc(torch.randn(N, Co, 33, 32, generator=g), dtype)
        xs = (torch.rand(N, Ci, generator=g) + 0.5).to(DEV) if case == 's2_scaled' else None
        _check(lambda: [cg._wgrad_raw(gr, x, 3, 3, 2, (0, 0), x_scale=xs)], 1e-5)
    else:
        N, Ci, Co = 8, 128, 128
        x = _nhwc(torch.randn(N, Ci, 16, 16, generator=g), dtype)
        gr = _nhwc(torch.randn(N, Co, 16, 16, generator=g), dtype)
        xs = (torch.rand(N, Ci, generator=g) + 0.5).to(DEV)
        gs = (torch.rand(N, Co, generator=g) + 0.5).to(DEV)
        _check(lambda: [cg._wgrad_raw(gr, x, 3, 3, 1, (1, 1), x_scale=xs, g_scale=gs)], 1e-5)


def test_det_affine_grid_sample_bwd():
    """The ADA warp's input gradient: a fixed-order gather per input pixel in deterministic mode (bitwise equal
    twice), against affine_grid + grid_sample's input gradient in float64 as the atomic scatter is held
    (test_ops_gpu.py::test_affine_grid_sample), with a static buffer and a dynamic logical extent as the augment
    pipe uses it."""
    from torch_utils.ops import grid_sample_gradfix as gs
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 3, 140, 136, generator=g)
    theta = torch.tensor([[[1.05, 0.1, 0.03], [-0.08, 0.95, -0.02]], [[0.9, -0.2, 0.1], [0.15, 1.1, 0.05]],
                          [[0.7, 0.0, -0.2], [0.0, 1.3, 0.1]]])
    size = [3, 3, 150, 146]
    dy = torch.randn(size, generator=g)
    grid = F.affine_grid(theta.double(), size, align_corners=False)
    xd = x.to(DEV).requires_grad_(True)
    refs = []
    for hw in (None, (130, 128)):
        xr = (x if hw is None else x[:, :, :hw[0], :hw[1]]).double().requires_grad_(True)
        gr, = torch.autograd.grad(F.grid_sample(xr, grid, align_corners=False), [xr], dy.double())
        refs.append(gr if hw is None else F.pad(gr, [0, 136 - hw[1], 0, 140 - hw[0]]))

    def fn():
        out = []
        for hw in (None, (130, 128)):
            dyn = None if hw is None else torch.tensor(hw, dtype=torch.int32, device=DEV)
            y = gs.affine_grid_sample(xd, theta.to(DEV), size, dyn_hw=dyn)
            gx, = torch.autograd.grad(y, [xd], dy.to(DEV))
            out.append(gx if hw is None else gx[:, :, :hw[0], :hw[1]])
        return out
    with sg2hip.deterministic():
        poison.poison_det_scratch(DEV)
        a = [t.clone() for t in fn()]
        poison.poison_det_scratch(DEV)
        b = [t.clone() for t in fn()]
    fast = fn()
    for i, (u, v, w, r) in enumerate(zip(a, b, fast, refs)):
        r = r if i == 0 else r[:, :, :130, :128]
        assert torch.equal(u, v), f'extent {i}: deterministic runs differ'
        assert rel_err(u, r) < 1e-5 and rel_err(w, r) < 1e-5, (rel_err(u, r), rel_err(w, r))


@pytest.mark.parametrize('seed', [0, 1])
def test_det_gather_matches_scatter_ada_maps(seed, monkeypatch):
    """The gather's scan box (the exact preimage widened by 1/64 output pixel) misses no contribution: bitwise equal
    to the gather scanning one pixel beyond the rounded-out box (SG2_GATHER_WIDE=1: the same candidates in the same
    order plus ones that contribute nothing), and, like the atomic scatter, equal to grid_sample's float64 gradient to the rounding of the float sampling coordinates
(2^-11 of the sum of the terms' magnitudes plus the largest |dy|), over maps drawn as the ADA pipe draws them
    (scale 2^(0.2 N(0,1)), anisotropy, rotation, translation) plus a zoom-in to a quarter and a zoom-out by 3, at
    the pipe's 2x-upsampled sizes in a static buffer with a dynamic extent."""
    from torch_utils.ops import grid_sample_gradfix as gs
    g = torch.Generator().manual_seed(100 + seed)
    n = 12
    s = torch.exp2(0.2 * torch.randn(n, generator=g))
    s[:3] = torch.tensor([0.25, 0.4, 3.0])
    a = torch.exp2(0.2 * torch.randn(n, generator=g))
    r = (torch.rand(n, generator=g) - 0.5) * 0.6
    tx, ty = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.1
    c, si = torch.cos(r), torch.sin(r)
    theta = torch.stack([torch.stack([s * a * c, -s * si, tx], 1), torch.stack([s * si, s / a * c, ty], 1)], 1)
    x = torch.randn(n, 1, 524, 530, generator=g)
    size = [n, 1, 512, 520]
    dy = torch.randn(size, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    dyn = torch.tensor([500, 516], dtype=torch.int32, device=DEV)

    def fn():
        y = gs.affine_grid_sample(xd, theta.float().to(DEV), size, dyn_hw=dyn)
        return torch.autograd.grad(y, [xd], dy.to(DEV))[0][:, :, :500, :516]
    with sg2hip.deterministic():
        poison.poison_det_scratch(DEV)
        u = fn().clone()
        monkeypatch.setenv('SG2_GATHER_WIDE', '1')
        poison.poison_det_scratch(DEV)
        wide = fn().clone()
        monkeypatch.delenv('SG2_GATHER_WIDE')
    assert torch.equal(u, wide), f'{int((u != wide).sum())} pixels differ from the wide scan'
    w = fn()
    xr = x[:, :, :500, :516].double().requires_grad_(True)
    grid = F.affine_grid(theta.double(), size, align_corners=False)
    ref, = torch.autograd.grad(F.grid_sample(xr, grid, align_corners=False), [xr], dy.double())
    mag, = torch.autograd.grad(F.grid_sample(xr, grid, align_corners=False), [xr], dy.double().abs())
    # the float sampling coordinates (|ix| up to ~10^3, a few roundings of 2^-24) move each bilinear weight by up to
    # ~2^-12 (and, at a pixel boundary, a weight that small to the neighbouring pixel): a missed contribution of
    # weight >= 2^-9 is caught
    tol = 2.0 ** -11 * (mag + float(dy.abs().max()))
    for name, got in (('gather', u), ('scatter', w)):
        err = (got.double().cpu() - ref).abs()
        bad = err > tol
        assert not bool(bad.any()), (f'{name}: {int(bad.sum())} pixels off the float64 gradient, max '
                                     f'{float(err.max()):.3g}, in samples {sorted(set(bad.nonzero()[:, 0].tolist()))}')


def test_det_dot_hw_and_vjp_axpy():
    from torch_utils.ops import conv2d_gradfix as cg
    g = torch.Generator().manual_seed(5)
    a = _nhwc(torch.randn(3, 64, 37, 41, generator=g), torch.float16)
    b = _nhwc(torch.randn(3, 64, 37, 41, generator=g), torch.float16)
    _check(lambda: [cg.dot_hw(a, b)], 1e-5)
    # vjp_axpy's dot goes through per-workgroup slots too (the form of modconv._LayerVJP: G and sum_p g_dx * dxs)
    sa, sb = (torch.rand(3, 64, generator=g) + 0.5).to(DEV), torch.randn(3, 64, generator=g).to(DEV)
    _check(lambda: list(cg.vjp_axpy(a, sa, b, sb, e=b)), 1e-5)


@pytest.mark.timeout(300)
@pytest.mark.parametrize('dt', [None, 'fp16'])
def test_det_isolated_iteration_c2(dt):
    """A whole phase-isolated iteration at the C2 configuration's width (256^2, cbase 16384, batch 4), twice in
    deterministic mode: every gradient summary (norm and sampled entries), pl_mean and every reported statistic
    bitwise equal."""
    import config_parity as cp
    from golden_util import load
    fdt = None if dt is None else torch.float16
    runs = []
    for _ in range(2):
        cfg, inp, tape, fix = cp.load_fixture(load('train_c2_iso.npz'))
        poison.poison_det_scratch(DEV)      # the trainer's deterministic scope registers this same scratch
        runs.append(cp.run_product(cfg, inp, tape, DEV, fp16_dtype=fdt, isolated=True, deterministic=True))
    (g1, s1), (g2, s2) = runs
    assert sorted(g1) == sorted(g2)
    diff = [k for k in g1 if not np.array_equal(np.asarray(g1[k]), np.asarray(g2[k]))]
    assert not diff, f'{len(diff)} summaries differ between deterministic runs, e.g. {diff[:3]}'
    for (n1, v1), (n2, v2) in zip(s1, s2):
        assert n1 == n2 and np.array_equal(v1, v2), n1


def test_det_affine_grid_sample_bwd_singular():
    """A singular affine map (det 0: both output axes sample along one input line): the deterministic gather has
    no finite inverse to bound its scan, so it scans the whole output; its input gradient must still equal
    grid_sample's in float64, as the atomic scatter's does."""
    from torch_utils.ops import grid_sample_gradfix as gs
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 40, 36, generator=g)
    theta = torch.tensor([[[0.5, 0.5, 0.1], [0.5, 0.5, -0.1]], [[0.0, 0.0, 0.2], [0.0, 0.0, 0.3]]])
    size = [2, 3, 44, 40]
    dy = torch.randn(size, generator=g)
    grid = F.affine_grid(theta.double(), size, align_corners=False)
    xr = x.double().requires_grad_(True)
    ref, = torch.autograd.grad(F.grid_sample(xr, grid, align_corners=False), [xr], dy.double())
    xd = x.to(DEV).requires_grad_(True)

    def fn():
        y = gs.affine_grid_sample(xd, theta.to(DEV), size)
        return torch.autograd.grad(y, [xd], dy.to(DEV))[0]
    with sg2hip.deterministic():
        poison.poison_det_scratch(DEV)
        u = fn().clone()
    w = fn()
    assert rel_err(u, ref) < 1e-5 and rel_err(w, ref) < 1e-5, (rel_err(u, ref), rel_err(w, ref))


@pytest.mark.parametrize('geom', [(512, 512, 3, 1, 1, 2, 8, 8), (64, 40, 3, 1, 1, 3, 10, 9), (40, 104, 3, 2, 0, 2, 17, 17),
                                  (48, 136, 1, 1, 0, 2, 12, 12), (8, 520, 3, 1, 1, 1, 4, 4)])
@pytest.mark.parametrize('layout', [True, 'swap'])
def test_det_wgrad_param_layout(geom, layout):
    """The f32 weight gradient's fixed-order slot sum written straight into the parameter layout
    (sg2_conv2d_wgrad_oikk: [A, B, kh, kw], or [B, A, kh, kw] for 'swap'; an LDS-transposed tile of one a x 64 b per
    workgroup): contiguous in that layout, deterministic, equal to the K-major slot sum's permuted view to the
    rounding of its summation order, and to a float64
    weight gradient; B not a multiple of 64, 1x1 and stride-2 forms included."""
    from torch_utils.ops import conv2d_gradfix as cg
    A, B, k, stride, pad, N, H, W = geom
    g = torch.Generator().manual_seed(41)
    x = _nhwc(torch.randn(N, B, H, W, generator=g), torch.float32)
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gr = _nhwc(torch.randn(N, A, oh, ow, generator=g), torch.float32)
    with sg2hip.deterministic():
        poison.poison_det_scratch(DEV)
        p1 = cg._wgrad_raw(gr, x, k, k, stride, (pad, pad), alpha=0.5, param_layout=layout).clone()
        poison.poison_det_scratch(DEV)
        p2 = cg._wgrad_raw(gr, x, k, k, stride, (pad, pad), alpha=0.5, param_layout=layout)
        poison.poison_det_scratch(DEV)
        plain = cg._wgrad_raw(gr, x, k, k, stride, (pad, pad), alpha=0.5)
        torch.cuda.synchronize()
    assert p2.shape == (A, B, k, k)
    assert (p2.transpose(0, 1) if layout == 'swap' else p2).is_contiguous()
    assert torch.equal(p1, p2), 'parameter-layout weight gradient not deterministic'
    ref = 0.5 * torch.nn.grad.conv2d_weight(x.double().cpu(), (A, B, k, k), gr.double().cpu(), stride=stride,
                                            padding=pad)
    e_plain = rel_err(p2, plain.double().cpu())
    assert e_plain < 1e-6, f'parameter layout vs K-major slot sum {e_plain:.3g}'
    e_ref = rel_err(p2, ref)
    assert e_ref < 1e-5, f'parameter layout vs float64 {e_ref:.3g}'


# ------------------------------------------------------------------ ragged shapes from a NaN-filled scratch
# The cases above are mostly whole tiles.  Below, the ragged shapes of the float-atomic tests (test_ops_gpu.py) at
# their smallest, in deterministic mode from a poisoned scratch into poisoned outputs, held to the float64 references
# and tolerances of those atomic-mode twins.
def _det_poisoned(fn):
    """fn() -> list of tensors.  Twice in deterministic mode, each run from a NaN-filled scratch: no NaN, bitwise
    equal -> the first run's outputs."""
    with sg2hip.deterministic():
        poison.poison_det_scratch(DEV)
        a = [t.detach().clone() for t in fn()]
        poison.poison_det_scratch(DEV)
        b = [t.detach().clone() for t in fn()]
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        nan = torch.isnan(x)
        assert not bool(nan.any()), (f'output {i}: {int(nan.sum())} of {x.numel()} elements NaN (unwritten output or '
                                     f'slot), first at {tuple(nan.nonzero()[0].tolist())} of {tuple(x.shape)}')
        assert torch.equal(x, y), f'output {i}: deterministic runs differ'
    return a


def _ew(got, ref, slack, dtype, what):
    print(f'elementwise det {what}: worst error / bound {EW.assert_elementwise(got, ref, slack, dtype, what):.3g}')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape,scaled,kernel', [((3, 128, 96, 20, 37), False, 'dma'), ((3, 128, 96, 20, 37), True, 'reg'),
                                                 ((2, 8, 40, 16, 16), False, 'dma'), ((2, 8, 40, 16, 16), True, 'reg'),
                                                 ((3, 128, 96, 20, 27), True, 'dma')])
def test_det_poisoned_wgrad3x3_halo(dtype, shape, scaled, kernel):
    """The stride-1 halo weight gradient's slots (w3_det_slots, not zeroed) at test_wgrad3x3_halo's ragged shapes
    (N, A, B, H, W): A and B no multiples of the 64-channel block.  wgrad3x3_run's arithmetic, 256 target workgroups:
      (3, 128, 96, 20, 37): 32 x 8 tiles, 2 x 3 = 6 a sample, 18 in all; 2 x 2 channel blocks; splits = min(256 / 4,
        18 / 4) = 4, tiles_per_block = ceil(18 / 4) = 5, splits = ceil(18 / 5) = 4: the last split holds 3 tiles.
        Plain: the LDS-DMA kernel.  Scaled: the largest divisor of 6 that is <= 5 is 3 < 4: register-staged kernel.
      (2, 8, 40, 16, 16): 16 x 16 tiles, 1 a sample, 2 in all; splits = max(1, 2 / 4) = 1, tiles_per_block 2.  Plain:
        LDS-DMA; scaled: divisor 1 < 4: register-staged, its one workgroup spanning both samples.
      (3, 128, 96, 20, 27): 16 x 16 tiles, 2 x 2 = 4 a sample, 12 in all; splits = min(64, 12 / 4) = 3,
        tiles_per_block 4 = a divisor of 4, >= 4: scaled, the LDS-DMA kernel takes it (ragged right / bottom tiles).
    Reference, tolerance and elementwise rounding model per kernel as in test_wgrad3x3_halo ('f32': x s kept in f32 by
    the LDS-DMA kernel; 'x_f32s': round(x s) by the register-staged one); N H W <= 2220 at every shape."""
    from torch_utils.ops import conv2d_gradfix as cg
    N, A, B, H, W = shape
    g0 = torch.Generator().manual_seed(21)
    g = _nhwc(torch.randn(N, A, H, W, generator=g0), dtype)
    x = _nhwc(torch.randn(N, B, H, W, generator=g0), dtype)
    s = (torch.rand(N, B, generator=g0) + 0.5).to(DEV) if scaled else None
    dw, = _det_poisoned(lambda: [cg._wgrad_raw(g, x, 3, 3, 1, (1, 1), x_scale=s)])
    xs = (x.float() * s[:, :, None, None]).to(dtype) if scaled else x
    ref = torch.nn.grad.conv2d_weight(xs.double().cpu(), [A, B, 3, 3], g.double().cpu(), padding=1)
    assert rel_err(dw, ref) < (2e-3 if dtype == torch.float16 else 1e-2)
    gd = g.double().cpu()
    if scaled and kernel == 'dma':
        rm, sl = EW.wgrad_ref(gd, EW.mod_x_f32(x.cpu(), s.cpu(), dtype), [A, B, 3, 3], f32_ops=3, padding=1)
    else:
        xm = EW.mod_x_f32s(x.cpu(), s.cpu(), dtype) if scaled else x.double().cpu()
        rm, sl = EW.wgrad_ref(gd, xm, [A, B, 3, 3], padding=1)
    _ew(dw, rm, sl, torch.float32, f'wgrad3x3 {shape} scaled={scaled} {kernel} {str(dtype)[6:]}')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('s2p', ['1', '0'])
def test_det_poisoned_wgrad_s2(dtype, s2p, monkeypatch):
    """The stride-2 halo weight gradient's slots, pipelined 16 x 6 form (SG2_WGRAD_S2P=1: 2 x 3 tiles a sample, 12 in
    all, 3 splits of 4) and 16 x 8 form (0: 2 x 2 tiles a sample, 8 in all, 2 splits of 4), on test_wgrad_halo_phases'
    conv_s2 (2 x 64 x 33 x 41 -> 72 x 16 x 20: ragged tiles, Cout 72 a partial channel block), its reference and
    tolerance."""
    from torch_utils.ops import conv2d_gradfix as cg
    monkeypatch.setenv('SG2_WGRAD_S2P', s2p)
    g0 = torch.Generator().manual_seed(31)
    N, Ci, Co = 2, 64, 72
    x = _nhwc(torch.randn(N, Ci, 33, 41, generator=g0), dtype)
    g = _nhwc(torch.randn(N, Co, 16, 20, generator=g0), dtype)
    dw, = _det_poisoned(lambda: [cg._wgrad_raw(g, x, 3, 3, 2, (0, 0))])
    rm, sl = EW.wgrad_ref(g.double().cpu(), x.double().cpu(), [Co, Ci, 3, 3], stride=2)
    assert rel_err(dw, rm) < (2e-3 if dtype == torch.float16 else 1e-2)
    _ew(dw, rm, sl, torch.float32, f'wgrad s2 s2p={s2p} {str(dtype)[6:]}')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('geom', [(45, 33, 1, 0, 3, 9, 7), (20, 37, 2, 0, 3, 9, 7), (3, 70, 3, 1, 3, 9, 7),
                                  (48, 512, 3, 1, 2, 4, 4)])
def test_det_poisoned_conv_generic(dtype, geom):
    """The implicit-GEMM conv's dot and split-K slots and the generic weight gradient's pixel-split slots (conv.hip
    SG2_DET_GET sites) at test_pack_weight's ragged channel counts (Cout, Cin, k) on a 9 x 7 image, and the split-K
    512-channel 4 x 4 layer with Cout = 48.  Tolerances: test_conv_fused_dot_and_scale's (1e-5 f32, 5e-3 fp16) for the
    output and the dot, test_conv2d_fwd_bwd's for the weight gradient (2e-5 f32, 8e-3 fp16)."""
    from torch_utils.ops import conv2d_gradfix as cg
    Cout, Cin, k, pad, N, H, W = geom
    g0 = torch.Generator().manual_seed(29)
    x = _nhwc(torch.randn(N, Cin, H, W, generator=g0), dtype)
    w = (torch.randn(Cout, Cin, k, k, generator=g0) / (Cin * k * k) ** 0.5).to(DEV).to(dtype)
    oh, ow = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    s = (torch.rand(N, Cout, generator=g0) + 0.5).to(DEV)
    src = _nhwc(torch.randn(N, Cout, oh, ow, generator=g0), dtype)
    gr = _nhwc(torch.randn(N, Cout, oh, ow, generator=g0), dtype)
    wp = cg._pack_conv(w)

    def fn():
        y, _, dot = cg.conv_fused(x, wp, Cout, oh, ow, k, k, 1, (pad, pad), out_scale=s, dot_src=src)
        return [y, dot, cg._wgrad_raw(gr, x, k, k, 1, (pad, pad))]
    y, dot, dw = _det_poisoned(fn)
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), padding=pad)
    tol = 1e-5 if dtype == torch.float32 else 5e-3
    assert rel_err(y.float(), ref * s.double().cpu()[:, :, None, None]) < tol
    assert rel_err(dot, (ref.to(dtype).double() * src.double().cpu()).sum([2, 3])) < tol
    dwr = torch.nn.grad.conv2d_weight(x.double().cpu(), [Cout, Cin, k, k], gr.double().cpu(), padding=pad)
    assert rel_err(dw, dwr) < (2e-5 if dtype == torch.float32 else 8e-3)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('direct', ['1', '0'])
def test_det_poisoned_halo_tile_dot(dtype, direct, monkeypatch):
    """The halo kernel's per-tile dot slots (conv3x3.hip launch_halo_tiles) at (2, 64, 20, 37, 96): ragged right and
    bottom pixel tiles, Cout no multiple of 64, both epilogues (SG2_HALO_DIRECT); the dgrad form of
    test_conv3x3_halo_direct, its reference and tolerances."""
    from torch_utils.ops import conv2d_gradfix as cg
    monkeypatch.setenv('SG2_HALO_DIRECT', direct)
    monkeypatch.setenv('SG2_C64_RING', '0')
    N, Cin, H, W, Cout = 2, 64, 20, 37, 96
    g0 = torch.Generator().manual_seed(13)
    x = _nhwc(torch.randn(N, Cin, H, W, generator=g0), dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g0) / np.sqrt(Cin * 9)).to(DEV).to(dtype)
    d = (torch.rand(N, Cout, generator=g0) + 0.5).to(DEV)
    src = _nhwc(torch.randn(N, Cout, H, W, generator=g0), dtype)
    wp = cg._pack_conv(w)

    def fn():
        y, _, dot = cg.conv3x3_fused(x, wp, Cout, out_scale=d, dot_src=src)
        return [y, dot]
    y, dot = _det_poisoned(fn)
    xd, wd = x.double().cpu(), w.double().cpu()
    c0 = F.conv2d(xd, wd, padding=1)
    sl0 = EW.accumulation_slack(9 * Cin, F.conv2d(xd.abs(), wd.abs(), padding=1))
    dd = d.double().cpu()[:, :, None, None]
    tol = 5e-3 if dtype == torch.float16 else 2e-2
    assert rel_err(y.float(), c0 * dd) < tol
    assert rel_err(dot, (c0.to(dtype).double() * src.double().cpu()).sum([2, 3])) < tol
    _ew(y, c0 * dd, EW.epilogue_slack(sl0, c0, dd), dtype, f'halo direct={direct} dgrad out_scale {str(dtype)[6:]}')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', [(3, 64, 7, 512), (1, 8, 40, 24), (1, 91, 91, 512)])
def test_det_poisoned_det_sum_chunks(dtype, shape):
    """sg2_dot_hw and sg2_layer_bwd (N, H, W, C) through det_sum / det_sum_multi from a poisoned scratch, the chunk
    temporaries included.  The chunk pass runs when bx G < 512 and S > 64 (det.hip), S the pixel blocks a sample
    (times N for the bias gradient): (3, 64, 7, 512) gives S = 4 (dot_hw: 128 pixels a block), 7 and 21 (layer_bwd: 64
    a block); (1, 8, 40, 24) one block -- both sum in one launch.  (1, 91, 91, 512), 8281 pixels, reaches it with a
    short last chunk: dot_hw S = 65, K = min(ceil(65 / 64), ceil(512 / 8)) = 2 chunks of 33 and 32; layer_bwd
    S = 130 for both the bias (n = 512) and the demodulation (n = 512) gradients, K = 3 chunks of 44, 44, 42.
    References in float64; tolerances of test_dot_hw (1e-5) and test_layer_bwd (dc 5e-3 / 2e-2 and elementwise; db,
    dd, dnoise 1e-4)."""
    from torch_utils.ops import conv2d_gradfix as cg
    N, H, W, C = shape
    g0 = torch.Generator().manual_seed(3)
    y, c, dy = (_nhwc(torch.randn(N, C, H, W, generator=g0) * (2 if i == 0 else 1), dtype) for i in range(3))
    d = (torch.rand(N, C, generator=g0) + 0.5).to(DEV)
    dot, = _det_poisoned(lambda: [cg.dot_hw(y, c)])
    assert rel_err(dot, (y * c).double().cpu().sum([2, 3])) < 1e-5        # the product rounded to 16 bits, then summed
    dc, db, dd, dn = _det_poisoned(lambda: list(cg.layer_bwd(dy, y, c, d, act=1, alpha=0.2, gain=1.5, clamp=2.5)))
    yd = y.double().cpu()
    dz = (dy.double().cpu() * 1.5 * torch.where(yd > 0, 1.0, float(np.float32(0.2))) * ((yd > -2.5) & (yd < 2.5)).double())
    ref = dz * d.double().cpu()[:, :, None, None]
    assert rel_err(dc.float(), ref) < (5e-3 if dtype == torch.float16 else 2e-2)
    assert rel_err(db, dz.sum([0, 2, 3])) < 1e-4
    assert rel_err(dd, (dz * c.double().cpu()).sum([2, 3])) < 1e-4
    assert rel_err(dn, dz.sum(1, keepdim=True)) < 1e-4
    _ew(dc, ref, 3 * EW.EPS32 * ref.abs(), dtype, f'layer_bwd dc {shape} {str(dtype)[6:]}')


def test_det_sum_order_ignores_alignment():
    """det_sum's order must follow from the shapes alone (sg2_common.h): one weight gradient added into a zeroed
    accumulator at a 16-byte aligned offset and at a 4-byte one gives the same bits (or the misaligned call is
    refused with a clear sg2_last_error).  2 x 64 x 64 x 64 -> 64, fp16: 32 x 8 tiles, 16 a sample, 32 in all, one
    channel block: splits = min(256, 32 / 4) = 8, where adding s = 0..7 in sequence (the vec4 form: S <= 16,
    n = 64 x 9 x 64 = 36864 = 576 x 64 outputs, a multiple of 4) and four interleaved row sums differ."""
    from torch_utils.ops import conv2d_gradfix as cg
    N, A, B, H, W = 2, 64, 64, 64, 64
    g0 = torch.Generator().manual_seed(7)
    g = _nhwc(torch.randn(N, A, H, W, generator=g0), torch.float16)
    x = _nhwc(torch.randn(N, B, H, W, generator=g0), torch.float16)
    n = A * 9 * B
    acc = torch.zeros([n + 4], dtype=torch.float32, device=DEV)
    assert acc.data_ptr() % 16 == 0
    out = []
    with sg2hip.deterministic():
        for off in (0, 1):
            acc.zero_()
            poison.poison_det_scratch(DEV)
            try:
                dw = cg._wgrad_raw(g, x, 3, 3, 1, (1, 1), out=acc[off:off + n])
            except RuntimeError as e:
                assert off == 1 and 'align' in str(e), e       # a refusal must say why
                return
            assert dw.data_ptr() == acc.data_ptr() + 4 * off
            out.append(dw.clone())
            assert float(acc[:off].abs().sum()) == 0 and float(acc[off + n:].abs().sum()) == 0, 'wrote outside its slice'
    ref = torch.nn.grad.conv2d_weight(x.double().cpu(), [A, B, 3, 3], g.double().cpu(), padding=1)
    assert rel_err(out[0], ref) < 2e-3 and rel_err(out[1], ref) < 2e-3
    ndiff = int((out[0] != out[1]).sum())
    assert torch.equal(out[0], out[1]), f'{ndiff} of {n} sums differ in bits between the aligned and the offset output'
