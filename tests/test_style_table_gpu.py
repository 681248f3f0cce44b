"""The style path of a synthesis pass in table launches (networks_stylegan2._StyleTable on sg2_style_table,
SG2_STYLE_TABLE) against the per-layer route it stands in for (_prenorm / _demod per layer: SG2_STYLE_TABLE=0).

A table job runs the body of its single-layer kernel, so every value -- w_n, s_n, d, the first-order g_w and g_s, and
the second order through the create_graph nodes -- must be bitwise the per-layer route's, NaN patterns included.  The
forward values are also held to the references and bounds of test_ops_gpu.py::test_infnorm_prenorm (the reference
expression in f32, bit-exact) and ::test_demod_kernel (float64, 1e-5).  Outputs are allocated NaN-poisoned
(tests/poison.py), so an element no job writes fails the comparison."""
import numpy as np
import pytest
import torch

import poison
from golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
N = 3


@pytest.fixture(autouse=True)
def _poisoned_empties(request, monkeypatch):
    poison.poisoned_empties(monkeypatch, poison.op_modules(request.node.originalname))


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=lambda m: f'{what}: {m}')


def _mixed_layers():
    """(weight, styles, prenorm) of the mixed table: two fp16 3x3 layers, (8, 8) and (24, 16); an f32 3x3 layer
    (8, 8), demod only; a copy of the first with an all-zero weight row.  Layer 0 has a weight row with two equal
    maxima of opposite sign, a style row whose maximum is its first element and one whose maximum is its last.
    A 1x1 toRGB-style layer (no demodulation) has no entry here: style_table_pass knows demodulated layers only, and
    what keeps such a layer out of the table is the selection in SynthesisNetwork._style_table, which
    test_network_passes_bitwise holds to (its 16^2 network has three toRGB layers and five jobs, none of them theirs)."""
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    w0, s0 = mk(8, 8, 3, 3), mk(N, 8)
    w0[2, 5, 1, 1] = w0[2].abs().max() + 1.0
    w0[2, 7, 0, 2] = -w0[2, 5, 1, 1]
    s0[0, 0] = s0[0].abs().max() + 0.5
    s0[1, 7] = -(s0[1].abs().max() + 0.5)
    w1, s1 = mk(24, 16, 3, 3), mk(N, 16)
    w2, s2 = mk(8, 8, 3, 3), mk(N, 8)
    w3, s3 = w0.clone(), mk(N, 8)
    w3[5] = 0
    return [(w0, s0, True), (w1, s1, True), (w2, s2, False), (w3, s3, True)]


def _leaves(layers):
    return [(w.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True), p) for w, s, p in layers]


def _per_layer(net, layers):
    """The per-layer route: what SynthesisLayer.forward computes for one layer with the switch off."""
    res = []
    for w, s, pre in layers:
        wq, sq = net._prenorm(w, s) if pre else (w, s)
        res.append((wq, sq, net._demod(wq, sq)))
    return res


def _outputs(res, layers):
    """The differentiable outputs of a route, in one order: per layer (w_n, s_n, d) where prenorm, else (d,)."""
    return [t for r, (_, _, pre) in zip(res, layers) for t in (r if pre else r[2:])]


def _grad_outputs(layers, seed):
    """Random d w_n (a permuted view, as a weight-gradient kernel returns it, for every second layer), d s_n and dd."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, (w, s, pre) in enumerate(layers):
        o, i, kh, kw = w.shape
        if pre:
            gw = torch.randn(o, kh, kw, i, generator=g).to(DEV).permute(0, 3, 1, 2) if k % 2 == 0 else \
                torch.randn(o, i, kh, kw, generator=g).to(DEV)
            out += [gw, torch.randn(s.shape[0], i, generator=g).to(DEV)]
        out.append(torch.randn(s.shape[0], o, generator=g).to(DEV))
    return out


def _first_order(net, route, layers, seed=11):
    lv = _leaves(layers)
    res = route(lv)
    outs = _outputs(res, lv)
    with torch.no_grad():
        gos = _grad_outputs(layers, seed)
    grads = torch.autograd.grad(outs, [t for w, s, _ in lv for t in (w, s)], gos)
    return res, grads


def test_mixed_table_forward_and_first_order_bitwise():
    from training import networks_stylegan2 as net
    layers = _mixed_layers()
    ref, g_ref = _first_order(net, lambda lv: _per_layer(net, lv), layers)
    got, g_got = _first_order(net, net.style_table_pass, layers)
    for k, (r, t) in enumerate(zip(ref, got)):
        for name, a, b in zip(('w_n', 's_n', 'd'), r, t):
            _same(b.detach(), a.detach(), f'layer {k} {name}')
    for k, (a, b) in enumerate(zip(g_ref, g_got)):
        _same(b, a, f'layer {k // 2} {"g_w" if k % 2 == 0 else "g_s"}')
    # the closed forms: the reference expression in f32 (bit-exact, as test_infnorm_prenorm) and float64 (1e-5, as
    # test_demod_kernel), on the layers without the zero row
    for (w, s, pre), (wq, sq, d) in zip(layers[:3], got[:3]):
        wd, sd = w.to(DEV), s.to(DEV)
        if pre:
            o, i, kh, kw = w.shape
            wr = wd * (1 / np.sqrt(i * kh * kw) / wd.norm(float('inf'), dim=[1, 2, 3], keepdim=True))
            sr = sd / sd.norm(float('inf'), dim=1, keepdim=True)
            assert torch.equal(wq.detach(), wr) and torch.equal(sq.detach(), sr)
        w64, s64 = wq.detach().double().cpu(), sq.detach().double().cpu()
        d64 = ((w64[None] * s64[:, None, :, None, None]).square().sum([2, 3, 4]) + 1e-8).rsqrt()
        assert rel_err(d.detach().double().cpu(), d64) < 1e-5


def test_more_jobs_than_one_table_holds():
    """65 tiny fp16 layers: 130 pre-normalisation jobs and 65 demodulations forward, 130 + 130 backward -- every
    stage is split into several launches, with jobs on both sides of each seam."""
    from training import networks_stylegan2 as net
    g = torch.Generator().manual_seed(5)
    layers = [(torch.randn(8, 8, 3, 3, generator=g), torch.randn(N, 8, generator=g), True) for _ in range(65)]
    ref, g_ref = _first_order(net, lambda lv: _per_layer(net, lv), layers)
    got, g_got = _first_order(net, net.style_table_pass, layers)
    for k, (r, t) in enumerate(zip(ref, got)):
        for name, a, b in zip(('w_n', 's_n', 'd'), r, t):
            _same(b.detach(), a.detach(), f'layer {k} {name}')
    for k, (a, b) in enumerate(zip(g_ref, g_got)):
        _same(b, a, f'layer {k // 2} {"g_w" if k % 2 == 0 else "g_s"}')


@pytest.mark.parametrize('no_wgrad', [True, False])
def test_create_graph_second_order_bitwise(no_wgrad):
    """A two-layer stack (an fp16 layer and an f32 layer in one table): the first pass with grad mode on -- for the
    styles alone under no_weight_gradients (the path-length form, _DemodVJP) or for weights and styles (the composed
    form) -- then the second order into every weight and style.  Both routes run the same nodes."""
    from training import networks_stylegan2 as net
    from torch_utils.ops import conv2d_gradfix as cg
    layers = _mixed_layers()[1:3]

    def run(route):
        lv = _leaves(layers)
        outs = _outputs(route(lv), lv)
        with torch.no_grad():
            gos = _grad_outputs(layers, 13)
        y = sum((o * g).sum() for o, g in zip(outs, gos))
        ws, ss = [w for w, _, _ in lv], [s for _, s, _ in lv]
        with cg.no_weight_gradients(no_wgrad):
            first = torch.autograd.grad(y, ss if no_wgrad else ss + ws, create_graph=True)
        z = sum(f.square().sum() for f in first) + sum(o.square().sum() for o in outs)
        second = torch.autograd.grad(z, ws + ss)
        return [f.detach() for f in first] + list(second)

    ref = run(lambda lv: _per_layer(net, lv))
    got = run(net.style_table_pass)
    for k, (a, b) in enumerate(zip(ref, got)):
        _same(b, a, f'gradient {k}')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_packs_of_table_weights_bitwise(dtype):
    """The forward pack and the flipped / transposed packs of the table's w_n equal those of the per-layer _prenorm.
    The packs themselves are not served from a table here (each is still its own sg2_pack_weight launch on either
    route), so this pins only that the table's w_n enters the same packs with the same bits."""
    from training import networks_stylegan2 as net
    from torch_utils.ops import conv2d_gradfix as cg
    layers = [(w.to(DEV), s.to(DEV), p) for w, s, p in _mixed_layers()]
    with torch.no_grad():
        got = net.style_table_pass(layers)
        for (w, s, pre), (wq, _, _) in zip(layers, got):
            if not pre:
                continue
            wr = net._prenorm(w, s)[0]
            for pack in (lambda t: cg._pack_conv(t, dtype), lambda t: cg._pack_convT(t, dtype, flip=True),
                         lambda t: cg._pack_convT(t, dtype), lambda t: cg._pack_conv(t.transpose(0, 1), dtype)):
                _same(pack(wq), pack(wr), 'pack')


def test_refuses_inputs_it_could_not_differentiate_twice():
    """A non-contiguous or non-f32 weight / style would be saved as a converted copy without autograd history (the
    create_graph backward differentiates through the saved inputs): refused, not converted."""
    from training import networks_stylegan2 as net
    w, s = torch.randn(8, 8, 3, 3, device=DEV), torch.randn(N, 8, device=DEV)
    for bad_w, bad_s in [(w.double(), s), (w, s.half()), (w.transpose(0, 1), s), (w, torch.randn(8, N, device=DEV).t())]:
        with pytest.raises(RuntimeError, match='contiguous float32'):
            net.style_table_pass([(bad_w, bad_s, True)])


def _tiny_synthesis(net):
    torch.manual_seed(7)
    G = net.SynthesisNetwork(w_dim=32, img_resolution=16, img_channels=3, channel_base=256, channel_max=64,
                             num_fp16_res=2).to(DEV).requires_grad_(True)
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.1)
    return G


def test_network_passes_bitwise(monkeypatch):
    """A 16^2 synthesis network (an f32 block, two fp16 blocks; the toRGB layers are not demodulated and make no job):
    the image, every first-order parameter gradient, and the path-length pass (create_graph into ws, then the second
    order into the parameters) are bitwise the same with the table and per layer."""
    import sg2hip
    from training import networks_stylegan2 as net
    from torch_utils.ops import conv2d_gradfix as cg
    G = _tiny_synthesis(net)
    calls = []
    real = net.style_table_pass
    monkeypatch.setattr(net, 'style_table_pass', lambda layers: calls.append(layers) or real(layers))
    ws0 = torch.randn(N, G.num_ws, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    pl_noise = torch.randn(N, 3, 16, 16, generator=torch.Generator().manual_seed(2)).to(DEV)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(net, 'style_table', on)
        with sg2hip.deterministic(True, device=DEV):
            ws = ws0.clone().requires_grad_(True)
            img = G(ws, noise_mode='const')
            grads = torch.autograd.grad(img.square().sum(), list(G.parameters()) + [ws], allow_unused=True)
            ws2 = ws0.clone().requires_grad_(True)
            img2 = G(ws2, noise_mode='const')
            with cg.no_weight_gradients():
                pl, = torch.autograd.grad((img2 * pl_noise).sum(), [ws2], create_graph=True)
            grads2 = torch.autograd.grad(pl.square().sum(2).mean(1).sqrt().sum(), list(G.parameters()),
                                         allow_unused=True)
        res[on] = [img.detach(), pl.detach()] + list(grads) + list(grads2)
    assert len(calls) == 2                                        # one table per pass, only with the switch on
    assert [p for _, _, p in calls[0]] == [False, True, True, True, True]   # b4.conv1 | b8, b16: conv0, conv1
    assert len(res[True]) == len(res[False])
    for k, (a, b) in enumerate(zip(res[False], res[True])):
        assert (a is None) == (b is None), f'tensor {k}'
        if a is not None:
            _same(b, a, f'tensor {k}')
