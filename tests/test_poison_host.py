"""tests/poison.py on the CPU: the torch proxy NaN-fills floating-point empty / empty_like and nothing else, and the
blind spot it closes, stated as a test -- a "kernel" that leaves one element of its torch.empty output unwritten
passes every judge of the suite while the allocator hands it the previous, correct result's block, and fails each
of them under the poison."""
import types

import pytest
import torch

import elementwise as EW
import poison
from golden_util import rel_err


def _module():
    """A stand-in op module: `torch` is a global, looked up at call time, also inside an autograd Function."""
    mod = types.ModuleType('fake_op')
    mod.torch = torch
    src = '''
def alloc(*shape, **kw):
    return torch.empty(*shape, **kw)

def alloc_like(t, **kw):
    return torch.empty_like(t, **kw)

class Twice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip):
        y = torch.empty_like(x)
        flat, src = y.view(-1), (2 * x).view(-1)
        keep = torch.ones(flat.numel(), dtype=torch.bool)
        if skip is not None:
            keep[skip] = False
        flat[keep] = src[keep]              # the "kernel": writes all but element `skip`
        return y

    @staticmethod
    def backward(ctx, g):
        gx = torch.empty_like(g)
        gx.copy_(2 * g)
        return gx, None

def is_tensor(x):
    return isinstance(x, torch.Tensor)
'''
    exec(compile(src, 'fake_op', 'exec'), mod.__dict__)
    return mod


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_proxy_fills_float_empties(dtype, monkeypatch):
    mod = _module()
    poison.poisoned_empties(monkeypatch, [mod])
    a = mod.alloc([3, 5, 7], dtype=dtype)
    assert a.dtype == dtype and a.shape == (3, 5, 7) and bool(torch.isnan(a).all())
    b = mod.alloc(2, 4, dtype=dtype)                       # sizes as positional integers
    assert b.shape == (2, 4) and bool(torch.isnan(b).all())
    cl = mod.alloc([2, 8, 5, 3], dtype=dtype, memory_format=torch.channels_last)
    assert cl.is_contiguous(memory_format=torch.channels_last) and bool(torch.isnan(cl).all())
    like = mod.alloc_like(cl)
    assert like.dtype == dtype and like.is_contiguous(memory_format=torch.channels_last)
    assert bool(torch.isnan(like).all())
    scalar = mod.alloc((), dtype=dtype)
    assert scalar.shape == () and bool(torch.isnan(scalar))
    assert bool(torch.isnan(mod.alloc_like(torch.zeros(6, dtype=torch.int32), dtype=dtype)).all())


@pytest.mark.parametrize('dtype', [torch.int32, torch.uint8, torch.int64, torch.bool])
def test_proxy_leaves_integers_alone(dtype, monkeypatch):
    mod = _module()
    poison.poisoned_empties(monkeypatch, [mod])
    a = mod.alloc([4, 3], dtype=dtype)
    assert a.dtype == dtype and a.shape == (4, 3)
    src = torch.arange(12).reshape(4, 3).to(dtype)
    like = mod.alloc_like(src)
    assert like.dtype == dtype and like.shape == src.shape
    assert torch.equal(src, torch.arange(12).reshape(4, 3).to(dtype)), 'empty_like wrote to its argument'


def test_proxy_forwards_everything_else(monkeypatch):
    mod = _module()
    proxy = poison.poisoned_empties(monkeypatch, [mod])
    assert mod.torch is proxy and proxy is not torch
    assert mod.is_tensor(torch.zeros(1)) and not mod.is_tensor(3.0)
    assert proxy.Tensor is torch.Tensor and proxy.float16 is torch.float16 and proxy.cuda is torch.cuda
    assert proxy.autograd.Function is torch.autograd.Function and proxy.channels_last is torch.channels_last
    assert proxy.zeros is torch.zeros and proxy.nn.functional is torch.nn.functional
    assert 'empty' in dir(proxy) and 'zeros' in dir(proxy)
    with pytest.raises(AttributeError):
        proxy.no_such_attribute
    # an autograd Function defined before the patch allocates through the proxy in forward and backward
    x = torch.arange(6.0).reshape(2, 3).requires_grad_(True)
    y = mod.Twice.apply(x, None)
    assert torch.equal(y, 2 * x.detach())
    g, = torch.autograd.grad(y.sum(), [x])
    assert torch.equal(g, torch.full_like(g, 2.0))
    with poison.unpoisoned([mod]):
        assert mod.torch is torch
    assert mod.torch is proxy


def test_patch_is_undone(monkeypatch):
    mod = _module()
    with monkeypatch.context() as m:
        poison.poisoned_empties(m, [mod])
        assert bool(torch.isnan(mod.alloc([3])).all())
    assert mod.torch is torch


def test_real_op_modules_resolve_torch_at_call_time(monkeypatch):
    """The five patched modules hold `torch` as a module global (what the proxy replaces)."""
    mods = poison._resolve(poison.OP_MODULES)
    poison.poisoned_empties(monkeypatch, mods)
    for m in mods:
        assert isinstance(m.torch, poison.TorchProxy), m.__name__
    assert set(poison.op_modules('test_conv3x3_fused')) == set(poison.OP_MODULES)
    for name in poison.DYNAMIC_EXTENT_TESTS:
        left = poison.op_modules(name)
        assert not set(left) & set(poison.DYNAMIC_EXTENT_MODULES) and len(left) == 3, name


def test_unwritten_element_blind_spot_and_cure(monkeypatch, capsys):
    """A stand-in kernel that writes all but one element of its torch.empty output.  Unpoisoned, straight after a
    correct run of the same size was freed, the stale value may survive in the reused block (informational: the CPU
    allocator need not reuse it); poisoned, rel_err, assert_elementwise and torch.equal each reject the result."""
    mod = _module()
    x = torch.randn(64, 129, generator=torch.Generator().manual_seed(0))
    ref = (2 * x).double()
    hole = 64 * 129 - 1                                    # the last element: a ragged tile corner
    good = mod.Twice.apply(x, None)
    assert torch.equal(good.double(), ref)
    del good
    stale = mod.Twice.apply(x, hole)
    survived = bool(stale.view(-1)[hole] == ref.view(-1)[hole].float())
    with capsys.disabled():
        print(f'\nunpoisoned: the unwritten element {"still holds the previous correct value" if survived else "differs"}'
              f' (rel_err {rel_err(stale, ref):.3g})')
    del stale

    poison.poisoned_empties(monkeypatch, [mod])
    bad = mod.Twice.apply(x, hole)
    assert bool(torch.isnan(bad.view(-1)[hole])) and int(torch.isnan(bad).sum()) == 1
    assert not rel_err(bad, ref) < 1e-5                    # the suite's form: `assert rel_err(...) < tol`
    with pytest.raises(AssertionError, match='1 of 8256 elements outside'):
        EW.assert_elementwise(bad, ref, 1e-3, torch.float32, 'stand-in')
    assert not torch.equal(bad, (2 * x))
    assert not torch.equal(bad, bad.clone())               # even against itself: a twice-run comparison fails
    # and a complete write passes all three under the poison
    ok = mod.Twice.apply(x, None)
    assert rel_err(ok, ref) < 1e-7 and torch.equal(ok, 2 * x)
    EW.assert_elementwise(ok, ref, 0.0, torch.float32, 'stand-in')
