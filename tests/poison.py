"""NaN poison for memory the kernels are trusted to overwrite (test infrastructure; a plain module, no plugin).

Every op wrapper allocates its outputs with torch.empty, and deterministic mode sums slots of a scratch that nothing
initialises, so correctness rests on every output element being assigned and every slot element that is read having
been written by the same call.  A comparison cannot see a violation while the unwritten element still holds a
plausible value: the caching allocator hands a torch.empty the block the previous case of the same shape just freed
(holding that case's correct result), and a fresh process' scratch is zero pages.  NaN is data, not an address -- no
launch, trip count or index changes -- and every judge of the suite rejects it: golden_util.rel_err turns NaN and
fails its `<`, elementwise.ratios maps a NaN in `got` to inf, torch.equal is false on NaN.

    poisoned_empties(monkeypatch, modules)   torch.empty / torch.empty_like of those modules return NaN-filled floats
    unpoisoned(modules)                      context: the real torch back in those modules
    poison_det_scratch(device)               NaN into sg2hip's registered deterministic scratch
    zero_det_scratch(device)                 zeros into it: what a fresh process sees (teardown)
    op_modules(test_name)                    the modules a test of the op files poisons

The deterministic scratch holds float partial sums only: DetArena::get returns float*, and every user (the
SG2_DET_GET sites of conv.hip, conv3x3.hip, wgrad3x3.hip, layer_bwd.hip and det_sum's chunk temporaries in det.hip)
stores slots that det_sum reads back as floats -- no counters, tickets or indices -- so a NaN fill changes no
address.

Left unpoisoned, because their buffers are partial by contract (only the dynamic extent is written, and only the
extent is read) or are not established to hold floats only:
    torch_utils/ops/reflect_pad.py, training/augment_mi.py (theta / ints)    never patched
    torch_utils/ops/manifold.py, ppl.py, noise_reg.py (k-NN / LPIPS / noise-regulariser scratches)    never patched
    upfirdn2d._raw_lim and grid_sample_gradfix._Bwd with dyn_hw: these share a module with fully written outputs, so
    the proxy stays off upfirdn2d and grid_sample_gradfix in the tests that drive the dynamic-extent route
    (DYNAMIC_EXTENT_TESTS), and inside `unpoisoned` for the dyn_hw call of test_affine_grid_sample.
The partial-by-contract buffers are checked in tests/test_ada_geom_gpu.py instead: there each test poisons
reflect_pad, upfirdn2d and grid_sample_gradfix in its own body and holds every kernel of the ADA geometric chain to
three regions -- computed within its bound, zero band exactly 0.0, the rest still NaN -- and feeds each consumer its
input as the producer leaves it (tests/ada_regions.py; the region arithmetic alone in test_ada_geom_host.py).
"""
import contextlib
import importlib

import torch

OP_MODULES = ('torch_utils.ops.conv2d_gradfix', 'torch_utils.ops.bias_act', 'torch_utils.ops.upfirdn2d',
              'torch_utils.ops.grid_sample_gradfix', 'training.networks_stylegan2')
# the modules whose dynamic-extent buffers are partial by contract
DYNAMIC_EXTENT_MODULES = ('torch_utils.ops.upfirdn2d', 'torch_utils.ops.grid_sample_gradfix')
# the tests (function names, without parameters) that drive the dynamic-extent route: the ADA pipe and dyn_hw
DYNAMIC_EXTENT_TESTS = frozenset([
    # test_ops_gpu.py
    'test_augment_golden',
    'test_augment_geometric_fused_matches_torch_algebra',
    'test_augment_dynamic_extent',
    # test_deterministic_gpu.py
    'test_det_affine_grid_sample_bwd',
    'test_det_gather_matches_scatter_ada_maps',
    'test_det_isolated_iteration_c2',        # a whole iteration: runs the ADA pipe
])
# test_ops_gpu.py::test_affine_grid_sample runs poisoned except for its one dyn_hw call (unpoisoned() in its body)


class TorchProxy:
    """Stands in for the name `torch` in a module's globals: every attribute is the real torch's, except empty and
    empty_like, which fill a floating-point result with NaN (integer and bool tensors pass through untouched)."""

    def __init__(self, real=torch):
        object.__setattr__(self, '_real', real)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, '_real'), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, '_real'), name, value)

    def __dir__(self):
        return dir(object.__getattribute__(self, '_real'))

    @staticmethod
    def _poison(t):
        if t.is_floating_point():
            with torch.no_grad():
                t.fill_(float('nan'))
        return t

    def empty(self, *args, **kwargs):
        return self._poison(torch.empty(*args, **kwargs))

    def empty_like(self, *args, **kwargs):
        return self._poison(torch.empty_like(*args, **kwargs))


def _resolve(modules):
    return [importlib.import_module(m) if isinstance(m, str) else m for m in modules]


def poisoned_empties(monkeypatch, modules):
    """Replace the name `torch` in each module (module objects or dotted names) by a TorchProxy until monkeypatch
    undoes it.  The wrappers and their autograd Functions look `torch` up in the module's globals at call time, so
    the proxy in the globals reaches every torch.empty they make."""
    proxy = TorchProxy()
    for mod in _resolve(modules):
        assert getattr(mod, 'torch', None) is torch or isinstance(getattr(mod, 'torch', None), TorchProxy), \
            f'{mod.__name__} has no global named torch'
        monkeypatch.setattr(mod, 'torch', proxy)
    return proxy


@contextlib.contextmanager
def unpoisoned(modules):
    """The real torch back in the modules' globals for the duration (a call whose output is partial by contract)."""
    mods = _resolve(modules)
    saved = [m.torch for m in mods]
    for m in mods:
        m.torch = torch
    try:
        yield
    finally:
        for m, t in zip(mods, saved):
            m.torch = t


def op_modules(test_name):
    """The modules the autouse fixtures of test_ops_gpu.py, test_halo_dma_gpu.py and test_deterministic_gpu.py
    poison for the test function `test_name`."""
    if test_name in DYNAMIC_EXTENT_TESTS:
        return [m for m in OP_MODULES if m not in DYNAMIC_EXTENT_MODULES]
    return list(OP_MODULES)


def _det_scratch(device):
    import sg2hip
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    if sg2hip._det_scratch.get(dev) is None:
        with sg2hip.deterministic(device=dev):
            pass
    return sg2hip._det_scratch[dev]


def poison_det_scratch(device):
    """NaN into every float of the registered deterministic scratch (one fill pass; stream-ordered, so it lands
    before the next kernel of the current stream)."""
    _det_scratch(device).fill_(float('nan'))


def zero_det_scratch(device):
    """Zeros into the scratch: the state a fresh process sees, so no later test depends on the poison."""
    import sg2hip
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    buf = sg2hip._det_scratch.get(dev)
    if buf is not None:
        buf.zero_()
