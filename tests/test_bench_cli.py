"""bench.py's command line and its --dump-outputs writer, on the host: a plain run asks for none of the extra
measurements (--full is off by default and switches them on), and dump_outputs writes every parameter and float
buffer of G, D and G_ema, the ADA p and pl_mean as float32 .npy files -- small tensors whole, large ones as the
same sorted sample of elements in every call, the whole dump inside its byte budget."""
import os
import sys
import types

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '5', '--warmup', '2')
    assert (a.gpus, a.steps, a.warmup) == (1, 5, 2)
    assert a.full is False and a.dump_outputs is None
    b = _parse(monkeypatch, '--full', '--dump-outputs', 'some/dir')
    assert b.full is True and b.dump_outputs == 'some/dir'


class _Net(torch.nn.Module):
    def __init__(self, seed, big):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.weight = torch.nn.Parameter(torch.randn(big, generator=g).reshape(-1, 4))
        self.bias = torch.nn.Parameter(torch.randn(7, generator=g))
        self.register_buffer('w_avg', torch.randn(3, 5, generator=g).double())
        self.register_buffer('count', torch.arange(3))          # not floating point: left out


def _trainer():
    big = bench.DUMP_SAMPLE + 4000
    return types.SimpleNamespace(G=_Net(1, big), D=_Net(2, big), G_ema=_Net(3, big),
                                 augment_pipe=types.SimpleNamespace(p=torch.tensor(0.2)),
                                 loss=types.SimpleNamespace(pl_mean=torch.tensor(1.5)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs(tmp_path):
    tr = _trainer()
    bench.dump_outputs(tr, str(tmp_path / 'a'))
    bench.dump_outputs(tr, str(tmp_path / 'b'))
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert set(a) == {f'{n}.{k}' for n in ('G', 'D', 'G_ema') for k in ('weight', 'bias', 'w_avg')} | \
        {'augment_pipe.p', 'loss.pl_mean'}
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for n, m in (('G', tr.G), ('D', tr.D), ('G_ema', tr.G_ema)):
        assert np.array_equal(a[f'{n}.bias'], m.bias.detach().numpy())
        assert a[f'{n}.w_avg'].shape == (3, 5) and np.array_equal(a[f'{n}.w_avg'], m.w_avg.float().numpy())
        full, got = m.weight.detach().numpy().reshape(-1), a[f'{n}.weight']
        assert got.shape == (bench.DUMP_SAMPLE,)
        idx = np.sort(np.random.default_rng(0).choice(full.size, bench.DUMP_SAMPLE, replace=False))
        assert np.array_equal(got, full[idx])
    assert float(a['augment_pipe.p']) == np.float32(0.2) and float(a['loss.pl_mean']) == 1.5


def test_dump_outputs_keeps_its_budget(tmp_path, monkeypatch):
    tr = _trainer()
    monkeypatch.setattr(bench, 'DUMP_BUDGET', 11 * 4 * 100)     # 11 tensors: 100 elements each at the most
    bench.dump_outputs(tr, str(tmp_path))
    a = _load(tmp_path)
    assert len(a) == 11 and max(v.size for v in a.values()) == 100
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
