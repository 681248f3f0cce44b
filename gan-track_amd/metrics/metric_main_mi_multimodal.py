"""Metric registry of the training loop.  Drop-in for SG3/metrics/metric_main_mi_multimodal.py:27-95: the module
keeps the reference's entry points (register_metric, is_valid_metric, list_valid_metrics, calc_metric,
report_metric) and its output contract (one JSON line per evaluation appended to
<run_dir>/metric-<modality>-<metric>.jsonl); the FID metrics are the two the Claro / Pelvis runs name, the
precision / recall metrics (pr50k3_full, pr50k3) the one further metric the reference adapted to its per-modality
evaluation, and ppl2_wend the perceptual path length and kid50k the kernel inception distance its offline
evaluation (calc_metrics_mi_multimodal.py) names.  prdc50k5_full and prdc50k5 (precision, recall, density and
coverage, Naeem et al. 2020) are this project's own: the reference has no such metric."""
import json
import os
import time

import torch

import dnnlib
from . import metric_utils
from . import frechet_inception_distance
from . import precision_recall
from . import perceptual_path_length
from . import kernel_inception_distance
from . import density_coverage


class _Registry:
    """Metric name -> function(opts) -> {result name: float}; insertion-ordered."""

    def __init__(self):
        self.fns = {}

    def add(self, fn):
        if not callable(fn):
            raise AssertionError(f'metric {fn!r} is not callable')
        self.fns[fn.__name__] = fn
        return fn

    def check(self, name):
        if name not in self.fns:
            raise AssertionError(f'unknown metric {name!r}; valid: {sorted(self.fns)}')
        return self.fns[name]


_REGISTRY = _Registry()
register_metric = _REGISTRY.add


def is_valid_metric(metric):
    return metric in _REGISTRY.fns


def list_valid_metrics():
    return list(_REGISTRY.fns)


def _rank0_value(value, opts):
    """Every rank reports rank 0's number (the detector statistics are only complete there)."""
    if opts.num_gpus <= 1:
        return value
    t = torch.tensor(float(value), dtype=torch.float64, device=opts.device)
    torch.distributed.broadcast(t, src=0)
    return float(t.item())


def calc_metric(metric, **kwargs):
    """Evaluate one registered metric; returns {results, metric, total_time, total_time_str, num_gpus}."""
    fn = _REGISTRY.check(metric)
    opts = metric_utils.MetricOptions(**kwargs)
    start = time.time()
    raw = fn(opts)
    elapsed = time.time() - start
    results = dnnlib.EasyDict({name: _rank0_value(v, opts) for name, v in raw.items()})
    return dnnlib.EasyDict(results=results, metric=metric, total_time=elapsed,
                           total_time_str=dnnlib.util.format_time(elapsed), num_gpus=opts.num_gpus)


def report_metric(result_dict, mode, run_dir=None, snapshot_pkl=None):
    """Print the evaluation as one JSON line and append it to the run's per-modality metric log."""
    _REGISTRY.check(result_dict['metric'])
    result_dict['mode'] = mode
    rel = os.path.relpath(snapshot_pkl, run_dir) if (run_dir is not None and snapshot_pkl is not None) else snapshot_pkl
    record = dict(result_dict)
    record.update(snapshot_pkl=rel, timestamp=time.time())
    text = json.dumps(record)
    print(text)
    if run_dir is None or not os.path.isdir(run_dir):
        return
    path = os.path.join(run_dir, 'metric-%s-%s.jsonl' % (mode, result_dict['metric']))
    with open(path, 'at') as log:
        log.write(text + '\n')


def _fid(opts, name, max_real, xflip):
    """FID against all (max_real None) or 50k real images, 50k generated."""
    opts.dataset_kwargs.update(max_size=None)
    if xflip is not None:
        opts.dataset_kwargs.update(xflip=xflip)
    return {name: frechet_inception_distance.compute_fid(opts, max_real=max_real, num_gen=50000)}


@register_metric
def fid50k_full(opts):
    return _fid(opts, 'fid50k_full', None, False)


@register_metric
def fid50k(opts):
    return _fid(opts, 'fid50k', 50000, None)


@register_metric
def pr50k3_full(opts):
    """Precision / recall, k = 3, against up to 200k real images (SG3/metrics/metric_main_mi_multimodal.py:103-106)."""
    opts.dataset_kwargs.update(max_size=None, xflip=False)
    precision, recall = precision_recall.compute_pr(opts, max_real=200000, num_gen=50000, nhood_size=3,
                                                    row_batch_size=10000, col_batch_size=10000)
    return dict(pr50k3_full_precision=precision, pr50k3_full_recall=recall)


@register_metric
def pr50k3(opts):
    """Precision / recall, k = 3, against 50k real images (:147-150)."""
    opts.dataset_kwargs.update(max_size=None)
    precision, recall = precision_recall.compute_pr(opts, max_real=50000, num_gen=50000, nhood_size=3,
                                                    row_batch_size=10000, col_batch_size=10000)
    return dict(pr50k3_precision=precision, pr50k3_recall=recall)


@register_metric
def ppl2_wend(opts):
    """Perceptual path length in W, path endpoints, full image (:108-111)."""
    ppl = perceptual_path_length.compute_ppl(opts, num_samples=50000, epsilon=1e-4, space='w', sampling='end',
                                             crop=False, batch_size=2)
    return dict(ppl2_wend=ppl)


@register_metric
def kid50k(opts):
    """Kernel inception distance, 100 subsets of up to 1000, against 50k real images (:141-144).  (kid50k_full --
    the same with xflip off and the cap on the real set lifted to 10^6 -- draws from the same real set on every
    dataset below 50 000 images and is not registered.)"""
    opts.dataset_kwargs.update(max_size=None)
    kid = kernel_inception_distance.compute_kid(opts, max_real=50000, num_gen=50000, num_subsets=100,
                                                max_subset_size=1000)
    return dict(kid50k=kid)


def _prdc(opts, name, max_real):
    results = density_coverage.compute_prdc(opts, max_real=max_real, num_gen=50000, nhood_size=5)
    return {f'{name}_{key}': results[key] for key in ('precision', 'recall', 'density', 'coverage')}


@register_metric
def prdc50k5_full(opts):
    """Precision, recall, density and coverage, k = 5 (the paper's), against up to 200k real images."""
    opts.dataset_kwargs.update(max_size=None, xflip=False)
    return _prdc(opts, 'prdc50k5_full', 200000)


@register_metric
def prdc50k5(opts):
    """The same against 50k real images."""
    opts.dataset_kwargs.update(max_size=None)
    return _prdc(opts, 'prdc50k5', 50000)
