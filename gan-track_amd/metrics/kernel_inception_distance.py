"""Kernel Inception Distance (Binkowski et al. 2018, "Demystifying MMD GANs"), per modality
(SG3/metrics/kernel_inception_distance.py:18-44): the unbiased MMD^2 estimate between Inception features of real and
generated images under the kernel k(a, b) = (a.b / d + 1)^3, averaged over num_subsets random subsets of
m = min(n_real, n_gen, max_subset_size) rows each.

The subsets are drawn on the host from the global np.random in the reference's order (per subset: generated rows,
then real rows, both without replacement), so one numpy seed selects the same rows as the reference.  The sums run
on the fused MMD kernel (torch_utils/ops/poly_mmd.py: no gathered copy, no m x m matrix, float64 accumulation in a
fixed order); SG2_KID_FUSED=0 selects the reference's composition -- gather, `@`, cube and sum in float32 -- in torch
on the device, for A/B runs and timing.

Differences from the reference by design: both feature passes get `mode_dict` (per-modality evaluation, as FID and
precision / recall do; the reference's file omits it and cannot call its own metric_utils), and the Inception network
is supplied offline (SG2_FID_DETECTOR or metric_utils.register_detector), never downloaded."""
import os

import numpy as np
import torch

from torch_utils.ops import poly_mmd
from . import metric_utils
from . import frechet_inception_distance

DETECTOR_URL = frechet_inception_distance.DETECTOR_URL      # .../metrics/inception-2015-12-05.pkl: FID's network


def fused_default():
    return os.environ.get('SG2_KID_FUSED', '1') != '0'


def composed_subset_sums(gen, real, idx_gen, idx_real):
    """poly_mmd.subset_sums' result by the reference's composition, one subset at a time: float32 gather, three Gram
    matrices, `/ d + 1`, cube, float32 sums, the diagonal subtracted afterwards."""
    gen, real = gen.to(torch.float32), real.to(torch.float32)
    d = gen.shape[1]
    out = torch.empty([len(idx_gen), 3], dtype=torch.float64, device=gen.device)
    for s, (ig, ir) in enumerate(zip(idx_gen, idx_real)):
        x = gen[torch.as_tensor(np.asarray(ig), dtype=torch.int64, device=gen.device)]
        y = real[torch.as_tensor(np.asarray(ir), dtype=torch.int64, device=real.device)]
        kxx, kyy, kxy = (x @ x.T / d + 1) ** 3, (y @ y.T / d + 1) ** 3, (x @ y.T / d + 1) ** 3
        out[s, 0] = (kxx.sum() - kxx.diagonal().sum()).to(torch.float64)
        out[s, 1] = (kyy.sum() - kyy.diagonal().sum()).to(torch.float64)
        out[s, 2] = kxy.sum().to(torch.float64)
    return out


def kid_from_features(real_features, gen_features, num_subsets, max_subset_size, fused=None):
    """KID of two feature sets [n, d] on one device; draws 2 * num_subsets times from the global np.random."""
    n_real, n_gen = real_features.shape[0], gen_features.shape[0]
    m = min(min(n_real, n_gen), max_subset_size)
    idx_gen = np.empty([num_subsets, m], dtype=np.int64)
    idx_real = np.empty([num_subsets, m], dtype=np.int64)
    for s in range(num_subsets):
        idx_gen[s] = np.random.choice(n_gen, m, replace=False)
        idx_real[s] = np.random.choice(n_real, m, replace=False)
    if fused_default() if fused is None else fused:
        sums = poly_mmd.subset_sums(gen_features, real_features, idx_gen, idx_real)
    else:
        sums = composed_subset_sums(gen_features, real_features, idx_gen, idx_real)
    return poly_mmd.kid_from_sums(sums, m)


def compute_kid(opts, max_real, num_gen, num_subsets, max_subset_size):
    """The reference's signature and return value.  At num_gpus > 1 every rank holds the global feature set after
    FeatureStats.reduce(); rank 0 alone draws and computes, the others return nan (the registry broadcasts)."""
    detector_kwargs = dict(return_features=True)      # raw pool features, before the softmax
    real_features = metric_utils.compute_feature_stats_for_dataset(
        opts=opts, detector_url=DETECTOR_URL, detector_kwargs=detector_kwargs, mode_dict=opts.mode_dict,
        rel_lo=0, rel_hi=0, capture_all=True, max_items=max_real).get_all_torch()
    gen_features = metric_utils.compute_feature_stats_for_generator(
        opts=opts, detector_url=DETECTOR_URL, detector_kwargs=detector_kwargs, mode_dict=opts.mode_dict,
        rel_lo=0, rel_hi=1, capture_all=True, max_items=num_gen).get_all_torch()
    if opts.rank != 0:
        return float('nan')
    return kid_from_features(real_features.to(opts.device), gen_features.to(opts.device), num_subsets,
                             max_subset_size)
