"""Improved precision / recall (Kynkaanniemi et al. 2019), per modality (SG3/metrics/precision_recall.py:36-62).

precision = share of generated images whose VGG16 feature lies inside the real manifold (within the k-th neighbour
radius of some real feature), recall = the same with the roles swapped.  The features are captured as in the
reference (all of them, cast to fp16 on the device); the distance passes run on the fused k-NN kernels
(torch_utils/ops/manifold.py) instead of blocks of torch.cdist copied to the host, with the reference's fp16
rounding of the distances and radii kept (round16)."""
import torch

from torch_utils.ops import manifold
from . import metric_utils

DETECTOR_URL = 'https://api.ngc.nvidia.com/v2/models/nvidia/research/stylegan3/versions/1/files/metrics/vgg16.pkl'


def pr_from_features(real_features, gen_features, nhood_size):
    """(precision, recall) of two fp16 feature sets on one ROCm device."""
    results = {}
    for name, mani, probes in (('precision', real_features, gen_features), ('recall', gen_features, real_features)):
        radii = manifold.knn_radii(mani, nhood_size)
        results[name] = float(manifold.manifold_member(probes, mani, radii).to(torch.float32).mean())
    return results['precision'], results['recall']


def compute_pr(opts, max_real, num_gen, nhood_size, row_batch_size, col_batch_size):
    """The reference's signature and return value.  row_batch_size and col_batch_size are accepted and unused: they
    size the reference's distance-matrix blocks, and no distance matrix is formed here.  At num_gpus > 1 every rank
    holds the global feature set after FeatureStats.reduce() and computes the same, deterministic result."""
    detector_kwargs = dict(return_features=True)
    real_features = metric_utils.compute_feature_stats_for_dataset(
        opts=opts, detector_url=DETECTOR_URL, detector_kwargs=detector_kwargs, mode_dict=opts.mode_dict,
        rel_lo=0, rel_hi=0, capture_all=True, max_items=max_real).get_all_torch().to(opts.device).to(torch.float16)
    gen_features = metric_utils.compute_feature_stats_for_generator(
        opts=opts, detector_url=DETECTOR_URL, detector_kwargs=detector_kwargs, mode_dict=opts.mode_dict,
        rel_lo=0, rel_hi=1, capture_all=True, max_items=num_gen).get_all_torch().to(opts.device).to(torch.float16)
    return pr_from_features(real_features, gen_features, nhood_size)
