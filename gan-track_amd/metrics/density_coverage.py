"""Precision, recall, density and coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative
Models", ICML 2020), per modality.

Improved precision asks whether a generated feature lies in any real k-NN ball, so one outlying real slice with a huge
ball "contains" many fakes; improved recall is measured against a manifold built from the fakes and is over-estimated.
Density and coverage are built on the real balls only:

    count[i]   = #{ j : dist(gen_i, real_j) <= r_j }         r_j = the k-th neighbour distance of real_j (knn_radii)
    covered[j] = any_i dist(gen_i, real_j) <= r_j
    density    = sum(count) / (k p)        coverage = sum(covered) / n        precision = #{count > 0} / p

and recall is the membership pass with the roles swapped, at the same k.  The comparison is `<=` on the balls of
precision_recall.py (the `prdc` package uses `<`; the two differ on exact ties only), so precision here is pr50k's
precision at the same k, bit for bit, and density is read off the same balls.  All of them come from one pass over
the gen x real distance tiles (torch_utils/ops/manifold.py manifold_count); the features are captured as in
precision_recall.py (VGG16, all of them, fp16 on the device).

SG2_PRDC_FUSED=0 (or fused=False) runs the composition instead, on any device: float32 torch.cdist in row blocks,
rounded to fp16, then `<=`, sum(1), any(0), with radii from kthvalue(k + 1) of the same distances -- an A/B path."""
import os

import torch

from torch_utils.ops import manifold
from . import metric_utils
from .precision_recall import DETECTOR_URL

ROW_BLOCK = 4096        # rows of the composition's distance blocks


def _dist16(rows, cols):
    """fp16-rounded distances [rows, cols] of fp16 features, computed in float32."""
    return torch.cdist(rows.to(torch.float32), cols.to(torch.float32)).to(torch.float16)


def composed_radii(x, k):
    """knn_radii by composition: kthvalue(k + 1) of the fp16 distances of x against itself, the diagonal exactly 0."""
    out = []
    for lo in range(0, x.shape[0], ROW_BLOCK):
        d = _dist16(x[lo:lo + ROW_BLOCK], x)
        idx = torch.arange(d.shape[0], device=d.device)
        d[idx, lo + idx] = 0
        out.append(d.to(torch.float32).kthvalue(k + 1, dim=1).values)
    return torch.cat(out)


def composed_count(probes, mani, radii):
    """manifold_count by composition: (count int32 [p], covered bool [n])."""
    r16 = radii.to(torch.float16).to(torch.float32)[None, :]
    count = []
    covered = torch.zeros([mani.shape[0]], dtype=torch.bool, device=mani.device)
    for lo in range(0, probes.shape[0], ROW_BLOCK):
        inside = _dist16(probes[lo:lo + ROW_BLOCK], mani).to(torch.float32) <= r16
        count.append(inside.sum(dim=1, dtype=torch.int32))
        covered |= inside.any(dim=0)
    return torch.cat(count), covered


def fused_default():
    return os.environ.get('SG2_PRDC_FUSED', '1') != '0'


def prdc_from_features(real, gen, nhood_size, fused=None):
    """dict(precision, recall, density, coverage) of two fp16 feature sets [n, d] and [p, d] on one device; fused
    (default: SG2_PRDC_FUSED != 0) needs a ROCm device, the composition runs anywhere."""
    k = int(nhood_size)
    if fused is None:
        fused = fused_default()
    real, gen = real.to(torch.float16), gen.to(torch.float16)
    if fused:
        count, covered = manifold.manifold_count(gen, real, manifold.knn_radii(real, k))
        recalled = manifold.manifold_member(real, gen, manifold.knn_radii(gen, k))
    else:
        count, covered = composed_count(gen, real, composed_radii(real, k))
        recalled = composed_count(real, gen, composed_radii(gen, k))[0] > 0
    n, p = real.shape[0], gen.shape[0]
    return dict(precision=int((count > 0).sum()) / p,
                recall=int(recalled.sum()) / n,
                density=int(count.sum(dtype=torch.int64)) / (k * p),
                coverage=int(covered.sum()) / n)


def compute_prdc(opts, max_real, num_gen, nhood_size, fused=None):
    """The feature passes of precision_recall.compute_pr, then prdc_from_features.  At num_gpus > 1 every rank holds
    the global feature set after FeatureStats.reduce() and computes the same, deterministic result."""
    detector_kwargs = dict(return_features=True)
    real_features = metric_utils.compute_feature_stats_for_dataset(
        opts=opts, detector_url=DETECTOR_URL, detector_kwargs=detector_kwargs, mode_dict=opts.mode_dict,
        rel_lo=0, rel_hi=0, capture_all=True, max_items=max_real).get_all_torch().to(opts.device).to(torch.float16)
    gen_features = metric_utils.compute_feature_stats_for_generator(
        opts=opts, detector_url=DETECTOR_URL, detector_kwargs=detector_kwargs, mode_dict=opts.mode_dict,
        rel_lo=0, rel_hi=1, capture_all=True, max_items=num_gen).get_all_torch().to(opts.device).to(torch.float16)
    return prdc_from_features(real_features, gen_features, nhood_size, fused=fused)
