"""Score the projections of a run against their targets: MSE, PSNR, SSIM and, when asked, the squared LPIPS-feature
distance, per (patient, slice, modality).  The reference has no counterpart: its projector logs only its own loss.

A projection run directory (genlib/run_projector_mi_multimodal.py) holds training_options.json and `projected_w`, the
pickle {patient: {slice: w [num_ws, w_dim]}}.  score_run walks the dataset in file order with the projection loop's id
parsing, keeps the items whose (patient, slice) was projected, renders `batch` of them at a time with the generator the
projector loaded

    (G.synthesis(ws, noise_mode='const', force_fp32=True) + 1) * (255 / 2), clamped to [0, 255]

and makes one torch_utils.ops.ssim.ssim_mse call per batch against the float32 targets.  The images are rendered with
the generator's OWN noise buffers, as the projector's side-by-side PNG is: the noise the projector optimised along with
w is not stored, so the scores are those of the stored w, not of the optimiser's final image.

Written: <run>/reconstruction.csv (a row per patient, slice and modality, in dataset order), <run>/reconstruction.json
(per modality: count, mean / std / min / max of ssim and mse, the mean of the finite psnr values and the count of
infinite ones) and, with maps, <run>/<patient>/<modality>/ssim_map/map_<slice>.png.
"""
import csv
import json
import math
import os
import pickle

import numpy as np
import torch
import torch.nn.functional as F

import dnnlib
import legacy
from genlib.utils import util_general
from training.dataset_mi_multimodal import SafeUnpickler
from torch_utils.ops import ssim as ssim_op

CSV_NAME, JSON_NAME = 'reconstruction.csv', 'reconstruction.json'


def _device():
    return torch.device('cuda', 0)


class ProjectedWUnpickler(SafeUnpickler):
    """Admits what util_general.plain_dict writes (builtin containers, numpy arrays) and the reference's own file: a
    collections.defaultdict whose factory is its util_general.nested_dict, which is mapped to dict.  Every other global
    is refused by name."""

    def find_class(self, module, name):
        if (module, name) == ('collections', 'defaultdict'):
            import collections
            return collections.defaultdict
        if name == 'nested_dict' and module.split('.')[-1] == 'util_general':
            return dict
        try:
            return super().find_class(module, name)
        except pickle.UnpicklingError:
            raise pickle.UnpicklingError(f'projected_w refers to {module}.{name}: not a plain dict of arrays; '
                                         f'refused') from None


def load_projected_w(path):
    """{patient: {slice: float32 [num_ws, w_dim]}} as plain dicts, keys as stored."""
    with open(path, 'rb') as f:
        data = ProjectedWUnpickler(f).load()
    data = util_general.plain_dict(data)
    if not isinstance(data, dict) or not all(isinstance(v, dict) for v in data.values()):
        raise RuntimeError(f'{path}: expected {{patient: {{slice: w}}}}; got {type(data).__name__}')
    for patient, slices in data.items():
        for sl, w in slices.items():
            if not isinstance(w, np.ndarray) or w.ndim != 2:
                raise RuntimeError(f'{path}: w of ({patient}, {sl}) must be an array [num_ws, w_dim]; got '
                                   f'{type(w).__name__} {getattr(w, "shape", "")}')
    return data


def _item_ids(fname):
    """(patient, slice) of a dataset file name: the projection loop's own parsing."""
    _, id_patient, id_slice = util_general.split_dos_path_into_components(path=fname)
    return id_patient, util_general.get_filename_without_extension(path=id_slice)[-5:]


def select_items(dataset, projected_w):
    """[(dataset index, patient, slice)] in file order for the items `projected_w` holds (the file names come from the
    dataset's table, so no image is read for an item that was not projected); a key of projected_w with no dataset
    item is an error naming it."""
    wanted = {(p, s) for p, slices in projected_w.items() for s in slices}
    items, found = [], set()
    for idx in range(len(dataset)):
        key = _item_ids(dataset._image_fnames[int(dataset._raw_idx[idx])])
        if key in wanted and key not in found:
            items.append((idx,) + key)
            found.add(key)
    missing = sorted(wanted - found)
    if missing:
        raise RuntimeError(f'projected_w holds {len(missing)} (patient, slice) key(s) with no item in the dataset: '
                           f'{missing[:8]}{" ..." if len(missing) > 8 else ""}')
    return items


def render(G, ws):
    """float32 [B, C, H, W] in [0, 255] from ws [B, num_ws, w_dim], with the generator's own noise."""
    with torch.no_grad():
        img = (G.synthesis(ws, noise_mode='const', force_fp32=True) + 1) * (255 / 2)
    return img.to(torch.float32).clamp(0, 255)


def lpips_distances(detector, synth, target, modalities):
    """float32 [B, M]: the squared LPIPS-feature distance of every rendered slice to its target, per modality -- the
    projector's split, 256^2 area resize and feature call, then torch_utils.ops.ppl.pair_distances at eps = 1."""
    from genlib.projector.projector import lpips_features, split_modalities
    from torch_utils.ops import ppl
    s_mod, t_mod = split_modalities(synth, modalities), split_modalities(target, modalities)
    cols = []
    for m in list(s_mod):
        feats = []
        for img in (t_mod[m], s_mod[m]):
            img = img.clone()       # (the network normalises its input in place)
            if img.shape[2] > 256:
                img = F.interpolate(img, size=(256, 256), mode='area')
            feats.append(lpips_features(detector, img).to(torch.float32))
        cols.append(ppl.pair_distances(torch.cat(feats), eps=1.0))
    return torch.stack(cols, dim=1)


def summarise(rows, modalities, with_lpips):
    out = {}
    for m in modalities:
        sel = [r for r in rows if r['modality'] == m]
        entry = {'count': len(sel)}
        for key in ('ssim', 'mse') + (('lpips',) if with_lpips else ()):
            v = np.array([r[key] for r in sel], dtype=np.float64)
            entry[key] = {k: (float(getattr(v, k)()) if len(v) else None) for k in ('mean', 'std', 'min', 'max')}
        finite = [r['psnr'] for r in sel if math.isfinite(r['psnr'])]
        entry['psnr'] = {'mean_finite': float(np.mean(finite)) if finite else None,
                         'count_infinite': len(sel) - len(finite)}
        out[m] = entry
    return out


def format_table(summary):
    lines = [f'{"modality":<24s}{"count":>7s}{"ssim":>10s}{"+-":>9s}{"mse":>12s}{"psnr":>9s}{"inf":>5s}']
    for m, e in summary.items():
        if not e['count']:
            lines.append(f'{m:<24s}{0:>7d}')
            continue
        ps = e['psnr']['mean_finite']
        lines.append(f'{m:<24s}{e["count"]:>7d}{e["ssim"]["mean"]:>10.4f}{e["ssim"]["std"]:>9.4f}'
                     f'{e["mse"]["mean"]:>12.3f}{(f"{ps:.2f}" if ps is not None else "-"):>9s}'
                     f'{e["psnr"]["count_infinite"]:>5d}')
    return '\n'.join(lines)


def _write_map(run_dir, patient, modality, sl, smap):
    import PIL.Image
    out = os.path.join(run_dir, patient, modality, 'ssim_map')
    os.makedirs(out, exist_ok=True)
    grey = (smap.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
    PIL.Image.fromarray(grey).save(os.path.join(out, f'map_{sl}.png'))


def score_run(run_dir, data=None, network=None, batch=16, data_range=255.0, lpips=False, maps=False, G=None):
    """Score the run in `run_dir` (module docstring).  data / network override the dataset path and the snapshot file
    that training_options.json names; G: an already loaded generator in place of the snapshot.  Returns
    (rows, summary): the CSV's rows as dicts and the JSON's content."""
    with open(os.path.join(run_dir, 'training_options.json')) as f:
        opts = json.load(f)
    ts_kwargs = dnnlib.EasyDict(opts['training_set_kwargs'])
    if data is not None:
        ts_kwargs.path = data
    modalities = list(ts_kwargs.modalities)
    projected_w = load_projected_w(os.path.join(run_dir, 'projected_w'))
    device = _device()

    dataset = dnnlib.util.construct_class_by_name(**ts_kwargs)
    items = select_items(dataset, projected_w)
    detector = None
    if lpips:
        from genlib.projector.projector import LPIPS_URL
        from metrics import metric_utils
        detector = metric_utils.get_feature_detector(LPIPS_URL, device=device)
    if G is None:
        snapshot = network or opts.get('projector_kwargs', {}).get('outdir_model')
        if snapshot is None or not os.path.isfile(snapshot):
            raise RuntimeError(f'the snapshot {snapshot!r} of {run_dir} is not a file: name it with --network')
        print(f'Loading networks from "{snapshot}"...')
        with open(snapshot, 'rb') as f:
            G = legacy.load_network_pkl(f)['G_ema']
    G = G.eval().requires_grad_(False).to(device)
    channels = dataset.image_shape[0]
    if len(modalities) != channels:
        raise RuntimeError(f'the dataset holds {channels} image channel(s) for the modalities {modalities}: the scores '
                           f'are per modality, one channel each')
    if lpips and channels == 3:
        raise RuntimeError('--lpips: the projector reads three channels as one RGB image, not as three modalities')

    rows = []
    for start in range(0, len(items), int(batch)):
        chunk = items[start:start + int(batch)]
        target = torch.from_numpy(np.stack([dataset[idx][0] for idx, _, _ in chunk])).to(device).to(torch.float32)
        ws = torch.from_numpy(np.stack([np.asarray(projected_w[p][s], dtype=np.float32) for _, p, s in chunk])).to(device)
        synth = render(G, ws)
        if synth.shape != target.shape:
            raise RuntimeError(f'the generator renders {list(synth.shape[1:])}, the dataset holds {list(target.shape[1:])}')
        res = ssim_op.ssim_mse(synth.contiguous(), target.contiguous(), data_range=data_range, want_map=maps)
        out, smap = res if maps else (res, None)
        out = out.cpu().numpy()
        dist = lpips_distances(detector, synth, target, modalities).cpu().numpy() if lpips else None
        for b, (_, patient, sl) in enumerate(chunk):
            for c, m in enumerate(modalities):
                mse = float(out[b, c, 1])
                row = {'patient': patient, 'slice': sl, 'modality': m, 'mse': mse,
                       'psnr': ssim_op.psnr(mse, data_range), 'ssim': float(out[b, c, 0])}
                if lpips:
                    row['lpips'] = float(dist[b, c])
                rows.append(row)
                if maps:
                    _write_map(run_dir, patient, m, sl, smap[b, c])

    summary = summarise(rows, modalities, lpips)
    fields = ['patient', 'slice', 'modality', 'mse', 'psnr', 'ssim'] + (['lpips'] if lpips else [])
    with open(os.path.join(run_dir, CSV_NAME), 'wt', newline='') as f:
        w = csv.DictWriter(f, fieldnames=fields)
        w.writeheader()
        for row in rows:
            w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in row.items()})
    with open(os.path.join(run_dir, JSON_NAME), 'wt') as f:
        json.dump({'data_range': float(data_range), 'slices': len(items), 'modalities': summary}, f, indent=2)
    print(format_table(summary))
    return rows, summary

