"""Shared infrastructure of the perceptual-path-length tests (no dependency on the reference or on a GPU).

  * the cases of the fixture tests/golden/ppl_ref.npz (made by tests/golden/make_ppl_golden.py from the reference's own
    PPLSampler and compute_ppl on the projector fixture's tiny two-modality generator and projector_oracle.StandIn);
  * sample(): a pure-torch restatement of ONE sampler call (SG3/metrics/perceptual_path_length.py:48-90, with the
    per-modality channel selection) on any generator implementation -- the tests run it on the CPU oracle
    (oracle/sg2_oracle.py) with the fixture's tape replayed, or on given draws;
  * the fixture loader, and the bounds: max(FLOOR, FACTOR x the reference's own spread), the spread being the largest
    per-sample relative distance of a re-evaluation of the reference (one thread; every parameter nudged by 1 +- 2^-24,
    two sign seeds) from the reference run.
"""
import numpy as np
import torch

import projector_oracle as po

BATCH = 2
# name -> the sampler's arguments, the modality (channel) evaluated and the number of samples
CASES = {
    'wend_e4_m0': dict(space='w', sampling='end', epsilon=1e-4, crop=False, mode_idx=0, num_samples=128),
    'wend_e4_m1': dict(space='w', sampling='end', epsilon=1e-4, crop=False, mode_idx=1, num_samples=128),
    'wend_e2': dict(space='w', sampling='end', epsilon=1e-2, crop=False, mode_idx=0, num_samples=16),
    'wend_e2_crop': dict(space='w', sampling='end', epsilon=1e-2, crop=True, mode_idx=1, num_samples=16),
    'wfull_e4': dict(space='w', sampling='full', epsilon=1e-4, crop=False, mode_idx=1, num_samples=16),
    'zfull_e4': dict(space='z', sampling='full', epsilon=1e-4, crop=False, mode_idx=0, num_samples=16),
}
SPREADS = ('t1', 'n24s1', 'n24s2')
MAX_BOUND = 0.25            # a per-sample bound above this judges nothing
MAX_BOUND_E2 = 1e-2         # ... and the epsilon = 1e-2 cases are the ones that catch arithmetic errors


def slerp(a, b, t):
    """Unit vectors a', b' -> the point at angle t * angle(a', b') from a' on their great circle, renormalised."""
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)  # noqa: E731
    a, b = unit(a), unit(b)
    cos_ab = (a * b).sum(dim=-1, keepdim=True)
    angle = t * torch.acos(cos_ab)
    ortho = unit(b - cos_ab * a)
    return unit(a * torch.cos(angle) + ortho * torch.sin(angle))


def noise_buffers(G):
    return [buf for name, buf in G.named_buffers() if name.endswith('.noise_const')]


@torch.no_grad()
def sample(G, detector, c, epsilon, space, sampling, crop, mode_idx=None, draws=None):
    """dist [B] of one sampler call.  G's noise_const buffers are overwritten.  Draws: torch.rand, torch.randn, then
    torch.randn_like per buffer (replay a tape around the call), or draws = (t, z, [noise])."""
    batch = c.shape[0]
    bufs = noise_buffers(G)
    if draws is None:
        t = torch.rand([batch], device=c.device)
        z = torch.randn([batch * 2, G.z_dim], device=c.device)
        noise = [torch.randn_like(b) for b in bufs]
    else:
        t, z, noise = draws
    t = t * (1 if sampling == 'full' else 0)
    z0, z1 = z.chunk(2)
    if space == 'w':
        w0, w1 = G.mapping(z=torch.cat([z0, z1]), c=torch.cat([c, c])).chunk(2)
        wt0 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2))
        wt1 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2) + epsilon)
    else:
        zt0 = slerp(z0, z1, t.unsqueeze(1))
        zt1 = slerp(z0, z1, t.unsqueeze(1) + epsilon)
        wt0, wt1 = G.mapping(z=torch.cat([zt0, zt1]), c=torch.cat([c, c])).chunk(2)
    for b, n in zip(bufs, noise):
        b.copy_(n)
    img = G.synthesis(ws=torch.cat([wt0, wt1]), noise_mode='const', force_fp32=True)
    if mode_idx is not None:
        img = img[:, mode_idx:mode_idx + 1]
    if crop:
        q = img.shape[2] // 8
        img = img[:, :, q * 3:q * 7, q * 2:q * 6]
    factor = G.img_resolution // 256
    if factor > 1:
        n, ch, h, w = img.shape
        img = img.reshape(n, ch, h // factor, factor, w // factor, factor).mean([3, 5])
    img = (img + 1) * (255 / 2)
    if img.shape[1] == 1:
        img = img.repeat([1, 3, 1, 1])
    f0, f1 = detector(img, resize_images=False, return_lpips=True).chunk(2)
    return (f0 - f1).square().sum(1) / epsilon ** 2


def run_case(G, detector, case, tape=None):
    """Every sampler call of a fixture case on G -> dist [num_samples] (float64 numpy)."""
    kw = dict(CASES[case])
    n, mode_idx = kw.pop('num_samples'), kw.pop('mode_idx')
    c = torch.zeros([BATCH, G.c_dim])
    out = []
    ctx = tape.replay() if tape is not None else None
    if ctx is not None:
        ctx.__enter__()
    try:
        for _ in range(0, n, BATCH):
            out.append(sample(G, detector, c, mode_idx=mode_idx, **kw))
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return torch.cat(out)[:n].double().numpy()


def tape_draws(tape, G, calls):
    """The (t, z, [noise]) tuples of `calls` sampler calls, read from a fixture tape (CPU tensors)."""
    nbuf = len(noise_buffers(G))
    vals = [torch.from_numpy(np.array(v)) for _, v in tape.entries]
    assert len(vals) == calls * (2 + nbuf), (len(vals), calls, nbuf)
    per = 2 + nbuf
    return [(vals[i * per], vals[i * per + 1], vals[i * per + 2:(i + 1) * per]) for i in range(calls)]


def ppl_from_distances(dist):
    """numpy restatement of the percentile cut (the tests' own; the product's is metrics.perceptual_path_length's)."""
    dist = np.asarray(dist)
    s = np.sort(dist)
    lo = s[int(np.floor(0.01 * (len(s) - 1)))]
    hi = s[int(np.ceil(0.99 * (len(s) - 1)))]
    return float(dist[(dist >= lo) & (dist <= hi)].mean())


# ---- the fixture ----

def load_fixture(path):
    from rngtape import Tape
    with np.load(path, allow_pickle=False) as z:
        z = {k: z[k] for k in z.files}
    fix = {'det': {k[4:]: v for k, v in z.items() if k.startswith('det/')}, 'cases': {}}
    for case in CASES:
        pre = case + '/'
        fix['cases'][case] = dict(
            dist=z[pre + 'dist'], ppl=float(z[pre + 'ppl']),
            tape=Tape.from_npz({k[len(pre):]: v for k, v in z.items() if k.startswith(pre + 'tape')}, 'tape'),
            spread={s: dict(dist=z[f'{pre}r32_{s}/dist'], ppl=float(z[f'{pre}r32_{s}/ppl'])) for s in SPREADS})
    return fix


def rel_each(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.abs(want)


def bounds(ref_case):
    """((per-sample bound, spread), (ppl bound, spread)) of a fixture case."""
    d = max(float(rel_each(s['dist'], ref_case['dist']).max()) for s in ref_case['spread'].values())
    p = max(abs(s['ppl'] - ref_case['ppl']) / abs(ref_case['ppl']) for s in ref_case['spread'].values())
    return (max(po.FLOOR, po.FACTOR * d), d), (max(po.FLOOR, po.FACTOR * p), p)


def judge(got, ref_case, what, with_ppl=False, got_ppl=None, check=True):
    """Every per-sample distance within the case's bound of the reference run (and the ppl within its own);
    prints each figure first."""
    (bd, sd), (bp, sp) = bounds(ref_case)
    e = rel_each(got, ref_case['dist'])
    print(f'{what}: per-sample rel error max {e.max():.3g} median {np.median(e):.3g} (bound {bd:.3g}, reference spread '
          f'{sd:.3g})')
    bad = [] if e.max() <= bd else [f'per-sample {e.max():.3g} > {bd:.3g}']
    if with_ppl:
        got_ppl = ppl_from_distances(got) if got_ppl is None else got_ppl
        ep = abs(got_ppl - ref_case['ppl']) / abs(ref_case['ppl'])
        print(f'{what}: ppl {got_ppl:.6g} against {ref_case["ppl"]:.6g}: rel {ep:.3g} (bound {bp:.3g}, reference spread '
              f'{sp:.3g})')
        if not ep <= bp:
            bad.append(f'ppl {ep:.3g} > {bp:.3g}')
    assert not check or not bad, f'{what}: ' + '; '.join(bad)
    return float(e.max()), bd
