"""Image generation on the GPU: genlib.generate.synthesize_tiles against the plain composition, the float images
against the CPU oracle, and the three CLIs on a snapshot written by this build's saver.

The generator is the tiny one of test_projector_gpu.test_cli_smoke: 16^2, two channels, z_dim = w_dim = 16, two
mapping layers, noise_strength 0.1 (so the noise modes differ), and a non-zero w_avg (so truncation does something).
synthesize_tiles is compared with G.synthesis on the SAME chunks followed by image_tiles_u8_ref, so the test does not
depend on whether the generator is bitwise batch-invariant (nobody has established that).  The float images are held
to the project's f32 parity floor, 1e-4 relative L2 (parity_train / test_projector_gpu)."""
import os

import numpy as np
import pytest
import torch

import projector_oracle as po

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MODS = po.MODALITIES
KW = dict(c_dim=0, img_resolution=16, img_channels=2, channel_base=64, channel_max=8)
SEEDS = [0, 1, 2, 3, 7]


def _tiny(mod):
    return mod.Generator(z_dim=16, w_dim=16, num_fp16_res=0, mapping_kwargs=dict(num_layers=2), **KW)


@pytest.fixture(scope='module')
def G_cpu():
    from training import networks_stylegan2 as net
    torch.manual_seed(3)
    G = _tiny(net).eval().requires_grad_(False)
    with torch.no_grad():
        for n, p in G.named_parameters():
            if n.endswith('noise_strength'):
                p.fill_(0.1)
        G.mapping.w_avg.copy_(torch.randn([16], generator=torch.Generator().manual_seed(4)) * 0.5)
    return G


@pytest.fixture(scope='module')
def G(G_cpu):
    import copy
    return copy.deepcopy(G_cpu).to(DEV)


@pytest.fixture(scope='module')
def snapshot(G_cpu, tmp_path_factory):
    import legacy
    from training import networks_stylegan2 as net
    path = str(tmp_path_factory.mktemp('snap') / 'network-snapshot-000004.pkl')
    D = net.Discriminator(num_fp16_res=0, **KW)
    legacy.save_network_pkl(path, G_cpu, D, G_cpu, None, dict(path='data.zip', modalities=MODS))
    return path


def _png(path):
    import PIL.Image
    img = PIL.Image.open(path)
    return img.mode, np.array(img)


def _library_tiles(G, seeds, psi=1.0, cutoff=None, noise_mode='const', force_fp32=False):
    """[len(seeds) * 16, 2 * 16] uint8: row s holds the two channels of seed s, each seed mapped and rendered alone."""
    from genlib import generate
    canvas = generate.new_canvas(G, (2, len(seeds)))
    for i, s in enumerate(seeds):
        ws = generate.map_seeds(G, [s], None, psi, cutoff)
        generate.synthesize_tiles(G, ws, canvas, first_tile=2 * i, noise_mode=noise_mode, force_fp32=force_fp32,
                                  tiles='grey', grid=(2, len(seeds)))
    return canvas.cpu().numpy()[:, :, 0]


# ---- the library ----

@pytest.mark.parametrize('batch', [1, 3])
def test_synthesize_tiles_against_the_composition(G, batch, monkeypatch):
    from genlib import generate
    from torch_utils.ops import image_tiles
    ws = generate.map_seeds(G, SEEDS, None, 0.7, 4)
    assert ws.shape == (5, G.num_ws, 16)
    grid = (4, 3)
    want = torch.full([3 * 16, 4 * 16, 1], 0xA5, dtype=torch.uint8, device=DEV)
    first = 1
    with torch.no_grad():
        for i in range(0, 5, batch):
            img = G.synthesis(ws[i:i + batch], noise_mode='const', force_fp32=False)
            image_tiles.image_tiles_u8_ref(img, out=want, tiles='grey', grid=grid, first_tile=first)
            first += 2 * img.shape[0]
    results = {}
    for env in ('1', '0'):
        monkeypatch.setenv('SG2_GEN_FUSED', env)
        assert generate.fused() == (env == '1')
        got = torch.full_like(want, 0xA5)
        keep = []
        nxt = generate.synthesize_tiles(G, ws, got, first_tile=1, noise_mode='const', batch=batch, tiles='grey', grid=grid,
                                        keep=keep)
        assert nxt == 11 and len(keep) == -(-5 // batch) and sum(k.shape[0] for k in keep) == 5
        assert torch.equal(got, want), f'SG2_GEN_FUSED={env}, batch {batch}: {int((got != want).sum())} bytes differ'
        results[env] = got
    assert torch.equal(results['0'], results['1'])
    host = want.cpu().numpy()
    assert (host[:16, :16] == 0xA5).all() and (host[32:, 48:] == 0xA5).all()      # cell 0 and cell 11: not addressed
    assert len(np.unique(host[:16, 16:32])) > 8


def test_synthesize_tiles_per_channel_canvases(G):
    from genlib import generate
    ws = generate.map_seeds(G, SEEDS[:3], None, 1.0, None)
    grey = generate.new_canvas(G, (2, 3))
    generate.synthesize_tiles(G, ws, grey, tiles='grey', grid=(2, 3))
    per = [generate.new_canvas(G, (3, 1)) for _ in range(2)]
    generate.synthesize_tiles(G, ws, per, tiles='channels', grid=(3, 1))
    for n in range(3):
        for k in range(2):
            assert torch.equal(generate.cell(per[k], n, (3, 1), 16), generate.cell(grey, 2 * n + k, (2, 3), 16))
    with pytest.raises(ValueError):
        generate.synthesize_tiles(G, ws, per, tiles='grey')


def test_float_images_against_the_oracle(G, G_cpu):
    from genlib import generate
    from oracle import sg2_oracle as O
    ref = _tiny(O).eval().requires_grad_(False)
    ref.load_state_dict(G_cpu.state_dict())
    z = generate.seeds_to_z(SEEDS, 16)
    with torch.no_grad():
        want = ref(z, None, truncation_psi=0.7, truncation_cutoff=4, noise_mode='const').double().numpy()
    ws = generate.map_seeds(G, SEEDS, None, 0.7, 4)
    keep = []
    generate.synthesize_tiles(G, ws, generate.new_canvas(G, (2, 5)), noise_mode='const', batch=2, tiles='grey',
                              grid=(2, 5), keep=keep)
    got = torch.cat(keep).double().cpu().numpy()
    assert got.shape == want.shape == (5, 2, 16, 16)
    err = po.rel(got, want)
    print(f'float images vs oracle (psi 0.7, cutoff 4, const): rel L2 {err:.3g} (bound {po.FLOOR:.3g})')
    assert np.isfinite(got).all() and err <= po.FLOOR


# ---- the CLIs ----

def test_gen_images_cli(G, snapshot, tmp_path):
    import gen_images_mi_multimodal as cli
    from click.testing import CliRunner
    out = tmp_path / 'const'
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0-3', '--trunc', '0.7', '--trunc-cutoff', '4',
                                        '--outdir', str(out), '--raw'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    want = _library_tiles(G, [3], psi=0.7, cutoff=4)
    imgs = {}
    for k, m in enumerate(MODS):
        for s in range(4):
            mode, imgs[m, s] = _png(out / m / f'seed{s:04d}.png')
            assert mode == 'L' and imgs[m, s].shape == (16, 16) and imgs[m, s].dtype == np.uint8
        assert np.array_equal(imgs[m, 3], want[:, 16 * k:16 * (k + 1)]), m
        assert not np.array_equal(imgs[m, 0], imgs[m, 1])
    raw = np.load(out / 'seed0003.npy')
    assert raw.shape == (2, 16, 16) and raw.dtype == np.float32
    assert not os.path.exists(out / 'grid.png')
    # --noise-mode none differs from const; --batch and --grid give the same per-seed files plus grid.png
    none = tmp_path / 'none'
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '3', '--trunc', '0.7', '--trunc-cutoff', '4',
                                        '--noise-mode', 'none', '--outdir', str(none)], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    for m in MODS:
        assert not np.array_equal(_png(none / m / 'seed0003.png')[1], imgs[m, 3])
    # --trunc 0: every seed is the image of w_avg
    t0 = tmp_path / 'trunc0'
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0,5,9', '--trunc', '0', '--outdir', str(t0),
                                        '--grid', '3x2', '--modalities', 'a,b'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    for m in ('a', 'b'):
        first = _png(t0 / m / 'seed0000.png')[1]
        assert len(np.unique(first)) > 8
        for s in (5, 9):
            assert np.array_equal(_png(t0 / m / f'seed{s:04d}.png')[1], first)
    mode, grid = _png(t0 / 'grid.png')
    assert mode == 'L' and grid.shape == (2 * 16, 3 * 16)
    assert np.array_equal(grid[:16, :16], _png(t0 / 'a' / 'seed0000.png')[1])
    assert np.array_equal(grid[:16, 16:32], _png(t0 / 'b' / 'seed0000.png')[1])
    assert np.array_equal(grid[16:, 32:], _png(t0 / 'b' / 'seed0009.png')[1])
    # too small a grid and a wrong modality count are usage errors
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0-3', '--outdir', str(t0), '--grid', '2x2'])
    assert res.exit_code != 0 and '--grid' in res.output
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0', '--outdir', str(t0), '--modalities', 'a'])
    assert res.exit_code != 0 and 'modalities' in res.output


def test_style_mixing_cli(G, snapshot, tmp_path):
    import gen_images_style_mixing as cli
    from click.testing import CliRunner
    from genlib import generate
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--rows', '1,2', '--cols', '3,4,5', '--styles', '2-3',
                                        '--trunc', '0.7', '--outdir', str(tmp_path)], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    rows, cols = [1, 2], [3, 4, 5]
    # the sources: w truncated as w_avg + (w - w_avg) * psi over the mapping of all seeds at once, force_fp32
    seeds = sorted(rows + cols)
    with torch.no_grad():
        w_all = generate.truncate(G.mapping(generate.seeds_to_z(seeds, 16).to(DEV), None), G.mapping.w_avg, 0.7)
    src = generate.new_canvas(G, (2, 5))
    generate.synthesize_tiles(G, w_all, src, force_fp32=True, tiles='grey', grid=(2, 5))
    src = src.cpu().numpy()[:, :, 0]
    for k, m in enumerate(MODS):
        mode, grid = _png(tmp_path / m / 'grid.png')
        assert mode == 'L' and grid.shape == ((2 + 1) * 16, (3 + 1) * 16)
        assert (grid[:16, :16] == 0).all()
        for r, row in enumerate(rows):
            for c, col in enumerate(cols):
                mode, img = _png(tmp_path / m / f'{row}-{col}.png')
                assert mode == 'L' and np.array_equal(img, grid[16 * (r + 1):16 * (r + 2), 16 * (c + 1):16 * (c + 2)])
                assert not np.array_equal(img, _png(tmp_path / m / f'{row}-{row}.png')[1])
        for i, s in enumerate(seeds):
            want = src[16 * i:16 * (i + 1), 16 * k:16 * (k + 1)]
            assert np.array_equal(_png(tmp_path / m / f'{s}-{s}.png')[1], want), (m, s)
        for c, col in enumerate(cols):
            assert np.array_equal(grid[:16, 16 * (c + 1):16 * (c + 2)], _png(tmp_path / m / f'{col}-{col}.png')[1])
        for r, row in enumerate(rows):
            assert np.array_equal(grid[16 * (r + 1):16 * (r + 2), :16], _png(tmp_path / m / f'{row}-{row}.png')[1])
    # a mix is the row's image with the column's styles 2-3
    mix = generate.mix_styles(w_all[seeds.index(2)], w_all[seeds.index(4)], [2, 3]).unsqueeze(0)
    cv = generate.new_canvas(G, (2, 1))
    generate.synthesize_tiles(G, mix, cv, tiles='grey', grid=(2, 1))
    assert np.array_equal(cv.cpu().numpy()[:, :16, 0], _png(tmp_path / MODS[0] / '2-4.png')[1])
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--rows', '1', '--cols', '3', '--outdir', str(tmp_path)])
    assert res.exit_code != 0 and '--styles' in res.output        # the default 10-13 is past this generator's 6 layers


def test_gen_video_cli(G, snapshot, tmp_path):
    import gen_video as cli
    from click.testing import CliRunner
    out = tmp_path / 'frames'
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0,1', '--w-frames', '2', '--modality', MODS[1],
                                        '--output', str(out)], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert sorted(os.listdir(out)) == [f'frame_{i:05d}.png' for i in range(4)]
    frames = [_png(out / f'frame_{i:05d}.png') for i in range(4)]
    assert all(mode == 'L' and f.shape == (16, 16) for mode, f in frames)
    want = _library_tiles(G, [0, 1])
    assert np.array_equal(frames[0][1], want[:16, 16:]), 'frame 0 is the image of seed 0'
    assert np.array_equal(frames[2][1], want[16:, 16:]), 'frame w_frames is the image of seed 1'
    assert not np.array_equal(frames[1][1], frames[0][1]) and not np.array_equal(frames[1][1], frames[2][1])
    # a 2 x 1 grid: two cells, one keyframe each -- every frame is the two seeds side by side
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0,1', '--grid', '2x1', '--w-frames', '1',
                                        '--output', str(tmp_path / 'grid')], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    mode, f = _png(tmp_path / 'grid' / 'frame_00000.png')
    assert f.shape == (16, 32) and np.array_equal(f[:, :16], want[:16, :16]) and np.array_equal(f[:, 16:], want[16:, :16])
    res = CliRunner().invoke(cli.main, ['--network', snapshot, '--seeds', '0,1,2', '--grid', '2x1', '--output', str(out)])
    assert res.exit_code != 0 and 'divisible' in res.output
