"""The image generation library's host side (no GPU): the command-line grammar, the latent helpers against the
reference's lines restated here, the keyframe interpolation, the torch composition image_tiles_u8_ref against a numpy
restatement of the reference's output stage (image_tiles_cases.np_tiles), the three CLIs' --help, and the new C entry
point's export and argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import image_tiles_cases as tc


@pytest.fixture(scope='module')
def generate():
    from genlib import generate
    return generate


# ---- grammar ----

def test_parse_range(generate):
    assert generate.parse_range('1,2,5-10') == [1, 2, 5, 6, 7, 8, 9, 10]
    assert generate.parse_range('7') == [7]
    assert generate.parse_range('3-3,0') == [3, 0]
    assert generate.parse_range('5-3') == []            # the reference's grammar: an empty range, not an error
    assert generate.parse_range([4, 2]) == [4, 2]
    for bad in ('', 'a', '1,,2', '1-', '1-2-3', '1.5', '2 - 4'):
        with pytest.raises(ValueError):
            generate.parse_range(bad)


def test_parse_tuple(generate):
    assert generate.parse_tuple('4x2') == (4, 2)
    assert generate.parse_tuple('0,1') == (0, 1)
    assert generate.parse_tuple((3, 5)) == (3, 5)
    for bad in ('', '4', '4x', 'x2', '4x2x1', '4 x 2', '-4x2', '4;2'):
        with pytest.raises(ValueError):
            generate.parse_tuple(bad)


# ---- latents ----

def test_seeds_to_z(generate):
    seeds = [0, 3, 1500, 3]
    z = generate.seeds_to_z(seeds, 16)
    assert z.shape == (4, 16) and z.dtype == torch.float64
    for row, s in zip(z, seeds):
        assert np.array_equal(row.numpy(), np.random.RandomState(s).randn(16))
    assert torch.equal(z[1], z[3])


def test_truncate_and_mix_styles(generate):
    g = torch.Generator().manual_seed(5)
    w_avg = torch.randn([8], generator=g)
    all_w = torch.randn([3, 6, 8], generator=g)
    for psi in (1, 0.7, 0.0):
        want = w_avg + (all_w - w_avg) * psi
        assert torch.equal(generate.truncate(all_w, w_avg, psi), want)
    assert torch.equal(generate.truncate(all_w, w_avg, 0)[2, 4], w_avg)
    styles = [2, 3, 5]
    row, col = all_w[0], all_w[1]
    row_before, col_before = row.clone(), col.clone()
    want = row.clone()
    want[styles] = col[styles]
    got = generate.mix_styles(row, col, styles)
    assert torch.equal(got, want)
    assert torch.equal(row, row_before) and torch.equal(col, col_before), 'the sources come through unchanged'
    assert got.data_ptr() != row.data_ptr()
    assert torch.equal(got[[0, 1, 4]], row[[0, 1, 4]]) and torch.equal(got[styles], col[styles])


def test_interp_ws(generate):
    K, w_frames, num_ws, w_dim = 3, 4, 2, 8
    key = torch.randn([K, num_ws, w_dim], generator=torch.Generator().manual_seed(9))
    frames = list(generate.interp_ws(key, w_frames))
    assert len(frames) == K * w_frames
    assert all(f.shape == (num_ws, w_dim) for f in frames)
    for k in range(K):
        assert np.abs(frames[k * w_frames].numpy() - key[k % K].numpy()).max() <= 1e-6
    # the period is K: the curve's frame K * w_frames is frame 0 again
    import scipy.interpolate
    x = np.arange(-K * 2, K * 3)
    curve = scipy.interpolate.interp1d(x, np.tile(key.numpy(), [5, 1, 1]), kind='cubic', axis=0)
    assert np.abs(curve(K) - frames[0].numpy()).max() <= 1e-6
    for i, f in enumerate(frames):
        assert np.array_equal(f.numpy(), curve(i / w_frames)), i
    # between keyframes the curve moves
    assert np.abs(frames[1].numpy() - frames[0].numpy()).max() > 1e-3


def test_keyframe_seeds():
    import gen_video
    s, k = gen_video.keyframe_seeds([5, 6, 7, 8], (2, 1))
    assert k == 2 and s.tolist() == [5, 6, 7, 8]
    s, k = gen_video.keyframe_seeds([5, 6], (2, 1), num_keyframes=3)
    assert k == 3 and s.tolist() == [5, 6, 5, 6, 5, 6]
    with pytest.raises(ValueError):
        gen_video.keyframe_seeds([1, 2, 3], (2, 1))
    s, _ = gen_video.keyframe_seeds(list(range(8)), (2, 2), shuffle_seed=1)
    want = np.arange(8)
    np.random.RandomState(seed=1).shuffle(want)
    assert s.tolist() == want.tolist()


# ---- image_tiles_u8_ref on CPU against numpy ----

def test_boundary_values_tell_one_rounding_from_two():
    x = tc.boundary_values()
    assert x.shape == (768,) and x.dtype == np.float32
    two = tc.np_to_u8(x, 'trunc')
    one = np.clip((x.astype(np.float64) * 127.5 + 128).astype(np.float32), 0, 255).astype(np.uint8)   # exact, then ONE rounding
    assert int((one != two).sum()) == 95


def _inputs(kind, shape, seed):
    if kind == 'uniform':
        return np.random.RandomState(seed).uniform(-1.3, 1.3, shape).astype(np.float32)
    return tc.fill(shape, tc.boundary_values() if kind == 'boundary' else tc.tie_values(), seed)


CASES = [  # (tiles, C, grid, first_tile) for N = 5 images
    ('hwc', 1, None, 0), ('hwc', 3, (3, 2), 1), ('hwc', 3, (5, 1), 0),
    ('grey', 2, (3, 4), 2), ('grey', 3, None, 0), ('grey', 1, (2, 3), 1),
    (0, 2, (3, 2), 0), (1, 2, (4, 2), 3), (2, 3, None, 0),
]


@pytest.mark.parametrize('mode,lo,hi,kind', [('trunc', -1, 1, 'uniform'), ('trunc', -1, 1, 'boundary'),
                                             ('rint', -1, 1, 'uniform'), ('rint', -1, 1, 'boundary'),
                                             ('rint', 0, 255, 'ties'), ('rint', -0.3, 1.7, 'uniform')])
@pytest.mark.parametrize('tiles,c,grid,first_tile', CASES)
def test_image_tiles_u8_ref_against_numpy(tiles, c, grid, first_tile, mode, lo, hi, kind):
    from torch_utils.ops import image_tiles
    n, h, w = 5, 16, 12
    x = _inputs(kind, (n, c, h, w), seed=h + c)
    t = tc.n_tiles(x.shape, tiles)
    g = grid or (t, 1)
    cout = c if tiles == 'hwc' else 1
    want, mask = tc.np_tiles(x, np.full([g[1] * h, g[0] * w, cout], 0xA5, np.uint8), mode, lo, hi, tiles, g, first_tile)
    canvas = torch.full([g[1] * h, g[0] * w, cout], 0xA5, dtype=torch.uint8)
    got = image_tiles.image_tiles_u8_ref(torch.from_numpy(x), out=canvas, mode=mode, lo=lo, hi=hi, tiles=tiles, grid=grid,
                                         first_tile=first_tile)
    assert got is canvas
    assert np.array_equal(got.numpy(), want)
    assert (got.numpy()[~mask] == 0xA5).all() and mask.sum() == t * h * w * cout
    if first_tile == 0:     # out=None: a black canvas
        fresh = image_tiles.image_tiles_u8_ref(torch.from_numpy(x), mode=mode, lo=lo, hi=hi, tiles=tiles, grid=grid)
        want0, _ = tc.np_tiles(x, np.zeros_like(want), mode, lo, hi, tiles, g, 0)
        assert np.array_equal(fresh.numpy(), want0)


def test_image_tiles_u8_ref_ties_round_to_even():
    from torch_utils.ops import image_tiles
    x = torch.tensor([0.5, 1.5, 2.5, 253.5, 254.5, 255.5, -0.5]).reshape(1, 1, 1, 7)
    got = image_tiles.image_tiles_u8_ref(x, mode='rint', lo=0, hi=255).flatten().tolist()
    assert got == [0, 2, 2, 254, 254, 255, 0]


def test_image_tiles_u8_ref_widens_16_bit_first():
    from torch_utils.ops import image_tiles
    x = torch.from_numpy(tc.fill((2, 1, 4, 8), tc.boundary_values(), 1))
    for dt in (torch.float16, torch.bfloat16):
        xs = x.to(dt)
        for mode in ('trunc', 'rint'):
            assert torch.equal(image_tiles.image_tiles_u8_ref(xs, mode=mode),
                               image_tiles.image_tiles_u8_ref(xs.float(), mode=mode))


def test_image_tiles_argument_errors_on_cpu():
    from torch_utils.ops import image_tiles
    x = torch.zeros(2, 2, 4, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        image_tiles.image_tiles_u8(x, tiles='grey')
    ref = image_tiles.image_tiles_u8_ref
    with pytest.raises(RuntimeError, match='hwc'):
        ref(x, tiles='hwc')
    with pytest.raises(RuntimeError, match='channel'):
        ref(x, tiles=2)
    with pytest.raises(RuntimeError, match='grid'):
        ref(x, tiles='grey', grid=(3, 1))
    with pytest.raises(RuntimeError, match='first_tile'):
        ref(x, tiles='grey', first_tile=1)
    with pytest.raises(RuntimeError, match='out'):
        ref(x, tiles='grey', out=torch.zeros(4, 16, 1))
    with pytest.raises(RuntimeError, match='out'):
        ref(x, tiles='grey', out=torch.zeros(4, 12, 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='lo and hi'):
        ref(x, tiles='grey', mode='rint', lo=1, hi=1)
    with pytest.raises(RuntimeError, match='contiguous'):
        ref(x.permute(0, 1, 3, 2)[:, :, :, ::2], tiles='grey')
    with pytest.raises(RuntimeError, match='float32'):
        ref(x.to(torch.int32), tiles='grey')
    with pytest.raises(RuntimeError, match='mode'):
        ref(x, tiles='grey', mode='round')


# ---- the CLIs ----

@pytest.mark.parametrize('module', ['gen_images_mi_multimodal', 'gen_images_style_mixing', 'gen_video'])
def test_cli_help(module):
    import importlib
    from click.testing import CliRunner
    res = CliRunner().invoke(importlib.import_module(module).main, ['--help'])
    assert res.exit_code == 0, res.output
    assert '--network' in res.output and '--trunc' in res.output


def test_cli_bad_seeds_is_a_usage_error():
    import gen_images_mi_multimodal as cli
    from click.testing import CliRunner
    res = CliRunner().invoke(cli.main, ['--network', 'none.pkl', '--seeds', 'a-b', '--outdir', 'x'])
    assert res.exit_code == 2 and '--seeds' in res.output


def test_video_without_imageio_says_so(tmp_path):
    try:
        import imageio  # noqa: F401
        return      # installed: the branch under test cannot be reached
    except ImportError:
        pass
    import gen_video
    from click.testing import CliRunner
    res = CliRunner().invoke(gen_video.main, ['--network', 'none.pkl', '--seeds', '0,1', '--output',
                                              str(tmp_path / 'lerp.mp4')])
    assert res.exit_code != 0 and 'imageio' in res.output


# ---- the C entry point ----

def test_library_exports_image_tiles():
    import sg2hip
    lib = sg2hip.lib()
    assert 'sg2_image_tiles_u8' in sg2hip.SIGNATURES and hasattr(lib, 'sg2_image_tiles_u8')
    p = ctypes.c_void_p(64)

    def call(canvas=p, img=p, dtype=0, n=2, c=2, h=4, w=4, tiles=-2, mode=0, lo=-1.0, hi=1.0, gw=4, gh=1, first=0):
        rc = lib.sg2_image_tiles_u8(canvas, img, dtype, n, c, h, w, tiles, mode, lo, hi, gw, gh, first, None)
        return rc, lib.sg2_last_error().decode()

    for kw, word in ((dict(canvas=None), 'non-null'), (dict(dtype=3), 'dtype'), (dict(n=0), 'at least 1'),
                     (dict(tiles=-1), 'SG2_TILES_HWC needs'), (dict(tiles=2), 'channel'), (dict(tiles=-3), 'tiles'),
                     (dict(mode=2), 'mode'), (dict(gw=0), 'grid'), (dict(gw=3), 'exceeds the grid'),
                     (dict(first=1), 'exceeds the grid'), (dict(first=-1), 'exceeds the grid'),
                     (dict(mode=1, lo=2.0, hi=2.0), 'differ'), (dict(mode=1, hi=float('nan')), 'finite'),
                     (dict(mode=1, hi=float('inf')), 'finite'), (dict(img=ctypes.c_void_p(66)), 'aligned')):
        rc, msg = call(**kw)
        assert rc < 0 and word in msg, (kw, rc, msg)
