"""The judges, fixtures and dispatch plans of tests/test_conv_f32_gpu.py, checked without a GPU.

The GPU file holds the f32 convolutions of csrc/conv.hip -- the three-way bf16 split in-loop ('s3') and on
pre-split planes ('p3'), and the f32-input MFMA ('exact') -- to two judges built in tests/elementwise.py.  Here:

  * mutants: a CPU emulation of the six-product scheme (bf16 round-to-nearest-even splits, f32 accumulation per
    32-deep K stage in mfma_s3's order) equals float64 bitwise on each plane fixture, and leaving out any product a
    fixture needs changes at least 90 % of its nonzero outputs; the three fixtures cover all six products.  On
    normal operands the full scheme sits far inside Judge 2's bound -- and so do the three low-product mutants,
    which is why Judge 1 exists;
  * preconditions: the exact integer fixture (every sum of |terms| below 2^24 quanta) and the plane fixtures (one
    product per output) for every case of both tables;
  * edge reach: conv_fwd_plan / conv_wgrad_plan, which mirror the host dispatch read from conv.hip, on the case
    tables reach every edge the GPU file is meant to reach; each assertion names its edge.
"""
import pytest
import torch
import torch.nn.functional as F

import elementwise as EW

FWD, WGRAD = EW.CF_FWD_CASES, EW.CF_WGRAD_CASES
LOW = ('lh', 'hl', 'mm')


def _fwd_forms(name):
    return EW.cf_forms(FWD[name][5])


def _wgrad_forms(name):
    A, B, k = WGRAD[name][:3]
    return EW.cf_forms((A, B), wgrad_1x1_small=k == 1 and min(A, B) <= 4)


# ------------------------------------------------------------------ the split and its mutants
def test_s3_split_is_exact_on_normals():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(64, generator=g) * 2.0 ** 100,
                   torch.randn(64, generator=g) * 2.0 ** -100, torch.tensor([0.0, -0.0, 1.0, -1.0])]).float()
    h, m, l = EW.s3_split(x)
    for p in (h, m, l):
        assert torch.equal(p.bfloat16().float(), p)
    assert torch.equal((h.double() + m.double() + l.double()).float(), x)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert float(m.abs().max()) > 0 and float(l.abs().max()) > 0


def _as_gemm(name, kind, sparse):
    """A plane fixture of the 1x1 case `name` as X [pixels, Cin] @ W [Cin, Cout] (f32) and its float64 product."""
    case = FWD[name]
    x, w = EW.cf_plane_fwd_operands(case, kind, sparse)
    X = x.permute(0, 2, 3, 1).reshape(-1, case[5]).float()
    W = w[:, :, 0, 0].t().contiguous().float()
    return X, W, X.double() @ W.double()


@pytest.mark.parametrize('sparse', ['a', 'b'])
@pytest.mark.parametrize('kind', list(EW.CF_PLANE_FIXTURES))
def test_plane_fixture_mutants(kind, sparse):
    X, W, ref = _as_gemm('f1', kind, sparse)
    assert torch.equal(EW.s3_matmul_emulated(X, W).double(), ref), 'the six-product scheme is not exact on the fixture'
    nz = ref != 0
    needs = EW.CF_PLANE_FIXTURES[kind]
    for drop in EW.S3_ORDER:
        changed = (EW.s3_matmul_emulated(X, W, drop=drop).double() != ref) & nz
        share = float(changed.sum()) / float(nz.sum())
        print(f'plane fixture {kind} sparse {sparse}: dropping {drop} changes {share:.3f} of the nonzero outputs')
        if drop in needs:
            assert share >= 0.9, (kind, drop, share)
        else:
            assert share == 0, (kind, drop, share)


def test_plane_fixtures_cover_all_six_products():
    assert set().union(*map(set, EW.CF_PLANE_FIXTURES.values())) == set(EW.S3_ORDER)


@pytest.mark.parametrize('K', [72, 1152])
def test_bound_holds_the_scheme_and_cannot_see_a_low_product(K):
    """Normal operands: the emulation within Judge 2's bound; the mutants that drop l h', h l' or m m' also stay
    inside it (Judge 2 alone would pass a kernel with half of its products missing) while dropping the leading
    product does not."""
    g = torch.Generator().manual_seed(K)
    X, W = torch.randn(96, K, generator=g), torch.randn(K, 48, generator=g) / K ** 0.5
    ref, A = X.double() @ W.double(), X.double().abs() @ W.double().abs()
    slack = EW.conv_f32_slack('s3', K, 1, A)
    full = EW.assert_elementwise(EW.s3_matmul_emulated(X, W), ref, slack, torch.float32, f'emulation K {K}')
    line = [f'full {full:.3g}']
    for drop in LOW:
        r = EW.assert_elementwise(EW.s3_matmul_emulated(X, W, drop=drop), ref, slack, torch.float32, f'mutant {drop}')
        line.append(f'-{drop} {r:.3g}')
    print(f'six-product emulation K {K}: worst error / bound ' + ', '.join(line))
    # (the bound grows as K^2: at K = 1152 it only refuses the loss of the leading product)
    for drop in ('mh', 'hm', 'hh') if K == 72 else ('hh',):
        assert float(EW.ratios(EW.s3_matmul_emulated(X, W, drop=drop), ref, slack, torch.float32).max()) > 1, drop
    exact = EW.conv_f32_slack('exact', K, 1, A)
    EW.assert_elementwise(X @ W, ref, exact, torch.float32, 'f32 matmul')


def test_emulation_is_exact_on_the_integer_fixture():
    op, refs = EW.cf_fwd_exact_refs(FWD['f1'])
    X = (op['x'].float() * op['in_scale'].float()[:, :, None, None]).permute(0, 2, 3, 1).reshape(-1, 72)
    W = op['w'][:, :, 0, 0].t().contiguous().float()
    got = EW.s3_matmul_emulated(X, W).double().view(3, 7, 7, 24).permute(0, 3, 1, 2)
    assert torch.equal(got, refs['full']['c'])
    assert not torch.equal(EW.s3_matmul_emulated(X, W, drop='hh').double().view(3, 7, 7, 24).permute(0, 3, 1, 2),
                           refs['full']['c'])


# ------------------------------------------------------------------ preconditions
@pytest.mark.parametrize('name', list(FWD))
def test_exact_fixture_precondition_fwd(name):
    op, refs = EW.cf_fwd_exact_refs(FWD[name])          # asserts the precondition
    full = refs['full']
    assert float((full['y'] - op['residual']).abs().max()) == EW.CF_EXACT['clamp'], 'the clamp is never reached'
    assert float(((full['v'].abs() < EW.CF_EXACT['clamp']) & (full['v'] < 0)).double().mean()) > 0.05, 'no lrelu side'


@pytest.mark.parametrize('name', list(WGRAD))
def test_exact_fixture_precondition_wgrad(name):
    op, refs = EW.cf_wgrad_exact_refs(WGRAD[name])
    assert float(refs['scaled'].abs().max()) > 0 and refs['scaled'].shape == refs['plain'].shape


@pytest.mark.parametrize('sparse', ['a', 'b'])
@pytest.mark.parametrize('kind', list(EW.CF_PLANE_FIXTURES))
def test_plane_fixtures_have_one_term_per_output(kind, sparse):
    for name in EW.CF_PLANE_FWD:
        case = FWD[name]
        x, w = EW.cf_plane_fwd_operands(case, kind, sparse)
        terms = F.conv2d((x != 0).double(), (w != 0).double(), stride=case[1], padding=case[2])
        EW.cf_plane_assert_one_term(terms, F.conv2d(x, w, stride=case[1], padding=case[2]), (name, kind, sparse))
    for name in EW.CF_PLANE_WGRAD:
        A, B, k, stride, pad = WGRAD[name][:5]
        g, x = EW.cf_plane_wgrad_operands(WGRAD[name], kind, sparse)
        kw = dict(stride=stride, padding=pad)
        terms = torch.nn.grad.conv2d_weight((x != 0).double(), (A, B, k, k), (g != 0).double(), **kw)
        EW.cf_plane_assert_one_term(terms, torch.nn.grad.conv2d_weight(x, (A, B, k, k), g, **kw), (name, kind, sparse))


# ------------------------------------------------------------------ edge reach of the case tables
def _plan(name, form='s3', **kw):
    return EW.conv_fwd_plan(*FWD[name], form=form, **kw)


def test_fwd_edges():
    p = _plan('f3')
    assert p['phases'][0][0] == 147 and 147 - p['BM'] == 19, 'f3: a 19-row second M tile'
    assert 147 // 49 == 3 and p['BM'] > 2 * 49, 'f3: a tile spanning three samples'
    assert p['nck'] == 2 and p['live_last'] == 8 == p['BK'] // 4, 'f3: nck 2 with a quarter-live last K stage'
    assert p['BN'] == 64 and FWD['f3'][8] == 40, 'f3: Cout 40 in a 64 tile'
    assert p['splits'] == 4 and p['split_steps'][0] == [5, 5, 5, 3], 'f3: 4 splits, the last short'
    assert _plan('f3', 'p3')['live_last'] == 8 and 'p3' in _fwd_forms('f3'), 'f3: the c < Cin mask of a P3 K stage'
    p = _plan('f3w')
    assert p['BN'] == 128 and p['grid'][1] == 2 and FWD['f3w'][8] - 128 == 8, 'f3w: BN 128, second N tile 8 live'
    assert FWD['f3w'][5] == 8 and p['live_last'] == 8 and p['splits'] == 2 and 'p3' in _fwd_forms('f3w'), 'f3w: Cin 8'
    for form in EW.CF_FORMS:
        p = _plan('f1', form)
        assert max(nk for _, _, nk in p['phases']) // 4 <= 1 and p['splits'] == 1, 'f1: never splits'
    assert _plan('f1')['phases'][0][2] // 4 == 0, 'f1: maxnk // 4 == 0'
    for form in EW.CF_FORMS:
        p = _plan('f1d', form)
        assert p['splits'] > 1 and p['phases'][0][1] == 1, 'f1d: a 1x1 that splits'
        assert p['BN'] == 128 and FWD['f1d'][8] == 72, 'f1d: wide ragged Cout'
    assert FWD['fd'][1] == 2 and not FWD['fd'][3] and _plan('fd')['splits'] == 2, 'fd: stride-2 taps'
    for form in EW.CF_FORMS:
        p = _plan('fu', form)
        assert [(M, t) for M, t, _ in p['phases']] == [(168, 4), (144, 2), (140, 2), (120, 1)], 'fu: four phases'
        assert (3, 1) in p['early_return'], 'fu: an early-return tile (if (m0 >= M) return)'
        assert p['splits'] > 1 and {ph for ph, _ in p['empty']} == {1, 2, 3}, 'fu: empty splits in the short phases'
        assert all(s[0] > 0 for s in p['split_steps']), 'fu: every phase has work'
    p = _plan('fu')
    assert any(0 < s[0] < p['kper'] for s in p['split_steps']), 'fu: a phase with fewer K steps than kper'
    p = _plan('f1t')
    assert FWD['f1t'][3] and p['phases'] == [(72, 1, 1)] and p['splits'] == 1, 'f1t: the 1x1 data gradient'
    for form in ('s3', 'exact'):
        assert not _plan('fn', form)['vec'], 'fn: scalar-load form'
    assert _fwd_forms('fn') == ('s3', 'exact'), 'fn: no p3'
    for name, cout in (('frgb1', 1), ('frgb3', 3)):
        p = _plan(name)
        assert p['family'] == 'generic' and p['BN'] == 64 and FWD[name][8] == cout, 'frgb: a nearly empty N tile'
    for name in ('fk1_8', 'fk1_64', 'fk3_8', 'fk3_64'):
        assert _plan(name)['family'] == 'smallk' and _plan(name, 'exact')['family'] == 'smallk', 'fk: conv1x1_smallk'
        p = _plan(name, dot=True)
        assert p['family'] == 'smallk_dot', 'fk: conv1x1_smallk_dot'
        assert 0 < p['last_wg_pixels'] < EW.SK_ITERS * p['ppi'], 'fk: a partly empty last workgroup per sample'
        assert _fwd_forms(name) == ('s3', 'exact')
    assert _plan('fk1_64')['grid'][0] > 1 and _plan('fk1_64')['items'] % 256, 'fk: more than one block, a ragged last one'
    p = _plan('fk40')
    assert p['family'] == 'generic' and not p['vec'] and FWD['fk40'][5] == 3, 'fk40: the same depth on the generic kernel'
    assert _plan('f3', workspace=False)['splits'] == 1, 'no workspace: no split'


def _wplan(name, form='s3'):
    return EW.conv_wgrad_plan(*WGRAD[name], form=form)


def test_wgrad_edges():
    p = _wplan('w3')
    assert p['splits'] == 1 and p['K'] % 32 == 19 and (p['BM'], p['BN']) == (64, 64), 'w3: one split, ragged last chunk'
    p = _wplan('wA')
    assert (p['BM'], p['BN']) == (128, 64) and p['tiles'] == (2, 1), 'wA: 128x64 tile, two A tiles'
    assert p['splits'] == 2 and p['split_pixels'][1] % 32 and p['split_pixels'][1] < p['kper'], 'wA: second split ragged'
    p = _wplan('wB')
    assert (p['BM'], p['BN']) == (64, 128) and p['tiles'] == (1, 2) and p['splits'] == 2, 'wB: 64x128'
    p = _wplan('wAB')
    assert (p['BM'], p['BN']) == (128, 128) and WGRAD['wAB'][0] % 128 and WGRAD['wAB'][1] % 128, 'wAB: both ragged'
    assert WGRAD['wd'][3] == 2 and _wplan('wd')['family'] == 'generic', 'wd: stride 2'
    assert WGRAD['w1'][2] == 1 and _wplan('w1')['family'] == 'generic' and 'p3' in _wgrad_forms('w1'), 'w1: 1x1'
    assert not _wplan('wn')['vec'] and _wgrad_forms('wn') == ('s3', 'exact'), 'wn: scalar-load form'
    for name in WGRAD:
        if name.startswith('wsb') or name.startswith('wsa'):
            fam = 'smallb' if name.startswith('wsb') else 'smalla'
            for form in ('s3', 'exact'):
                assert _wplan(name, form)['family'] == fam, f'{name}: wgrad1x1_{fam} in f32'
            assert _wgrad_forms(name) == ('s3', 'exact')
    assert _wplan('wsb64_3')['grid'][0] > 1 and _wplan('wsb64_3')['items'] % 256, 'wsb: several blocks, a ragged one'
    assert _wplan('wsa3_64')['grid'][0] > 1, 'wsa: several blocks'
    assert _wplan('wsa3_64')['items'] < 4 * 256 * _wplan('wsa3_64')['grid'][0], 'wsa: the tail loop after the 4-pixel unroll'
    for name in ('w3', 'wA', 'wAB', 'w1'):
        assert 'p3' in _wgrad_forms(name) and WGRAD[name][1] % 4 == 0, f'{name}: the parameter-layout slot sum'


def test_plans_follow_the_split_rules():
    """splits = min(cdiv(512, blocks), maxnk // 4) over blocks < 512; kper = cdiv(maxnk, splits); wgrad: min(chunks //
    8, cdiv(1024, mt nt KK)), kper a multiple of BK, splits = cdiv(M, kper)."""
    p = EW.conv_fwd_plan(3, 1, 1, False, 4, 512, 4, 4, 512)
    assert (p['splits'], p['kper']) == (36, 4) and p['nck'] == 16
    p = EW.conv_fwd_plan(3, 1, 1, False, 64, 512, 32, 32, 512)
    assert p['splits'] == 1
    p = EW.conv_wgrad_plan(512, 512, 3, 1, 1, 64, 16, 16)
    assert p['chunks'] == 512 and p['splits'] == 8 and p['kper'] == 2048
    p = EW.conv_wgrad_plan(512, 512, 3, 1, 1, 64, 16, 16, form='exact')
    assert p['BK'] == 16 and p['chunks'] == 1024 and p['splits'] == 8
