"""The case tables, the float64 references, the bounds and the restated host rules of tests/conv_rules.py, held on the CPU (nothing is
launched): every case reaches the plan it names -- by dl3p_conv2d_gemm_plan_query AND by the Python restatement of the planner --,
the tables reach every instantiation, the kernels' index arithmetic is exact over its whole claimed domain, a float32 evaluation of
every route stays inside the bounds in two summation orders, and the three references are adjoint to each other."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from conftest import load_pkg  # noqa: E402
import conv_rules as R  # noqa: E402

F = np.float32


def _ops():
    return load_pkg('ops')


@pytest.fixture
def options():
    """dl3p_set_option for the time of a test; every knob touched goes back to 'not set'"""
    L = load_pkg('_lib').lib()
    touched = {}
    routed = L.get_option(b'split_wgrad')

    def set_(name, v):
        touched[name] = True
        assert L.set_option(name.encode(), v) == 0
    yield set_
    for name in touched:
        L.set_option(name.encode(), {'conv_sb': -1, 'wgrad_tile': -1, 'split_wgrad_tile': -1, 'split_wgrad': routed}.get(name, 0))


def test_case_names_are_unique_and_every_case_names_its_edge():
    for table in (R.GEMM, R.WGRAD, R.STEM, R.DIRECT):
        assert len({c.name for c in table}) == len(table)
        assert all(len(c.edge) > 10 for c in table)


def test_geometry_is_the_wrappers_geometry():
    ops = _ops()
    for c in R.GEMM + R.WGRAD + R.DIRECT:
        assert R.conv_geometry(c.H, c.W, c.k, c.s, c.r, c.pad) == ops.conv_geometry(c.H, c.W, c.k, c.s, c.r, c.pad), c.name
    for c in R.STEM:
        assert R.conv_geometry(c.H, c.W, 3, 2, 1, c.pad) == ops.conv_geometry(c.H, c.W, 3, 2, 1, c.pad), c.name


def _tuple(pl):
    return (pl['nt'], pl['mi'], pl['gx'], pl['gy'], pl['m_tiles'], 0)


def test_case_table_reaches_its_plans(options):
    """the tile / form / trip count a case names == dl3p_conv2d_gemm_plan_query == the planner restated in conv_rules"""
    ops = _ops()
    cus, rows = R.machine()
    assert (cus, rows) == (256, 2048)
    wrong = {}
    options('conv_sb', 2)
    for c in R.GEMM:
        for which, role, (M, K, N) in zip('fd', (0, 2), R.gemm_shapes(c)):
            want = getattr(c, which)
            if which == 'f' and not ops.conv2d_gemm_supported(c.Cin, c.Cout, c.k, c.s):
                continue
            got = ops.conv2d_gemm_plan_query(role, M, K, N)
            mine = R.plan_conv_gemm(M, N, cus, rows)
            if got != _tuple(mine) or (want is not None and want != (mine['nt'], mine['mi'], R.trips(mine))):
                wrong[c.name, which] = (got, mine, want)
            if role == 0:
                assert ops.conv2d_gemm_plan_query(1, M, K, N) == got
            # the split twin (roles 5 / 6 / 7): the restated plan where the shape is served, -1 where it is not
            for twin in ((5, 6) if role == 0 else (7,)):
                sb = ops.conv2d_gemm_plan_query(twin, M, K, N)
                if R.conv_sb_supported(role, M, K, N):
                    if sb != _tuple(R.plan_gemm_sb_ga(M, N, cus, rows)):
                        wrong[c.name, which, twin] = (sb, R.plan_gemm_sb_ga(M, N, cus, rows))
                elif sb[0] != -1:
                    wrong[c.name, which, twin] = sb
    for c in R.WGRAD:
        g = R.geo_of(c)
        M, K, N = c.N * g.Ho * g.Wo, c.k * c.k * c.Cin, c.Cout
        options('conv_sb', 0 if c.sb is None else 2)
        options('wgrad_tile', c.tile)
        options('split_wgrad', 1)
        options('split_wgrad_tile', -1 if c.sb is None else c.sb)
        got = ops.conv2d_gemm_plan_query(4, M, K, N)
        mine = R.plan_conv_wgrad(M, K, N, cus, rows, 0 if c.sb is None else 2, c.tile, -1 if c.sb is None else c.sb)
        if got != (mine['form'], mine['tile'], mine['tiles'], mine['slabs'], mine['mchunk'], 0) or got[:4] != c.want:
            wrong[c.name] = (got, mine, c.want)
        # the workspace the entry point asks for holds the slabs the plan writes
        assert ops.lib().conv2d_gemm_bwd_weight_workspace(c.N, g.Ho, g.Wo, c.Cin, c.Cout, c.k) >= 4 * got[3] * K * N, c.name
    assert not wrong, wrong


def test_the_tables_reach_every_instantiation():
    cus, rows = R.machine()
    plans = []
    for c in R.GEMM:
        for (M, K, N) in R.gemm_shapes(c):
            plans.append(R.plan_conv_gemm(M, N, cus, rows))
    assert {p['nt'] for p in plans} == set(range(1, 9))
    assert {p['mi'] for p in plans} == {1, 2}
    # the second trip of the persistent loop, under the default plan, at both tile heights
    assert {p['mi'] for p in plans if p['gx'] < p['m_tiles']} == {1, 2}
    # the split twins run wherever they are served: their plans reach every nt, both tile heights and a second trip as well
    sb = [R.plan_gemm_sb_ga(M, N, cus, rows) for _, _, (M, K, N) in R.split_cases()]
    assert {p['nt'] for p in sb} == set(range(1, 9)) and {p['mi'] for p in sb} == {1, 2}
    assert any(p['gx'] < p['m_tiles'] for p in sb) and any(p['mi'] == 2 and p['nt'] > 1 for p in sb)
    assert {role for _, role, _ in R.split_cases()} == {0, 2}
    assert {c.want[1] for c in R.WGRAD if c.want[0] == 0} == {0, 1, 2, 3}
    assert sorted(c.sb for c in R.WGRAD if c.sb is not None) == [0, 1, 2, 3, 4]
    assert {c.want[1] for c in R.WGRAD if c.want[0] == 4} == {0, 1, 2, 3}
    by = {c.name: c for c in R.GEMM}
    (M, K, N), _ = R.gemm_shapes(by['ntail_f100'])
    assert by['ntail_f100'].f == (7, 1, 1) and R.cdiv(M, 64) * R.cdiv(R.cdiv(N, 16), 8) <= 6 * cus      # (7: the small-grid regime only)
    (M, K, N), _ = R.gemm_shapes(by['mi2'])
    assert R.plan_conv_gemm(M - 128, N, cus, rows)['mi'] == 1 and R.plan_conv_gemm(M, N, cus, rows)['mi'] == 2      # the smallest M
    # row counts against the 64-row tile, M = 1, the split kernel's own smallest / odd sizes, K tails
    ms = {R.gemm_shapes(c)[0][0] for c in R.GEMM}
    assert {m % 64 for m in ms} >= {0, 1, 63} and 1 in ms and {1024, 1025, 1087} <= ms
    ks = {R.gemm_shapes(c)[0][1] for c in R.GEMM}
    assert {k % 32 for k in ks} >= {0, 4, 12, 28} and {4, 65464} <= ks
    assert {c.k for c in R.GEMM} == {1, 2, 3, 4, 5, 7} and {c.Cin for c in R.GEMM} >= {4, 12, 20, 36}
    assert any(K % 8 == 4 for _, role, (M, K, N) in R.split_cases() if role == 0) and any(K % 8 == 4 for _, role, (M, K, N) in R.split_cases() if role == 2)
    wm = [c.N * R.geo_of(c).Ho * R.geo_of(c).Wo for c in R.WGRAD]
    assert {m % 32 for m in wm} >= {1, 31} and max(wm) >= 1 << 20
    assert {R.geo_of(c).Wo for c in R.WGRAD} >= {1, 3, 5, 7, 127, 129} and {R.geo_of(c).Ho for c in R.WGRAD} >= {1, 3, 5, 7, 127, 129}


def test_unsupported_reductions_are_refused():
    ops = _ops()
    assert ops.conv2d_gemm_supported(1336, 16, 7, 1) and not ops.conv2d_gemm_supported(1340, 16, 7, 1)
    assert 49 * 1336 == 65464 < 65536 <= 49 * 1340


# ------------------------------------------------------------------------------------------------ index arithmetic
def test_cmagic_is_exact_for_every_admitted_channel_count():
    """tap = umulhi(k, floor(2^32 / C) + 1) == k // C for every C % 4 == 0 and every k < 2^16 (a superset of k k C < 65536, k = 1 .. 7).
    umulhi is monotone in k and k // C is a step function, so it is enough to hold at both sides of every step: k = q C - 1 and q C;
    every k is checked outright for the channel counts of the tables and all C <= 256."""
    for C in range(4, 65536, 4):
        q = np.arange(1, 65535 // C + 1, dtype=np.int64)
        assert np.array_equal(R.tap_of(q * C, C), q) and np.array_equal(R.tap_of(q * C - 1, C), q - 1), C
        assert R.tap_of(65535, C) == 65535 // C
    k = np.arange(65536, dtype=np.int64)
    for C in sorted(set(range(4, 257, 4)) | {c.Cin for c in R.GEMM} | {c.Cout for c in R.GEMM}):
        assert np.array_equal(R.tap_of(k, C), k // C), C
    # the mutation the rule is one step away from: floor(2^32 / C) without the + 1 is off at k = C for every C that is no power of 2
    assert ((np.uint64(12) * np.uint64((1 << 32) // 12)) >> np.uint64(32)) == 0


def test_kwmagic_is_exact_for_every_tap():
    for k in range(1, 8):
        tap = np.arange(k * k)
        assert np.array_equal(R.ky_of(tap, k), tap // k), k
    # ... and one step away it is not: 65536 // k without the + 1 puts tap 3 of a 3 x 3 kernel into row 0
    assert R.ky_of(3, 3, 65536 // 3) == 0 and R.ky_of(3, 3) == 1


def test_divmod_small_is_exact_over_the_24_bit_range():
    a = np.arange(1 << 24, dtype=np.int32)
    ds = {1, 2, 3, 16383}
    for c in R.WGRAD:
        g = R.geo_of(c)
        ds |= {g.Wo, g.Ho}
    uncorrected = 0
    for d in sorted(ds):
        q, r = R.divmod_small(a, d)
        assert np.array_equal(q, a // d) and np.array_equal(r, a % d), d
        uncorrected += int((R.divmod_small(a, d, correct=False)[0] != a // d).sum())
    assert uncorrected > 0      # the correction step is not decoration: without it some row of some divisor decodes wrongly
    # ... and the table has rows that need it, so that the GPU file notices a kernel without it
    need = set()
    for c in R.WGRAD:
        g = R.geo_of(c)
        m = a[:c.N * g.Ho * g.Wo]
        if (R.divmod_small(m, g.Wo, correct=False)[0] != m // g.Wo).any():
            need.add(c.name)
    assert need >= {'w_wo41', 'w_big'}, need


def test_the_parity_rule_is_the_references_tap_test():
    """stride-2 data gradient: a tap at ty = iy + pad_t - ky rate exists iff ty >= 0, ty even and ty / 2 < Ho; ty >> 1 of a negative or
    odd ty is a VALID row index (-1 >> 1 = -1, 3 >> 1 = 1), so everything hangs on the sign test and the parity mask"""
    for c in R.GEMM:
        if c.s != 2:
            continue
        g = R.geo_of(c)
        pix, ok = (t.numpy() for t in R.tap_index(g))
        reach = np.zeros((g.H, g.W, g.k, g.k), bool)                   # (input pixel, tap) pairs of the float64 reference
        for m in range(g.Ho * g.Wo):
            for t in range(g.k * g.k):
                if ok[m, t]:
                    reach[pix[m, t] // g.W, pix[m, t] % g.W, t // g.k, t % g.k] = True
        iy, ix, ky, kx = np.meshgrid(np.arange(g.H), np.arange(g.W), np.arange(g.k), np.arange(g.k), indexing='ij')
        ty, tx = iy + g.pt - ky * g.r, ix + g.pl - kx * g.r
        got, sy, sx = R.parity_tap(ty, tx, 1, g.Ho, g.Wo)
        assert np.array_equal(got, reach), c.name
        if c.name == 's2_0101_odd':
            assert (ty < 0).any() and (ty % 2 == 1).any()
            # without the mask: odd ty would read row ty >> 1; without the sign test: ty = -1 would pass as row -1 < Ho
            assert (((ty >= 0) & (tx >= 0) & (sy < g.Ho) & (sx < g.Wo)) != reach).any()
    ok, sy, _ = R.parity_tap([-2, -1, 0, 1, 2, 3], [0] * 6, 1, 2, 1)
    assert ok.tolist() == [False, False, True, False, True, False] and sy.tolist() == [-1, -1, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ stem and direct rules
def test_stem_cases_sit_on_both_sides_of_the_interior_rule():
    got = {}
    for c in R.STEM:
        Ho, Wo, pt, pl = R.conv_geometry(c.H, c.W, 3, 2, 1, c.pad)
        got[c.name] = (R.stem_interior_tiles(c.H, c.W, pt, pl, Ho, Wo), pl, Wo, c.N * Ho * R.stem_segments(Wo))
        assert got[c.name][0] == c.interior, (c.name, got[c.name])
    assert [got[n][0] for n in ('st_w128', 'st_w129', 'st_w130')] == [0, 1, 1] and all(got[n][1] == 0 for n in ('st_w128', 'st_w129', 'st_w130'))
    assert [got[n][0] for n in ('st_w255', 'st_w256', 'st_w257')] == [0, 1, 1] and all(got[n][1] == 1 for n in ('st_w255', 'st_w256', 'st_w257'))
    assert {got[n][2] for n in got} >= {1, 63, 64, 65, 128, 129} and {c.H for c in R.STEM} >= {2, 3, 4}
    assert any(got[n][3] % 4 for n in got) and {c.Cout for c in R.STEM} == {16, 32}


def test_wchunk_launches_and_patch_padding():
    assert R.wchunks(27) == [(0, 27)] and R.wchunks(147) == [(0, 32), (32, 32), (64, 32), (96, 32), (128, 19)]
    assert R.ld_col(27) == 28 and R.ld_col(147) == 148 and R.ld_col(36) == 36
    ks = {c.k * c.k * c.Cin for c in R.DIRECT}
    assert {27, 147} <= ks and {c.Cout for c in R.DIRECT} >= {4, 16, 64}


# ------------------------------------------------------------------------------------------------ references and bounds
BIG = 1 << 17      # cases from here up are emulated on a slice of their output columns


def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64))


def _inside(got, chk, what):
    chk.verify(torch.from_numpy(got.astype(np.float64)), what)
    return chk.worst(torch.from_numpy(got.astype(np.float64)))


@pytest.mark.parametrize('c', R.GEMM, ids=lambda c: c.name)
def test_float32_reference_stays_inside_its_bound(c):
    """forward (with the prologue and a bias) and data gradient (onto a base of another magnitude), float32 op for op in two
    summation orders: inside the bound, and the bound is no free pass -- the worst element's error is above 0.02 U sum|terms|, where an
    evaluation in float64 would sit nine orders below"""
    d, g = R.conv_inputs(c), R.geo_of(c)
    (Mf, Kf, Nf), (Md, Kd, Nd) = R.gemm_shapes(c)
    cols = slice(0, 8) if max(Mf * Kf * Nf, Md * Kd * Nd) >= (1 << 26) else slice(None)
    a32 = R.pro32(d['x'], d['sc'], d['sh'], d['act'])
    P32 = R.patches32(a32, g)
    chk = R.fwd_ref(_t(d['x']), _t(d['w']), g, _t(d['sc']), _t(d['sh']), d['act'], bias=_t(d['bias']))
    n_max, chk = chk.n, R.Check(chk.ref[:, cols], chk.bound[:, cols])
    chk.n = n_max
    worst = 0.0
    for order in (0, 1):
        y = R.matmul32(P32, d['w'], order, cols) + d['bias'][cols]
        worst = max(worst, _inside(y, chk, '%s forward order %d' % (c.name, order)))
    assert 0.02 < worst * float(chk.n.max()) and worst <= 1.0, worst
    # data gradient: the terms of an input pixel in (output pixel, tap, co) order and reversed
    pix, ok = (t.numpy() for t in R.tap_index(g))
    w3 = d['w'].reshape(g.k * g.k, c.Cin, c.Cout)
    dcols = slice(0, 8) if cols != slice(None) else slice(None)
    chk = R.dgrad_ref(_t(d['dy']), _t(d['w']), g, c.Cin, base=_t(d['xbase']))
    if c.name == 's2_k1':      # three input pixels in four have no tap: the kernel must write +0 there
        assert float(chk.reached.double().mean()) == (4 * 3) / (7 * 6)
    ref = R.Check(chk.ref[:, dcols], chk.bound[:, dcols])
    ref.n = chk.n
    worst = 0.0
    for order in (0, 1):
        gx = d['xbase'][:, dcols].copy()
        taps = range(g.k * g.k) if order == 0 else reversed(range(g.k * g.k))
        for t in taps:
            part = R.matmul32(d['dy'], np.ascontiguousarray(w3[t].T), order, dcols).reshape(c.N, g.Ho * g.Wo, -1)
            dst = gx.reshape(c.N, c.H * c.W, -1)
            for n in range(c.N):
                np.add.at(dst[n], pix[ok[:, t], t], part[n][ok[:, t]])
        worst = max(worst, _inside(gx, ref, '%s data gradient order %d' % (c.name, order)))
    assert 0.02 < worst * float(chk.n.max()) and worst <= 1.0, worst


@pytest.mark.parametrize('c', R.WGRAD, ids=lambda c: c.name)
def test_float32_weight_gradient_stays_inside_its_bound(c):
    d, g = R.conv_inputs(c), R.geo_of(c)
    M = c.N * g.Ho * g.Wo
    cols = slice(0, 4) if M >= BIG else slice(None)
    a32 = R.pro32(d['x'], d['sc'], d['sh'], d['act'])
    P32 = R.patches32(a32, g)
    chk = R.wgrad_ref(_t(d['x']), _t(d['dy'][:, cols]), g, _t(d['sc']), _t(d['sh']), d['act'])
    worst = 0.0
    for order in (0, 1):
        gw = np.empty((P32.shape[1], d['dy'][:, cols].shape[1]), F)
        for j in range(gw.shape[1]):
            gw[:, j] = R.sum32(P32 * d['dy'][:, cols][:, j:j + 1], order)
        worst = max(worst, _inside(gw, chk, '%s order %d' % (c.name, order)))
    assert 0.02 < worst * float(chk.n.max()) and worst <= 1.0, worst


@pytest.mark.parametrize('c', [c for c in R.GEMM if c.N * c.H * c.W <= 4096], ids=lambda c: c.name)
def test_the_three_references_are_adjoint(c):
    """<conv(x), dy> = <x, dgrad(dy)> = <w, wgrad(x, dy)> in float64 (no prologue: the identities are those of the linear map)"""
    d, g = R.conv_inputs(c), R.geo_of(c)
    x, w, dy = _t(d['x']), _t(d['w']), _t(d['dy'])
    y, gx, gw = R.fwd_ref(x, w, g), R.dgrad_ref(dy, w, g, c.Cin), R.wgrad_ref(x, dy, g)
    a, b, e = float((y.ref * dy).sum()), float((x * gx.ref).sum()), float((w * gw.ref).sum())
    scale = float((y.mag * dy.abs()).sum())
    assert abs(a - b) <= 1e-12 * scale and abs(a - e) <= 1e-12 * scale, (a, b, e)
    # the magnitudes are adjoint too (the same identity on |operands|), and the term counts add up to the same total
    assert abs(float((y.mag * dy.abs()).sum()) - float((x.abs() * gx.mag).sum())) <= 1e-12 * scale
    assert float(y.n.sum()) * c.Cout == float(gx.n.sum()) * c.Cin == float(gw.n.sum()) * c.Cout
    assert bool((gx.ref[~gx.reached] == 0).all())


def test_padding_applies_to_the_activation_not_to_the_input():
    """a prologue with act(shift) != 0: padding x instead of a would be off by a whole term, far outside the bound"""
    c = next(c for c in R.GEMM if c.name == 'rate_ge_h')
    d, g = R.conv_inputs(c), R.geo_of(c)
    chk = R.fwd_ref(_t(d['x']), _t(d['w']), g, _t(d['sc']), _t(d['sh']), d['act'])
    wrong = chk.ref + (torch.relu(_t(d['sh'])).repeat(g.k * g.k)[None] @ _t(d['w'])) - \
        (R.patches(torch.relu(_t(d['sh']))[None].expand(c.N * c.H * c.W, -1), g).reshape(-1, g.k * g.k * c.Cin) @ _t(d['w']))
    assert float(((wrong - chk.ref).abs() / chk.bound).min()) > 1e3
