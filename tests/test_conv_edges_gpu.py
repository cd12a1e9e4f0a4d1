"""The dense-conv kernels per element at their gather, tile and plan edges.

Every case of tests/conv_rules.py names the edge it reaches; tests/test_conv_rules_cpu.py holds the table to the planner.  Here every
entry point is called through ops.lib() on operands that sit in canary planes of their own (NaN-with-payload / +Inf / -Inf beside the
channels and in three rows after the last one, another layout per operand), every output element is held to the bound of
conv_rules -- (n + r + 1) U sum|terms|, no max|want| -- and every sentinel around an output must come back bit-identical.
The split-bf16 twins are held to 1e-5 sum|terms| and to 3 x the fp32 route's own worst figure on the same launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import conv_rules as R  # noqa: E402
from conv_rules import Plane, plane, out_plane, vec, ptr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def T64(a):
    return None if a is None else T(a).double()


class Flat:
    """a contiguous operand (a kernel matrix, a workspace) with NaN behind it"""

    def __init__(self, t, pad=64):
        t = t.reshape(-1)
        self.buf = torch.full((t.numel() + pad,), float('nan'), dtype=torch.float32, device=DEV)
        self.buf[:t.numel()] = t
        self.t, self.p = self.buf[:t.numel()], self.buf.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def L(ops):
    """ops.lib() with every option a test moved put back to 'not set' afterwards"""
    lib = ops.lib()
    moved = set()
    # the split weight gradient follows "split_wgrad", which a bf16 executor of an earlier test file leaves at 0: the cases that ask for
    # the split kernel pin it to 1; whatever was there is put back
    routed = lib.get_option(b'split_wgrad')

    class Opt:
        def __getattr__(self, name):
            return getattr(lib, name)

        def opt(self, name, v):
            moved.add(name)
            assert lib.set_option(name.encode(), v) == 0
    try:
        yield Opt()
    finally:
        for name in moved:
            lib.set_option(name.encode(), {'conv_sb': -1, 'wgrad_tile': -1, 'split_wgrad_tile': -1, 'split_wgrad': routed}.get(name, 0))


def geo_args(c, g):
    return (c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.r, g.pt, g.pl, g.Ho, g.Wo, stream())


# ------------------------------------------------------------------------------------------------ forward
def launch_fwd(L, ops, c, g, d, xp, sb, stats, bias, base_layout='off4'):
    """-> (y plane, statistic plane or None, rows)"""
    M, K = c.N * g.Ho * g.Wo, c.k * c.k * c.Cin
    y = out_plane(M, c.Cout, base_layout)
    wt = T(d['w']).t().contiguous()
    sc, sh, b = vec(d['sc']), vec(d['sh']), vec(d['bias'] if bias else None)
    rows = ctypes.c_int(-1)
    role = (5 if sb else 0) + (1 if stats else 0)
    plan = ops.conv2d_gemm_plan_query(role, M, K, c.Cout)
    part = Plane(2 * plan[2], c.Cout, 'contig') if stats else None
    if sb:
        wsp = ops.split_bf16x3(wt)
        L.conv2d_gemm_fwd_sb(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], wsp.data_ptr(), wsp.shape[2], ptr(b), y.p, y.ld,
                             part.p if stats else None, ctypes.byref(rows), *geo_args(c, g))
    else:
        w = Flat(wt)
        L.conv2d_gemm_fwd(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], w.p, ptr(b), y.p, y.ld, part.p if stats else None,
                          ctypes.byref(rows), *geo_args(c, g))
    torch.cuda.synchronize()
    assert rows.value == plan[2], (c.name, rows.value, plan)
    return y, part, rows.value


def check_stats(y, part, rows, what):
    """the statistic rows (sum, sum of squares per workgroup) add up to the device's own y; rows past rows_out are untouched"""
    part.intact(what + ' statistic rows')
    p = part.t.double().reshape(rows, 2, -1)
    s1, s2 = R.stat_check(y.t, rows)
    s1.verify(p[:, 0].sum(0), what + ' sum y')
    s2.verify(p[:, 1].sum(0), what + ' sum y^2')


@pytest.mark.parametrize('c', [c for c in R.GEMM if c.f is not None], ids=lambda c: c.name)
def test_forward_per_element(ops, L, c):
    g, d = R.geo_of(c), R.conv_inputs(c)
    L.opt('conv_sb', 2)
    xp = plane(T(d['x']), 'ld4')
    chk = R.fwd_ref(T64(d['x']), T64(d['w']), g, T64(d['sc']), T64(d['sh']), d['act'], bias=T64(d['bias']))
    y, part, rows = launch_fwd(L, ops, c, g, d, xp, False, True, True)
    y.intact(c.name)
    chk.verify(y.t, c.name + ' forward')
    check_stats(y, part, rows, c.name)
    # without statistics, in another layout: the same bits; without bias: its own reference
    y2, _, _ = launch_fwd(L, ops, c, g, d, xp, False, False, True, 'ld4')
    y2.intact(c.name)
    assert torch.equal(y2.t.view(torch.int32), y.t.view(torch.int32)), c.name + ': statistics change the output'
    y3, _, _ = launch_fwd(L, ops, c, g, d, xp, False, False, False, 'contig')
    y3.intact(c.name)
    R.fwd_ref(T64(d['x']), T64(d['w']), g, T64(d['sc']), T64(d['sh']), d['act']).verify(y3.t, c.name + ' forward, no bias')
    xp.intact(c.name + ' input')
    M, K = c.N * g.Ho * g.Wo, c.k * c.k * c.Cin
    if R.conv_sb_supported(0, M, K, c.Cout):
        e32 = chk.rel(y.t)
        for stats in (True, False):
            ys, part, rows = launch_fwd(L, ops, c, g, d, xp, True, stats, True)
            ys.intact(c.name + ' split')
            esb = chk.rel(ys.t)
            print('%s split forward: %.3g of sum|terms| (fp32 route %.3g)' % (c.name, esb, e32))
            assert esb < R.SB_ABS and esb < R.SB_REL * e32 + R.SB_FLOOR, (c.name, esb, e32)
            if stats:
                check_stats(ys, part, rows, c.name + ' split')
                first = ys
            else:
                assert torch.equal(ys.t.view(torch.int32), first.t.view(torch.int32))


def test_forward_refuses_a_reduction_of_2_to_the_16(ops, L):
    """k = 7, Cin = 1340: K = 65660 does not fit the 16-bit tap decode; the launch is refused and the output untouched"""
    x = plane(torch.ones(9, 1340, device=DEV), 'ld4')
    y = out_plane(9, 16, 'off4')
    w = Flat(torch.ones(16 * 49 * 1340, device=DEV))
    with pytest.raises(ops.Dl3pError):
        L.conv2d_gemm_fwd(x.p, x.ld, None, None, 0, w.p, None, y.p, y.ld, None, None, 1, 3, 3, 1340, 16, 7, 1, 1, 3, 3, 3, 3, stream())
    torch.cuda.synchronize()
    assert torch.equal(y.bits, y.keep)


# ------------------------------------------------------------------------------------------------ data gradient
def launch_dgrad(L, ops, c, g, d, dyp, sb, acc, layout):
    M = c.N * c.H * c.W
    gx = out_plane(M, c.Cin, layout, T(d['xbase']) if acc else None)
    w = Flat(T(d['w']))
    wd = Flat(torch.zeros(c.Cin * c.k * c.k * c.Cout, device=DEV))
    L.conv2d_gemm_dgrad_weights(w.p, wd.p, c.k, c.Cin, c.Cout, stream())
    if sb:
        wdsp = ops.split_bf16x3(wd.t.reshape(c.Cin, c.k * c.k * c.Cout))
        L.conv2d_gemm_bwd_data_sb(dyp.p, dyp.ld, wdsp.data_ptr(), wdsp.shape[2], gx.p, gx.ld, int(acc), *geo_args(c, g))
    else:
        L.conv2d_gemm_bwd_data(dyp.p, dyp.ld, wd.p, gx.p, gx.ld, int(acc), *geo_args(c, g))
    torch.cuda.synchronize()
    assert torch.isnan(wd.buf[wd.t.numel():]).all()
    return gx


def check_unreached(gx, chk, base, what):
    """input pixels no tap reaches: exactly +0, or the base bit for bit"""
    dead = ~chk.reached
    if bool(dead.any()):
        bits = gx.t.view(torch.int32)[dead]
        want = torch.zeros_like(bits) if base is None else base.view(torch.int32)[dead]
        assert torch.equal(bits, want), what + ': a pixel without a tap was written'
    return int(dead.sum())


@pytest.mark.parametrize('c', R.GEMM, ids=lambda c: c.name)
def test_data_gradient_per_element(ops, L, c):
    g, d = R.geo_of(c), R.conv_inputs(c)
    L.opt('conv_sb', 2)
    dyp = plane(T(d['dy']), 'off4')
    chk = R.dgrad_ref(T64(d['dy']), T64(d['w']), g, c.Cin)
    gx = launch_dgrad(L, ops, c, g, d, dyp, False, False, 'ld4')
    gx.intact(c.name)
    chk.verify(gx.t, c.name + ' data gradient')
    dead = check_unreached(gx, chk, None, c.name)
    if c.name in ('s2_k1', 's2_r2'):
        assert dead > 0
    acc = R.dgrad_ref(T64(d['dy']), T64(d['w']), g, c.Cin, base=T64(d['xbase']))
    ga = launch_dgrad(L, ops, c, g, d, dyp, False, True, 'off4')
    ga.intact(c.name + ' accumulate')
    acc.verify(ga.t, c.name + ' data gradient, accumulate')
    check_unreached(ga, acc, T(d['xbase']), c.name + ' accumulate')
    dyp.intact(c.name + ' dy')
    M, K = c.N * c.H * c.W, c.k * c.k * c.Cout
    if R.conv_sb_supported(2, M, K, c.Cin):
        gs = launch_dgrad(L, ops, c, g, d, dyp, True, False, 'contig')
        gs.intact(c.name + ' split')
        esb, e32 = chk.rel(gs.t), chk.rel(gx.t)
        print('%s split data gradient: %.3g of sum|terms| (fp32 route %.3g)' % (c.name, esb, e32))
        assert esb < R.SB_ABS and esb < R.SB_REL * e32 + R.SB_FLOOR, (c.name, esb, e32)
        check_unreached(gs, chk, None, c.name + ' split')


# ------------------------------------------------------------------------------------------------ the address padded taps load from
POISON = [c for c in R.GEMM if c.name in ('map_5x7_span', 'rate_ge_h', 's2_0101_odd', 'sb_m1087', 'sb_k3_c20')]


@pytest.mark.parametrize('c', POISON, ids=lambda c: c.name)
def test_poison_at_the_address_padded_taps_load_from(ops, L, c):
    """NaN in channels 0 .. 3 of pixel (0, 0) of image 0 -- byte offset 0 of the gathered operand, which every padded tap loads and
    must discard AFTER the prologue: only the outputs whose receptive field holds that pixel may be non-finite"""
    g, d = R.geo_of(c), R.conv_inputs(c)
    L.opt('conv_sb', 2)
    pix, ok = R.tap_index(g, DEV)
    M, K = c.N * g.Ho * g.Wo, c.k * c.k * c.Cin
    # forward: output rows of image 0 with an inside tap on pixel 0
    hit = torch.zeros(M, dtype=torch.bool, device=DEV)
    hit[:g.Ho * g.Wo] = (ok & (pix == 0)).any(1)
    x = T(d['x']).clone()
    chk = R.fwd_ref(x.double(), T64(d['w']), g, T64(d['sc']), T64(d['sh']), d['act'], bias=T64(d['bias']))
    x[0, :4] = float('nan')
    xp = plane(x, 'off4')
    def beside(got, ref, mask, sb, e32, what):
        """every element outside `mask`: the fp32 bound, or the split rule against the fp32 route's figure e32; -> this route's figure"""
        got = torch.where(mask[:, None], ref.ref.float(), got)
        if sb:
            e = ref.rel(got)
            assert torch.isfinite(got).all() and e < R.SB_ABS and e < R.SB_REL * e32 + R.SB_FLOOR, (what, e, e32)
            return e
        ref.verify(got, what)
        return ref.rel(got)
    assert 0 < int(hit.sum()) < M
    e32 = None
    for sb in (False, True) if R.conv_sb_supported(0, M, K, c.Cout) else (False,):
        y, _, _ = launch_fwd(L, ops, c, g, d, xp, sb, False, True, 'ld4')
        y.intact(c.name)
        e32 = beside(y.t, chk, hit, sb, e32, c.name + ' forward beside the poison' + ' (split)' * sb)
    # weight gradient: rows k = tap * Cin + (0 .. 3) of the taps through which some output pixel of image 0 reads pixel 0
    tap_hit = (ok & (pix == 0)).any(0)
    k_hit = (tap_hit[:, None] & (torch.arange(c.Cin, device=DEV) < 4)[None]).reshape(-1)
    wchk = R.wgrad_ref(T64(d['x']), T64(d['dy']), g, T64(d['sc']), T64(d['sh']), d['act'])
    dyp = plane(T(d['dy']), 'ld4')
    e32 = None
    for sb in (False, True) if R.conv_sb_supported(4, M, K, c.Cout) else (False,):
        L.opt('conv_sb', 2 if sb else 0)
        L.opt('split_wgrad', 1)
        assert ops.conv2d_gemm_plan_query(4, M, K, c.Cout)[0] == (4 if sb else 0)
        gw = launch_wgrad(L, c, g, d, xp, dyp)[0]
        gw.intact(c.name)
        e32 = beside(gw.t, wchk, k_hit, sb, e32, c.name + ' weight gradient beside the poison' + ' (split)' * sb)
    L.opt('conv_sb', 2)
    # data gradient: the input pixels output pixel 0 of image 0 reaches
    dy = T(d['dy']).clone()
    dchk = R.dgrad_ref(dy.double(), T64(d['w']), g, c.Cin)
    dy[0, :4] = float('nan')
    reach = torch.zeros(c.N * c.H * c.W, dtype=torch.bool, device=DEV)
    reach[pix[0][ok[0]]] = True
    dyp = plane(dy, 'ld4')
    e32 = None
    for sb in (False, True) if R.conv_sb_supported(2, c.N * c.H * c.W, c.k * c.k * c.Cout, c.Cin) else (False,):
        gx = launch_dgrad(L, ops, c, g, d, dyp, sb, False, 'off4')
        gx.intact(c.name)
        e32 = beside(gx.t, dchk, reach, sb, e32, c.name + ' data gradient beside the poison' + ' (split)' * sb)
        assert torch.equal(gx.t.view(torch.int32)[~dchk.reached], torch.zeros_like(gx.t.view(torch.int32)[~dchk.reached]))


# ------------------------------------------------------------------------------------------------ weight gradient
def launch_wgrad(L, c, g, d, xp, dyp, slabs=False, gb=False):
    """-> (gw plane, gb plane or None, rows)"""
    K = c.k * c.k * c.Cin
    need = L.conv2d_gemm_bwd_weight_workspace(c.N, g.Ho, g.Wo, c.Cin, c.Cout, c.k)
    ws = Flat(torch.full((need // 4,), float('nan'), device=DEV))
    gw = out_plane(K, c.Cout, 'contig')
    gbp = out_plane(1, c.Cout, 'contig') if gb else None
    sc, sh = vec(d['sc']), vec(d['sh'])
    rows = ctypes.c_int(-1)
    if slabs:
        L.conv2d_gemm_bwd_weight_slabs(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], dyp.p, dyp.ld, ws.p, need, ctypes.byref(rows),
                                       *geo_args(c, g))
        L.reduce_rows(ws.p, rows.value, K * c.Cout, gw.p, 0, stream())
    else:
        L.conv2d_gemm_bwd_weight(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], dyp.p, dyp.ld, gw.p, gbp.p if gb else None, ws.p, need,
                                 *geo_args(c, g))
    torch.cuda.synchronize()
    assert torch.isnan(ws.buf[need // 4:]).all(), c.name + ': the workspace was overrun'
    return gw, gbp, rows.value


@pytest.mark.parametrize('c', R.WGRAD, ids=lambda c: c.name)
def test_weight_gradient_per_element(ops, L, c):
    g, d = R.geo_of(c), R.conv_inputs(c)
    M, K = c.N * g.Ho * g.Wo, c.k * c.k * c.Cin
    xp, dyp = plane(T(d['x']), 'off4'), plane(T(d['dy']), 'ld4')
    chk = R.wgrad_ref(T64(d['x']), T64(d['dy']), g, T64(d['sc']), T64(d['sh']), d['act'])
    L.opt('conv_sb', 0)
    L.opt('wgrad_tile', c.tile)
    want = c.want if c.sb is None else None
    plan = ops.conv2d_gemm_plan_query(4, M, K, c.Cout)
    assert want is None or plan[:4] == want, (c.name, plan)
    gw, gb, _ = launch_wgrad(L, c, g, d, xp, dyp, gb=True)
    gw.intact(c.name)
    gb.intact(c.name + ' gb')
    chk.verify(gw.t, c.name + ' weight gradient')
    R.colsum_check(dyp.t).verify(gb.t, c.name + ' bias gradient')
    g2, _, rows = launch_wgrad(L, c, g, d, xp, dyp, slabs=True)
    assert rows == plan[3], (c.name, rows, plan)
    assert torch.equal(g2.t.view(torch.int32), gw.t.view(torch.int32)), c.name + ': slabs + reduce_rows differ from the one call'
    if c.sb is not None:
        L.opt('conv_sb', 2)
        L.opt('split_wgrad', 1)
        L.opt('split_wgrad_tile', c.sb)
        plan = ops.conv2d_gemm_plan_query(4, M, K, c.Cout)
        assert plan[:4] == c.want, (c.name, plan)
        gs, gbs, _ = launch_wgrad(L, c, g, d, xp, dyp, gb=True)
        gs.intact(c.name + ' split')
        esb, e32 = chk.rel(gs.t), chk.rel(gw.t)
        print('%s split weight gradient: %.3g of sum|terms| (fp32 route %.3g)' % (c.name, esb, e32))
        assert esb < R.SB_ABS and esb < R.SB_REL * e32 + R.SB_FLOOR, (c.name, esb, e32)
        assert torch.equal(gbs.t.view(torch.int32), gb.t.view(torch.int32))
        g2, _, rows = launch_wgrad(L, c, g, d, xp, dyp, slabs=True)
        assert rows == plan[3] and torch.equal(g2.t.view(torch.int32), gs.t.view(torch.int32)), c.name
    xp.intact(c.name + ' x')
    dyp.intact(c.name + ' dy')


# ------------------------------------------------------------------------------------------------ the stem
def stem_inputs(c):
    r = R.rng_of(c.name)
    Ho, Wo, pt, pl = R.conv_geometry(c.H, c.W, 3, 2, 1, c.pad)
    g = R.Geo(c.N, c.H, c.W, 3, 2, 1, pt, pl, Ho, Wo)
    M = c.N * Ho * Wo
    d = dict(x=R.signed(r, (c.N * c.H * c.W, 3), 0.25, 2.0), w=R.signed(r, (27, c.Cout)), dy=R.signed(r, (M, c.Cout)),
             z=R.signed(r, (M, c.Cout), 0.25, 4.0), sc=r.uniform(0.5, 1.5, c.Cout).astype(F), sh=r.uniform(0.25, 0.75, c.Cout).astype(F),
             mu=r.uniform(-0.5, 0.5, c.Cout).astype(F), inv=r.uniform(0.5, 2.0, c.Cout).astype(F),
             coef=r.uniform(0.25, 1.0, (3, c.Cout)).astype(F))
    d['z'] = R.off_kinks(d['z'], d['sc'], d['sh'], R.RELU6)
    return g, d


def stem_geo(c, g):
    return (c.N, c.H, c.W, c.Cout, g.pt, g.pl, g.Ho, g.Wo, stream())


@pytest.mark.parametrize('c', R.STEM, ids=lambda c: c.name)
def test_stem_per_element(ops, L, c):
    """forward, weight gradient and weight gradient with the folded BatchNorm apply; the packed input (ldx = 3: the interior fast path
    where the case has interior tiles) against an ld = 7 view of the same values (always the general path): the same bits"""
    g, d = stem_inputs(c)
    cus, max_rows = R.machine()
    M, tiles = c.N * g.Ho * g.Wo, c.N * g.Ho * R.stem_segments(g.Wo)
    wk = Flat(torch.cat([T(d['w']), torch.zeros(1, c.Cout, device=DEV)]))
    x64, w64, dy64 = T64(d['x']), T64(d['w']), T64(d['dy'])
    fchk, wchk = R.fwd_ref(x64, w64, g), R.wgrad_ref(x64, dy64, g)
    # the folded apply: dz = c0 (g act'(z sc + sh) - c1 - (z - mu) inv c2), formed as fma(c0, g act', fma(-C, z, D)) with C = c0 inv c2 and
    # D = C mu - c0 c1: at most 6 roundings of |c0 g act'| + |C z| + |C mu| + |c0 c1| (two for C, the products and the difference of
    # D, the two fmas); r = 8 with the second-order terms
    z, sc, sh, mu, inv, (c0, c1, c2) = T64(d['z']), T64(d['sc']), T64(d['sh']), T64(d['mu']), T64(d['inv']), T64(d['coef'])
    u = z * sc + sh
    da = ((u > 0) & (u < 6)).double()
    C = c0 * inv * c2
    dz = c0 * (dy64 * da - c1 - (z - mu) * inv * c2)
    dzmag = (c0 * dy64 * da).abs() + (C * z).abs() + (C * mu).abs() + (c0 * c1).abs()
    P = R.patches(x64, g).reshape(M, 27)
    n = wchk.n
    bchk = R.Bounded(P.t() @ dz, P.abs().t() @ dzmag, n, 8)
    got = {}
    for layout in ('contig', 'ld4'):
        xp = plane(T(d['x']), layout)
        assert xp.ld == (3 if layout == 'contig' else 7)
        rows = ctypes.c_int(-1)
        want_rows = R.stem_grid(tiles, 4, cus, max_rows)
        y, part = out_plane(M, c.Cout, 'off4'), Plane(2 * want_rows, c.Cout, 'contig')
        L.stem_conv_fwd(xp.p, xp.ld, wk.p, y.p, y.ld, part.p, ctypes.byref(rows), *stem_geo(c, g))
        torch.cuda.synchronize()
        assert rows.value == want_rows
        y.intact(c.name)
        fchk.verify(y.t, '%s forward (%s)' % (c.name, layout))
        check_stats(y, part, rows.value, c.name)
        dyp, zp = plane(T(d['dy']), 'ld4'), plane(T(d['z']), 'off4')
        need = L.stem_conv_bwd_weight_workspace(c.N, g.Ho, g.Wo, c.Cout)
        assert need == 4 * 28 * c.Cout * R.stem_grid(tiles, 2, cus, max_rows)
        ws = Flat(torch.full((need // 4,), float('nan'), device=DEV))
        gw = out_plane(28, c.Cout, 'contig')
        L.stem_conv_bwd_weight(xp.p, xp.ld, dyp.p, dyp.ld, gw.p, ws.p, need, *stem_geo(c, g))
        torch.cuda.synchronize()
        gw.intact(c.name)
        wchk.verify(gw.t[:27], '%s weight gradient (%s)' % (c.name, layout))
        assert float(gw.t[27].abs().max()) == 0.0
        gf = out_plane(28, c.Cout, 'contig')
        cf = [vec(d[k]) for k in ('sc', 'sh', 'mu', 'inv', 'coef')]
        L.stem_conv_bwd_weight_slabs_bn(xp.p, xp.ld, dyp.p, dyp.ld, zp.p, zp.ld, cf[0].p, cf[1].p, R.RELU6, cf[2].p, cf[3].p, cf[4].p,
                                        ws.p, need, ctypes.byref(rows), *stem_geo(c, g))
        L.reduce_rows(ws.p, rows.value, 28 * c.Cout, gf.p, 0, stream())
        torch.cuda.synchronize()
        assert torch.isnan(ws.buf[need // 4:]).all()
        gf.intact(c.name)
        bchk.verify(gf.t[:27], '%s weight gradient with the folded apply (%s)' % (c.name, layout))
        xp.intact(c.name + ' x')
        got[layout] = (y.t.clone(), gw.t.clone(), gf.t.clone())
    for a, b in zip(got['contig'], got['ld4']):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), c.name + ': the packed launch and the view differ'


# ------------------------------------------------------------------------------------------------ conv.hip
@pytest.mark.parametrize('c', R.DIRECT, ids=lambda c: c.name)
def test_direct_kernels_and_patch_matrix_per_element(ops, L, c):
    g, d = R.geo_of(c), R.conv_inputs(c)
    M, K = c.N * g.Ho * g.Wo, c.k * c.k * c.Cin
    xp, dyp, w = plane(T(d['x']), 'ld4'), plane(T(d['dy']), 'off4'), Flat(T(d['w']))
    sc, sh = vec(d['sc']), vec(d['sh'])
    x64, w64, dy64 = T64(d['x']), T64(d['w']), T64(d['dy'])
    pro = (T64(d['sc']), T64(d['sh']), d['act'])
    # forward with statistics
    rows = ctypes.c_int(-1)
    y, part = out_plane(M, c.Cout, 'off4'), torch.full((2 * 2048 * c.Cout,), float('nan'), device=DEV)
    L.conv2d_fwd(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], w.p, y.p, y.ld, part.data_ptr(), ctypes.byref(rows), *geo_args(c, g))
    torch.cuda.synchronize()
    y.intact(c.name)
    R.fwd_ref(x64, w64, g, *pro).verify(y.t, c.name + ' forward')
    p = part[:rows.value * 2 * c.Cout].double().reshape(rows.value, 2, c.Cout)
    s1, s2 = R.stat_check(y.t, rows.value)
    s1.verify(p[:, 0].sum(0), c.name + ' sum y')
    s2.verify(p[:, 1].sum(0), c.name + ' sum y^2')
    assert torch.isnan(part[rows.value * 2 * c.Cout:]).all()
    # weight gradient: ceil(K / 32) launches into one gw
    need = L.conv2d_bwd_weight_workspace(c.N, g.Ho, g.Wo, c.Cin, c.Cout, c.k)
    ws, gw = Flat(torch.full((need // 4,), float('nan'), device=DEV)), out_plane(K, c.Cout, 'contig')
    L.conv2d_bwd_weight(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], dyp.p, dyp.ld, gw.p, ws.p, need, *geo_args(c, g))
    torch.cuda.synchronize()
    gw.intact(c.name)
    assert torch.isnan(ws.buf[need // 4:]).all()
    R.wgrad_ref(x64, dy64, g, *pro).verify(gw.t, c.name + ' weight gradient')
    # data gradient, plain and onto a base
    for acc in (False, True):
        gx = out_plane(c.N * c.H * c.W, c.Cin, 'ld4' if c.Cin % 4 == 0 else 'contig', T(d['xbase']) if acc else None)
        L.conv2d_bwd_data(dyp.p, dyp.ld, w.p, gx.p, gx.ld, int(acc), *geo_args(c, g))
        torch.cuda.synchronize()
        gx.intact(c.name)
        chk = R.dgrad_ref(dy64, w64, g, c.Cin, base=T64(d['xbase']) if acc else None)
        chk.verify(gx.t, c.name + ' data gradient')
        check_unreached(gx, chk, T(d['xbase']) if acc else None, c.name)
    # the patch matrix: the prologue's bits, zeros outside the image and in the pad columns
    kp = R.ld_col(K)
    col = out_plane(M, kp, 'contig')
    L.im2col(xp.p, xp.ld, ptr(sc), ptr(sh), d['act'], col.p, kp, c.N, c.H, c.W, c.Cin, c.k, c.s, c.r, g.pt, g.pl, g.Ho, g.Wo, stream())
    torch.cuda.synchronize()
    col.intact(c.name + ' patch matrix')
    want = np.zeros((M, kp), F)
    want[:, :K] = R.patches32(R.pro32(d['x'], d['sc'], d['sh'], d['act']), g)
    assert torch.equal(col.t.view(torch.int32), T(want).view(torch.int32)), c.name + ': patch matrix'
    if c.Cin % 4 == 0:
        # col2im of a gradient of the patch matrix (NaN in its pad columns: they are never read)
        r = R.rng_of(c.name + 'col')
        gc = np.full((M, kp), np.nan, F)
        gc[:, :K] = R.signed(r, (M, K))
        gcp = plane(T(gc), 'contig')
        pix, ok = R.tap_index(g, DEV)
        G = T64(gc[:, :K]).reshape(c.N, g.Ho * g.Wo, c.k * c.k, c.Cin)
        dst = (torch.arange(c.N, device=DEV)[:, None, None] * (c.H * c.W) + pix[None]).reshape(-1)
        okf = ok[None].expand(c.N, -1, -1).reshape(-1)
        for acc in (False, True):
            base = T64(d['xbase']) if acc else torch.zeros(c.N * c.H * c.W, c.Cin, dtype=torch.float64, device=DEV)
            ref, mag, cnt = base.clone(), base.abs(), torch.zeros(c.N * c.H * c.W, dtype=torch.float64, device=DEV)
            ref.index_add_(0, dst[okf], G.reshape(-1, c.Cin)[okf])
            mag.index_add_(0, dst[okf], G.reshape(-1, c.Cin)[okf].abs())
            cnt.index_add_(0, dst[okf], torch.ones_like(dst[okf], dtype=torch.float64))
            gx = out_plane(c.N * c.H * c.W, c.Cin, 'off4', T(d['xbase']) if acc else None)
            L.col2im(gcp.p, kp, gx.p, gx.ld, int(acc), c.N, c.H, c.W, c.Cin, c.k, c.s, c.r, g.pt, g.pl, g.Ho, g.Wo, stream())
            torch.cuda.synchronize()
            gx.intact(c.name + ' col2im')
            chk = R.Bounded(ref, mag, cnt[:, None] + acc, 0)
            chk.reached = cnt > 0
            chk.verify(gx.t, c.name + ' col2im')
            dead = check_unreached(gx, chk, T(d['xbase']) if acc else None, c.name + ' col2im')
            assert dead > 0 or c.r == 1
