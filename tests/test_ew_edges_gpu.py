"""The fp32 BatchNorm / elementwise kernels (bn_elementwise.hip), the window pools (pool.hip) and the bilinear resize
(resize_head.hip) at every lane-plan, row-loop and dispatch edge, against float64, per element.

Every case runs an entry point through ops.lib() on operands that sit inside buffers of their own (ew_rules.Plane): canary bit
patterns (a NaN with a payload, +Inf, -Inf) fill three rows past the last row and, for the 'ld4' (row stride C + 4) and 'off4' (base
4 floats in, row stride C + 8) layouts, the channels beside the view.  Every operand of a launch has a DIFFERENT layout, so a swapped
stride cannot go unseen; the canaries of every output must come back bit-identical, and a canary read from an input shows up as a
non-finite value in the comparison.  The references, the bounds (k fp32 roundings of the magnitudes of the terms that formed the
element, no tensor-scale term) and the near-kink rule are in tests/ew_rules.py; tests/test_ew_rules_cpu.py shows without a device
that a correct fp32 evaluation fits them.

One finding is recorded in the cases themselves: 33 -> 65 (ew_rules.RESIZE_FWD_STRIP) is one column short of the strip path
(W >= 2 w), so it runs the pixel kernel at two 256-channel slabs; 33 -> 66 sits on the switch and takes resize_fwd_seg_kernel<8>."""
import ctypes

import numpy as np
import pytest
import torch

import ew_rules as R
from oracle import np_ops as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32


def _s():
    return torch.cuda.current_stream().cuda_stream


def T(i):
    return {k: R.D(v, DEV) for k, v in i.items() if isinstance(v, np.ndarray)}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def vecs(i, o):
    """the per-channel operands of a case, each in a buffer with NaN behind it; None where the case passes a null pointer"""
    return {k: (R.vec(i[k]) if o[k] is not None else None) for k in ('sc', 'sh', 'rsc', 'rsh', 'mu', 'inv', 'coef')}


def step5():
    return torch.tensor([5], dtype=torch.int64, device=DEV)


def drop_mask(L, M, C, step):
    m = torch.empty((M, C), dtype=torch.float32, device=DEV)
    L.dropout_mask(float(R.RATE), R.SEED, step.data_ptr(), m.data_ptr(), M, C, _s())
    return m


class Worst:
    """the worst err / bound of every op, printed before the test ends (-s shows it)"""

    def __init__(self):
        self.w = {}

    def __call__(self, name, chk, got, what):
        self.w[name] = max(self.w.get(name, 0.0), chk.worst(got))
        chk.verify(got, name + ' ' + what)

    def show(self, title):
        print('\n%s: worst err / bound  %s' % (title, '  '.join('%s %.3f' % kv for kv in sorted(self.w.items()))))


# ----------------------------------------------------------------------------------------- 1. lane-plan walkers
def _lane_case(L, case, worst):
    C, M = case['C'], case['M']
    la, lb, lc = case['lay']
    i = R.lane_inputs(C, M)
    t = T(i)
    o = R.opts_of(case, i, DEV)
    v = vecs(i, o)
    p = R.ptr
    act, ract = case['act'], case['ract']
    what = 'C=%d M=%d act=%d nulls=%d lay=%s' % (C, M, act, case['nulls'], case['lay'])
    assert R.lane_kink_shares(t, o) <= R.KINK_SHARE_MAX, what
    G, Z, X, RR = R.plane(i['g'], la), R.plane(i['z'], lb), R.plane(i['x'], la), R.plane(i['r'], lb)
    s = _s()

    # bn_bwd_reduce: partial rows [rows][2][C]; everything past them stays NaN
    part = torch.full((R.MAX_STAT_ROWS * 2 * C,), float('nan'), dtype=torch.float32, device=DEV)
    rows = ctypes.c_int(0)
    L.bn_bwd_reduce(G.p, G.ld, Z.p, Z.ld, p(v['sc']), p(v['sh']), act, p(v['mu']), p(v['inv']), part.data_ptr(),
                    ctypes.byref(rows), M, C, s)
    rows = rows.value
    assert 0 < rows <= R.MAX_STAT_ROWS and rows == R.ew_nbx(M, C, R.MAX_STAT_ROWS), (what, rows)
    assert bool(torch.isnan(part[rows * 2 * C:]).all()), 'bn_bwd_reduce wrote past its %d rows: %s' % (rows, what)
    worst('bn_bwd_reduce', R.ref_bn_bwd_reduce(t, o, rows), part[:rows * 2 * C].double().reshape(rows, 2, C).sum(0), what)

    N, HW = R.split_rows(M)
    GP = R.plane(i['gp'], lb)
    for acc in (0, 1):
        base = i['old'] if acc else None
        # bn_bwd_apply
        Dz = R.out_plane(M, C, lc, base)
        L.bn_bwd_apply(G.p, G.ld, Z.p, Z.ld, p(v['sc']), p(v['sh']), act, p(v['mu']), p(v['inv']), p(v['coef']), Dz.p, Dz.ld, acc,
                       M, C, s)
        worst('bn_bwd_apply', R.ref_bn_bwd_apply(t, o, acc), Dz.t, what + ' acc=%d' % acc)
        Dz.intact('bn_bwd_apply ' + what)
        # scale_mask_bwd without dropout: a copy / an add
        Gx = R.out_plane(M, C, lc, base)
        L.scale_mask_bwd(G.p, G.ld, 0.0, R.SEED, None, Gx.p, Gx.ld, acc, M, C, s)
        worst('scale_mask_bwd', R.ref_scale_mask_bwd(t, acc), Gx.t, what + ' acc=%d' % acc)
        Gx.intact('scale_mask_bwd ' + what)
        # global_avgpool_bwd
        Gp = R.out_plane(M, C, lc, base)
        L.global_avgpool_bwd(GP.p, GP.ld, Gp.p, Gp.ld, acc, N, HW, C, s)
        worst('global_avgpool_bwd', R.ref_gap_bwd(t, N, HW, acc), Gp.t, what + ' acc=%d' % acc)
        Gp.intact('global_avgpool_bwd ' + what)
        # affine_act, without (acc = 0) and with the residual operand (its own coefficients, activation and stride)
        Y = R.out_plane(M, C, lc)
        if acc:
            L.affine_act(X.p, X.ld, p(v['sc']), p(v['sh']), act, RR.p, RR.ld, p(v['rsc']), p(v['rsh']), ract, 0.0, 0, None, Y.p, Y.ld,
                         M, C, s)
        else:
            L.affine_act(X.p, X.ld, p(v['sc']), p(v['sh']), act, None, 0, None, None, R.NONE, 0.0, 0, None, Y.p, Y.ld, M, C, s)
        worst('affine_act', R.ref_affine_act(t, o, bool(acc)), Y.t, what + ' residual=%d' % acc)
        Y.intact('affine_act ' + what)


@pytest.mark.parametrize('group', [0, 1, 2, 3])
def test_lane_plan_walkers(ops, group):
    """bn_bwd_reduce, bn_bwd_apply, affine_act, scale_mask_bwd and global_avgpool_bwd at C in ew_rules.CS (every class of pick_lanes)
    and M in {1, px - 1, px, px + 1, (1024 // nslab) px + 3}; the widths are dealt over four pytest cases"""
    worst = Worst()
    for case in R.lane_cases():
        if R.CS.index(case['C']) % 4 == group:
            _lane_case(ops.lib(), case, worst)
    worst.show('lane walkers %d' % group)


def test_dropout_keeps_the_elements_of_the_dense_mask(ops):
    """affine_act and scale_mask_bwd with rate 0.3 on strided views keep exactly the elements dl3p_dropout_mask keeps on the dense
    (M, C) tensor -- the mask index is m C + c, not m ld + c -- and scale them by 1 / (1 - rate) within 2 U"""
    L, s, p = ops.lib(), _s(), R.ptr
    worst = Worst()
    for C in (12, 120, 672, 1028):
        M = R.pick_lanes(C)[1] + 1
        i = R.lane_inputs(C, M)
        t = T(i)
        step = step5()
        keep = drop_mask(L, M, C, step)
        assert 0 < float(keep.mean()) < 1
        keepd = keep.double()
        what = 'C=%d M=%d' % (C, M)
        X, RR, G = R.plane(i['x'], 'ld4'), R.plane(i['r'], 'contig'), R.plane(i['g'], 'ld4')
        # act none, no coefficients: a kept element is x * keep_scale, one rounding
        o = R.opts_of(dict(act=R.NONE, ract=R.RELU6, nulls=1), i, DEV)
        Y = R.out_plane(M, C, 'off4')
        L.affine_act(X.p, X.ld, None, None, R.NONE, None, 0, None, None, R.NONE, R.RATE, R.SEED, step.data_ptr(), Y.p, Y.ld, M, C, s)
        assert torch.equal(Y.t != 0, (keep != 0) & (t['x'] != 0).to(keep.device)), 'affine_act: not the dense mask ' + what
        chk = R.ref_affine_act(t, o, False, R.RATE, keepd)
        assert float((chk.bound / chk.ref.abs().clamp_min(1e-300)).max()) <= 2 * R.U * (1 + 1e-9)
        worst('affine_act dropout', chk, Y.t, what)
        Y.intact('affine_act dropout ' + what)
        # h-swish prologue, dropout, then the residual
        o = R.opts_of(dict(act=R.HSWISH, ract=R.RELU6, nulls=0), i, DEV)
        v = vecs(i, o)
        Y = R.out_plane(M, C, 'off4')
        L.affine_act(X.p, X.ld, p(v['sc']), p(v['sh']), R.HSWISH, RR.p, RR.ld, p(v['rsc']), p(v['rsh']), R.RELU6, R.RATE, R.SEED,
                     step.data_ptr(), Y.p, Y.ld, M, C, s)
        worst('affine_act dropout + residual', R.ref_affine_act(t, o, True, R.RATE, keepd), Y.t, what)
        Y.intact('affine_act dropout + residual ' + what)
        for acc in (0, 1):
            Gx = R.out_plane(M, C, 'off4', i['old'] if acc else None)
            L.scale_mask_bwd(G.p, G.ld, R.RATE, R.SEED, step.data_ptr(), Gx.p, Gx.ld, acc, M, C, s)
            if not acc:
                assert torch.equal(Gx.t != 0, (keep != 0) & (t['g'] != 0)), 'scale_mask_bwd: not the dense mask ' + what
            worst('scale_mask_bwd dropout', R.ref_scale_mask_bwd(t, acc, R.RATE, keepd), Gx.t, what + ' acc=%d' % acc)
            Gx.intact('scale_mask_bwd dropout ' + what)
    worst.show('dropout')


def test_planted_kinks_follow_the_tf_convention(ops):
    """scale = 1, shift = 0 and z exactly at every kink: forward and gradient equal oracle.np_ops.act_fwd / act_bwd strictly (the
    inner derivative is 0 AT a kink)"""
    L, s = ops.lib(), _s()
    C, M = 12, 5
    one, zero = R.vec(np.ones(C, F)), R.vec(np.zeros(C, F))
    for act in R.ACTS:
        z = np.random.default_rng(act).standard_normal((M, C)).astype(F)
        kinks = R.KINKS[act]
        for j, k in enumerate(kinks):
            z[:3, 3 * j:3 * j + 3] = k
        g = (np.random.default_rng(9).standard_normal((M, C)) + 3).astype(F)
        planted = np.isin(z, kinks)
        Z, G = R.plane(z, 'ld4'), R.plane(g, 'off4')
        Y = R.out_plane(M, C, 'contig')
        L.affine_act(Z.p, Z.ld, one.p, zero.p, act, None, 0, None, None, R.NONE, 0.0, 0, None, Y.p, Y.ld, M, C, s)
        want = O.act_fwd(z.astype(np.float64), act)
        got = Y.t.double().cpu().numpy()
        assert np.array_equal(got[planted], want[planted]), 'forward at the kinks of act %d' % act
        Dz = R.out_plane(M, C, 'contig')
        L.bn_bwd_apply(G.p, G.ld, Z.p, Z.ld, one.p, zero.p, act, None, None, None, Dz.p, Dz.ld, 0, M, C, s)
        want = O.act_bwd(z.astype(np.float64), g.astype(np.float64), act)
        got = Dz.t.double().cpu().numpy()
        assert np.array_equal(got[planted], want[planted]), 'gradient at the kinks of act %d' % act
        assert planted.sum() == 9 * len(kinks)
        Y.intact('affine_act')
        Dz.intact('bn_bwd_apply')


# ----------------------------------------------------------------------------------------- 2. finalize and row reducers
def _row_buffer(x, slack_rows, width):
    """the rows followed by `slack_rows` NaN rows (no row loop may read them; a loop that ran one stage too far would stay inside)"""
    buf = torch.full(((x.shape[0] + slack_rows) * width,), float('nan'), dtype=torch.float32, device=DEV)
    buf[:x.size] = dev(x).reshape(-1)
    return buf


def test_finalize_row_loops(ops):
    """bn_finalize and bn_bwd_finalize on hand-made partial rows across the 512 / 128 / tail stages of reduce2_rows, with the `sums`
    path, the three moving-average rules and frozen mode; C = 4, 20, 36 leave channels of a 16-channel workgroup unused"""
    L, s = ops.lib(), _s()
    worst = Worst()
    for rows in R.FIN_ROWS:
        for C in R.FIN_CS:
            i = R.fin_inputs(rows, C)
            p64 = i['part'].astype(np.float64)
            part = _row_buffer(i['part'], 66, 2 * C)
            sums = torch.cat([dev(i['sums'].reshape(-1)), torch.full((8,), float('nan'), dtype=torch.float64, device=DEV)])
            ga, be, inv = R.vec(i['gamma']), R.vec(i['beta']), R.vec(np.random.default_rng(rows).uniform(0.5, 1.5, C).astype(F))
            sabs, ssabs = R.D(np.abs(p64[:, 0]).sum(0), DEV), R.D(np.abs(p64[:, 1]).sum(0), DEV)
            for use_sums in (False, True):
                if use_sums and rows not in (1, 65, 640):
                    continue
                se, sse = i['sums'] if use_sums else (R.exact_sum(i['part'][:, 0]), R.exact_sum(i['part'][:, 1]))
                se, sse = R.D(se, DEV), R.D(sse, DEV)
                r1 = 0 if use_sums else rows
                for um in (0, 1, 2):
                    what = 'rows=%d C=%d sums=%d update_moving=%d' % (rows, C, use_sums, um)
                    out = {k: R.out_plane(1, C, 'contig', b) for k, b in (('scale', None), ('shift', None), ('save_mean', None),
                                                                         ('save_invstd', None), ('moving_mean', i['mm']),
                                                                         ('moving_var', i['mv']))}
                    L.bn_finalize(part.data_ptr(), rows, sums.data_ptr() if use_sums else None, C, i['count'], ga.p, be.p, R.EPS,
                                  R.MOM, out['moving_mean'].p, out['moving_var'].p, um, out['scale'].p, out['shift'].p,
                                  out['save_mean'].p, out['save_invstd'].p, s)
                    ref = R.ref_bn_finalize(se, sse, sabs, ssabs, r1, i['count'], R.D(i['gamma'], DEV), R.D(i['beta'], DEV),
                                            R.D(i['mm'], DEV), R.D(i['mv'], DEV), um)
                    for k in ref:
                        worst('bn_finalize ' + k, ref[k], out[k].t.reshape(-1), what)
                    if not um:
                        assert torch.equal(out['moving_mean'].t.reshape(-1).cpu(), torch.from_numpy(i['mm'])), what
                    for k in out:
                        out[k].intact('bn_finalize %s %s' % (k, what))
                # bn_bwd_finalize: the same rows as [sum dyy, sum dyy * xhat]
                what = 'rows=%d C=%d sums=%d' % (rows, C, use_sums)
                dg, db = R.out_plane(1, C, 'contig'), R.out_plane(1, C, 'contig')
                coef = R.out_plane(3, C, 'contig')
                L.bn_bwd_finalize(part.data_ptr(), rows, sums.data_ptr() if use_sums else None, C, i['count'], ga.p, inv.p, None, 0,
                                  dg.p, db.p, coef.p, s)
                ref = R.ref_bn_bwd_finalize(se, sse, sabs, ssabs, r1, i['count'], R.D(i['gamma'], DEV), inv.buf[:C].double())
                got = {'dbeta': db.t[0], 'dgamma': dg.t[0], 'coef0': coef.t[0], 'coef1': coef.t[1], 'coef2': coef.t[2]}
                for k in ref:
                    worst('bn_bwd_finalize ' + k, ref[k], got[k], what)
                for pl in (dg, db, coef):
                    pl.intact('bn_bwd_finalize ' + what)
            # frozen: coef = [scale, 0, 0], no statistics read (null rows), dgamma / dbeta untouched
            dg, coef = R.out_plane(1, C, 'contig'), R.out_plane(3, C, 'contig')
            L.bn_bwd_finalize(None, 0, None, C, i['count'], None, None, ga.p, 1, dg.p, dg.p, coef.p, s)
            want = torch.cat([ga.buf[:C], torch.zeros(2 * C, device=DEV)]).reshape(3, C)
            assert torch.equal(coef.t, want), 'frozen bn_bwd_finalize rows=%d C=%d' % (rows, C)
            coef.intact('frozen')
            assert torch.equal(dg.bits, dg.keep), 'frozen bn_bwd_finalize wrote dgamma / dbeta'
    worst.show('finalize')


def test_reduce_partials_row_loop(ops):
    """bn_reduce_partials (double sums for SyncBN) across its 128-row pair loop and tail: within rows * 2^-53 * sum|x| of the exact sum"""
    L, s = ops.lib(), _s()
    w = 0.0
    for rows in R.PART_ROWS:
        for C2 in R.PART_C2:
            x = R.row_inputs(rows + C2, rows, C2)
            part = _row_buffer(x, 66, C2)
            out = torch.full((C2 + 8,), float('nan'), dtype=torch.float64, device=DEV)
            L.bn_reduce_partials(part.data_ptr(), rows, C2, out.data_ptr(), s)
            assert bool(torch.isnan(out[C2:]).all())
            err = np.abs(out[:C2].cpu().numpy() - R.exact_sum(x))
            bound = rows * R.UD * np.abs(x.astype(np.float64)).sum(0)
            w = max(w, float((err / bound).max()))
            assert (err <= bound).all(), 'bn_reduce_partials rows=%d C2=%d: worst err / bound %.3g' % (rows, C2, (err / bound).max())
    print('\nbn_reduce_partials: worst err / bound %.3f' % w)


def test_reduce_rows_both_variants(ops):
    """dl3p_reduce_rows: the wide variant (reduce_rows_kernel<64, 4>: rows <= 16 or n >= 65536) and the tall one (<16, 64>) across
    their 4 RL unroll and tail, plain and accumulating, canaries behind element n"""
    L, s = ops.lib(), _s()
    worst = Worst()
    for variant, cases in ((0, R.RR_WIDE), (1, R.RR_TALL)):
        for rows, n in cases:
            assert L.reduce_rows_variant(rows, n) == variant, (rows, n)
            x = R.row_inputs(rows * 131 + n, rows, n)
            part = _row_buffer(x, 3, n)
            old = R.row_inputs(7, 1, n)
            for acc in (0, 1):
                out = R.out_plane(1, n, 'contig', old if acc else None)
                L.reduce_rows(part.data_ptr(), rows, n, out.p, acc, s)
                worst('reduce_rows variant %d' % variant, R.ref_reduce_rows(x, R.D(old[0], DEV) if acc else None, DEV), out.t[0],
                      'rows=%d n=%d acc=%d' % (rows, n, acc))
                out.intact('reduce_rows rows=%d n=%d' % (rows, n))
    worst.show('reduce_rows')


# ----------------------------------------------------------------------------------------- 3. per-image reductions
def _workspace(L, N, HW, C):
    """tickets zero, partial rows NaN: every float a launch reads it must have written"""
    nbytes = L.pool_workspace(N, HW, C)
    assert nbytes == 4 * R.pool_workspace_floats(N, HW, C)
    ws = torch.full((nbytes // 4 + 8,), float('nan'), dtype=torch.float32, device=DEV)
    nt = R.pool_plan(N, HW, C, True)['ticket_floats']
    ws[:nt] = 0
    return ws, nbytes, nt


@pytest.mark.parametrize('chunked', [False, True])
def test_per_image_reductions(ops, chunked):
    """global_avgpool_fwd, scale_bcast_fwd and scale_bcast_bwd on the whole-image plan (no workspace) and the chunked one, at the
    edges of the eight-deep and two-deep unrolls, with an output stride != C; the workspace's tickets return to zero and three
    calls on one workspace agree bit for bit"""
    L, s, p = ops.lib(), _s(), R.ptr
    worst = Worst()
    j = 0
    for C in R.POOL_CS:
        for N in (1, 3):
            for HW in R.pool_hws(C, chunked):
                j += 1
                act = R.ACTS[j % 5]
                i = R.pool_inputs(N, HW, C)
                t = T(i)
                o = R.opts_of(dict(act=act, ract=R.NONE, nulls=j % 2), i, DEV)
                v = vecs(i, o)
                lay = R.LAYOUTS[j % 3:] + R.LAYOUTS[:j % 3]
                what = 'C=%d N=%d HW=%d act=%d chunked=%d' % (C, N, HW, act, chunked)
                assert R.kink_share(*R.pro64(t['x'], o['sc'], o['sh'])[:2], act) <= R.KINK_SHARE_MAX, what
                X, G, S = R.plane(i['x'], lay[0]), R.plane(i['g'], lay[1]), R.plane(i['s'], lay[2])
                ws, nbytes, nt = _workspace(L, N, HW, C) if chunked else (None, 0, 0)
                wp = ws.data_ptr() if chunked else None
                nck = R.pool_plan(N, HW, C, True)['nchunk'] if chunked else 1
                nck_fwd = nck if R.gap_fwd_chunks(N, HW, C, chunked) else 1
                ys = []
                for rep in range(3):
                    Y = R.out_plane(N, C, lay[1])
                    L.global_avgpool_fwd(X.p, X.ld, p(v['sc']), p(v['sh']), act, Y.p, Y.ld, 0.75, N, HW, C, wp, nbytes, s)
                    Y.intact('global_avgpool_fwd ' + what)
                    GX, GS = R.out_plane(N * HW, C, lay[2], i['old'] if rep == 1 else None), R.out_plane(N, C, lay[0])
                    L.scale_bcast_bwd(G.p, G.ld, X.p, X.ld, p(v['sc']), p(v['sh']), act, S.p, S.ld, R.HSIGMOID, GX.p, GX.ld,
                                      int(rep == 1), GS.p, GS.ld, N, HW, C, wp, nbytes, s)
                    GX.intact('scale_bcast_bwd gx ' + what)
                    GS.intact('scale_bcast_bwd gs ' + what)
                    if chunked:
                        assert int(ws[:nt].view(torch.int32).abs().sum()) == 0, 'tickets not back to zero: ' + what
                    cx, cs = R.ref_scale_bcast_bwd(t, o, N, HW, R.HSIGMOID, int(rep == 1), nck)
                    worst('scale_bcast_bwd gx', cx, GX.t, what)
                    ys.append((Y.t.clone(), GS.t.clone()))
                worst('global_avgpool_fwd', R.ref_gap_fwd(t, o, N, HW, 0.75, nck_fwd), ys[0][0], what)
                worst('scale_bcast_bwd gs', cs, ys[0][1], what)
                for y, gs in ys[1:]:
                    assert torch.equal(y, ys[0][0]) and torch.equal(gs, ys[0][1]), 'calls on one workspace differ: ' + what
                if chunked:                      # (scale_bcast_fwd has one plan)
                    Y = R.out_plane(N * HW, C, lay[1])
                    L.scale_bcast_fwd(X.p, X.ld, p(v['sc']), p(v['sh']), act, S.p, S.ld, R.HSIGMOID, Y.p, Y.ld, N, HW, C, s)
                    worst('scale_bcast_fwd', R.ref_scale_bcast_fwd(t, o, N, HW, R.HSIGMOID), Y.t, what)
                    Y.intact('scale_bcast_fwd ' + what)
    worst.show('per-image reductions chunked=%d' % chunked)


# ----------------------------------------------------------------------------------------- 4. pool.hip
def test_maxpool_windows(ops):
    """maxpool2d forward BIT-exact against the fp32 prologue followed by a float64 maximum; backward with and without the recorded
    argmax, plain and accumulating, compared wherever the ReLU is alive; three different strides for x, y and dy"""
    L, s = ops.lib(), _s()
    for k, st, pad in R.MAXPOOL_CASES:
        for C in (4, 12):
            N, H, W = 2, 9, 11
            Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
            i = R.pool_inputs2d(N, H, W, C, Ho, Wo, 10 * k + st + C)
            a, y, arg, gx, gm, cnt = R.ref_maxpool(i, R.RELU, k, st, pad, Ho, Wo)
            what = 'k=%d s=%d pad=%d C=%d' % (k, st, pad, C)
            X, DY = R.plane(i['x'], 'ld4'), R.plane(i['dy'], 'contig')
            sc, sh = R.vec(i['sc']), R.vec(i['sh'])
            Y = R.out_plane(N * Ho * Wo, C, 'off4')
            rec = torch.full((N * Ho * Wo * C + 16,), 0xEE, dtype=torch.uint8, device=DEV)
            L.maxpool2d_fwd(X.p, X.ld, sc.p, sh.p, R.RELU, Y.p, Y.ld, rec.data_ptr(), N, H, W, C, k, st, pad, pad, Ho, Wo, s)
            assert np.array_equal(Y.t.cpu().numpy().reshape(y.shape), y.astype(F)), 'maxpool forward not bit-exact: ' + what
            assert np.array_equal(rec[:-16].cpu().numpy().reshape(arg.shape), arg), 'recorded first maximum: ' + what
            assert bool((rec[-16:] == 0xEE).all())
            Y.intact('maxpool fwd ' + what)
            Y2 = R.out_plane(N * Ho * Wo, C, 'off4')
            L.maxpool2d_fwd(X.p, X.ld, sc.p, sh.p, R.RELU, Y2.p, Y2.ld, None, N, H, W, C, k, st, pad, pad, Ho, Wo, s)
            assert torch.equal(Y2.bits, Y.bits), 'maxpool forward without argmax: ' + what
            alive = dev(a > 0).reshape(-1, C)
            for use_rec in (False, True):
                for acc in (0, 1):
                    GX = R.out_plane(N * H * W, C, 'off4', i['old'] if acc else None)
                    L.maxpool2d_bwd(X.p, X.ld, sc.p, sh.p, R.RELU, DY.p, DY.ld, rec.data_ptr() if use_rec else None, GX.p, GX.ld, acc,
                                    N, H, W, C, k, st, pad, pad, Ho, Wo, s)
                    ref = R.D(gx, DEV).reshape(-1, C) + (R.D(i['old'], DEV).reshape(-1, C) if acc else 0)
                    mag = R.D(gm, DEV).reshape(-1, C) + (R.D(i['old'], DEV).reshape(-1, C).abs() if acc else 0)
                    bound = (R.D(cnt, DEV).reshape(-1, C) + acc + 1) * R.U * mag           # one add per window (+ the accumulate)
                    got = GX.t.double()
                    bad = alive & ~((got - ref).abs() <= bound)
                    assert not bool(bad.any()), 'maxpool backward (argmax=%d acc=%d) %s: %d elements' % (use_rec, acc, what, int(bad.sum()))
                    assert bool(torch.isfinite(got).all())
                    GX.intact('maxpool bwd ' + what)


def test_avgpool_windows(ops):
    """avgpool2d with (k, stride) in {(2, 2), (3, 2), (3, 3), (2, 3)} on maps where H - k is no multiple of the stride: rows and
    columns no window covers get exactly 0 in the backward; strided views, accumulate"""
    L, s = ops.lib(), _s()
    for k, st, H, W in R.AVGPOOL_CASES:
        N, C = 2, 12
        Ho, Wo = (H - k) // st + 1, (W - k) // st + 1
        i = R.pool_inputs2d(N, H, W, C, Ho, Wo, 100 * k + st)
        y, yb, gx, gm, cnt = R.ref_avgpool(i, R.HSWISH, k, st, Ho, Wo)
        what = 'k=%d s=%d %dx%d' % (k, st, H, W)
        X, DY = R.plane(i['x'], 'off4'), R.plane(i['dy'], 'ld4')
        sc, sh = R.vec(i['sc']), R.vec(i['sh'])
        Y = R.out_plane(N * Ho * Wo, C, 'ld4')
        L.avgpool2d_fwd(X.p, X.ld, sc.p, sh.p, R.HSWISH, Y.p, Y.ld, N, H, W, C, k, st, Ho, Wo, s)
        R.Check(R.D(y, DEV).reshape(-1, C), R.D(yb, DEV).reshape(-1, C)).verify(Y.t, 'avgpool fwd ' + what)
        Y.intact('avgpool fwd ' + what)
        for acc in (0, 1):
            GX = R.out_plane(N * H * W, C, 'contig', i['old'] if acc else None)
            L.avgpool2d_bwd(DY.p, DY.ld, GX.p, GX.ld, acc, N, H, W, C, k, st, Ho, Wo, s)
            old = R.D(i['old'], DEV).reshape(-1, C) if acc else 0
            ref = R.D(gx, DEV).reshape(-1, C) + old
            mag = R.D(gm, DEV).reshape(-1, C) + (old.abs() if acc else 0)
            # one add per covering window, the division (+ the accumulate), plus one
            R.Check(ref, (R.D(cnt, DEV).reshape(-1, C) + 2 + acc) * R.U * mag).verify(GX.t, 'avgpool bwd acc=%d %s' % (acc, what))
            if not acc:
                un = dev(cnt == 0).reshape(-1, C)
                assert bool(un.any()) and bool((GX.t[un] == 0).all()), 'uncovered rows / columns not exactly 0: ' + what
            GX.intact('avgpool bwd ' + what)


# ----------------------------------------------------------------------------------------- 5. bilinear resize
def test_resize_forward_paths(ops):
    """resize_bilinear_fwd on the strip kernels (SEG 16 and SEG 8, one and two 256-channel slabs, both sides of 15 w / W <= 3 and of
    W >= 2 w, a map that shrinks in y) and the pixel kernel, on strided views: every output within the two-level lerp's bound"""
    L, s = ops.lib(), _s()
    w8 = 0.0
    for N, h, w, C, H, W, lx, ly in R.RESIZE_FWD_STRIP + R.RESIZE_FWD_PIXEL:
        x = np.random.default_rng(h * 100 + W + C).standard_normal((N, h, w, C)).astype(F)
        ref, bound = R.ref_resize_fwd(x, H, W)
        what = '%dx%d -> %dx%d C=%d (%s)' % (h, w, H, W, C, R.resize_fwd_path(w, W, C))
        X, Y = R.plane(x, lx), R.out_plane(N * H * W, C, ly)
        L.resize_bilinear_fwd(X.p, X.ld, Y.p, Y.ld, N, h, w, C, H, W, s)
        chk = R.Check(R.D(ref, DEV).reshape(-1, C), R.D(bound, DEV).reshape(-1, C))
        w8 = max(w8, chk.worst(Y.t))
        chk.verify(Y.t, 'resize fwd ' + what)
        Y.intact('resize fwd ' + what)
        if (h, w) == (H, W):
            assert torch.equal(Y.t, X.t), 'identity resize'
    print('\nresize fwd: worst err / bound %.3f' % w8)


def test_resize_backward_windows(ops):
    """resize_bilinear_bwd through the RB_TIGHT, RB_MAXW and general windows and downsampling, at N h w in {1, 7, 9} (most XCD shares
    empty), plain and accumulating, on strided views, against the float64 transpose of the fp32-coefficient operator"""
    L, s = ops.lib(), _s()
    w8 = 0.0
    for N, h, w, C, H, W, lg, lx, _ in R.RESIZE_BWD:
        r = np.random.default_rng(h * 100 + W + C)
        g = r.standard_normal((N, H, W, C)).astype(F)
        old = r.standard_normal((N, h, w, C)).astype(F)
        ref, gm, nnz = R.ref_resize_bwd(g, h, w)
        G = R.plane(g, lg)
        for acc in (0, 1):
            what = '%dx%d <- %dx%d C=%d N=%d acc=%d' % (h, w, H, W, C, N, acc)
            GX = R.out_plane(N * h * w, C, lx, old if acc else None)
            L.resize_bilinear_bwd(G.p, G.ld, GX.p, GX.ld, acc, N, h, w, C, H, W, s)
            o64 = old.astype(np.float64) if acc else 0.0
            chk = R.Check(R.D(ref + o64, DEV).reshape(-1, C), R.D((nnz + 4 + acc) * R.U * (gm + np.abs(o64)), DEV).reshape(-1, C))
            w8 = max(w8, chk.worst(GX.t))
            chk.verify(GX.t, 'resize bwd ' + what)
            GX.intact('resize bwd ' + what)
    print('\nresize bwd: worst err / bound %.3f' % w8)
