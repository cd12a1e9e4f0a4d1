"""Hard-example mining on the MI355X (csrc/mining.hip) against tests/mining_rules.py.

Selection is exact: the record and the weights are compared bit for bit with the rule applied to the very map the device selected
from.  The maps themselves are compared with the float64 restatement of the heads' per-pixel losses under TOL, the bound
tests/test_model_gpu.py applies to the weighted head.  Through a model, the float64 oracle takes the weights the rule derives from
the oracle's OWN per-pixel losses; so that the two kept sets cannot differ, the test first asserts that no oracle loss lies within a
relative 1e-3 of the oracle's threshold.  Losses of a random batch are far too dense for that (thousands of values within a factor
of two of each other), so those batches carry user sample weights 2^U(-16, 0): the weighted losses then spread over five decades,
and the seeds below are ones for which the window around the threshold is empty (mobilenetv2_lite, 8450 pixels: seed 0 leaves 2
oracle losses inside it, seed 1 none; unet_lite, 2048 pixels: seed 0 none).  The dropout mask is the device's, so this was checked on
the MI355X, where the test asserts it.  Fast-SCNN at 256 x 256 has 131072 pixels, about 24 expected inside the window at any seed:
its step is held to the rule on the device's own map instead."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_pkg
import mining_rules as R
from test_model_gpu import TOL, _pair as _deeplab_pair, _data, _act_derivs, _act_derivs_seq

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64                       # floats of NaN in front of and behind every buffer a select reads or writes (a multiple of 4)
CHUNK = 1024                     # entries one workgroup of the histogram / weights kernels takes per trip (256 lanes x 16 bytes)
FIRST_WAVE = 1024 * CHUNK        # entries the capped grid (4 workgroups per CU) covers in its first trip


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _guarded(values):
    """a device copy of `values` [P] with NaN guard bands -> (whole buffer, the 16-byte aligned view of the P entries)"""
    P = values.size
    whole = torch.full((P + 2 * GUARD + 3,), float('nan'), dtype=torch.float32, device=DEV)
    view = whole[GUARD:GUARD + P]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    return whole, view


def _guard_intact(whole, P):
    w = whole.cpu().numpy()
    return bool(np.isnan(w[:GUARD]).all() and np.isnan(w[GUARD + P:]).all())


def _record(rec):
    h = rec.cpu().numpy()
    return dict(k=int(h[0]), theta=h[1:2].view(np.float32)[0], m=int(h[2]), m_plus=int(h[3]), scale=h[4:5].view(np.float32)[0],
                pad=h[5:].tolist())


def _assert_select_equals_rule(rec, l, p, M=0, s=0):
    """record == rule(l) bit for bit; -> (keep, scale) of the rule"""
    k, theta, keep, m, m_plus, scale = R.rule(l, p, M, s)
    r = _record(rec)
    assert (r['k'], r['m'], r['m_plus'], r['pad']) == (k, m, m_plus, [0, 0, 0]), (r, k, m, m_plus)
    assert _bits(r['theta'])[()] == _bits(theta)[()], (r['theta'], theta)
    assert _bits(r['scale'])[()] == _bits(scale)[()], (r['scale'], scale)
    return keep, scale


# ------------------------------------------------------------------------------------------------ selection on given maps
def _map(kind, P, rng):
    if kind == 'equal':
        return np.full(P, 1.25, np.float32)
    if kind == 'ulp':                  # two neighbouring floats: only the last radix pass tells them apart
        return (np.float32(1.0).view(np.uint32) + rng.integers(0, 2, P).astype(np.uint32)).view(np.float32)
    if kind == 'zeros':                # 90 % exact zeros: k often exceeds the non-zero count
        l = rng.uniform(0.0, 6.0, P).astype(np.float32)
        l[rng.uniform(size=P) < 0.9] = 0.0
        return l
    if kind == 'denormal':
        l = rng.integers(1, 1 << 20, P).astype(np.uint32).view(np.float32)
        l[rng.uniform(size=P) < 0.25] = 0.0
        return l
    if kind == 'inf':
        l = rng.uniform(0.0, 6.0, P).astype(np.float32)
        l[rng.integers(0, P)] = np.inf
        return l
    if kind == 'signed':               # negative losses (negative class or sample weights) and both zeros
        l = rng.standard_normal(P).astype(np.float32)
        l[rng.uniform(size=P) < 0.2] = 0.0
        l[rng.uniform(size=P) < 0.1] = -0.0
        return l
    raise ValueError(kind)


SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, CHUNK + 5, FIRST_WAVE + 7]


@pytest.mark.parametrize('P', SIZES)
@pytest.mark.parametrize('kind', ['equal', 'ulp', 'zeros', 'denormal', 'inf', 'signed'])
def test_select_and_weights_are_exact(ops, kind, P):
    rng = np.random.default_rng(1000 + P)
    l = _map(kind, P, rng)
    base = rng.uniform(0.25, 4.0, P).astype(np.float32)
    whole, dmap = _guarded(l)
    _, dbase = _guarded(base)
    for k in sorted({1, min(2, P), max(P - 1, 1), P}):
        p = 1.0 if k == P else (k + 0.5) / P                 # int(p P) == k
        assert R.kept_count(P, p, 0, 0) == k
        rec = ops.topk_threshold(dmap, p)          # a map from elsewhere: the select counts the first pass itself
        keep, scale = _assert_select_equals_rule(rec, l, p)
        for b, dbase_k in ((None, None), (base, dbase)):
            wwhole, wview = _guarded(np.zeros(P, np.float32))
            ops.mining_weights(dmap, rec, base=dbase_k, out=wview)
            want = np.where(keep, (np.float32(1.0) if b is None else b) * scale, np.float32(0.0)).astype(np.float32)
            assert np.array_equal(_bits(wview.cpu().numpy()), _bits(want)), (kind, P, k)
            assert _guard_intact(wwhole, P)
    assert _guard_intact(whole, P) and np.array_equal(_bits(dmap.cpu().numpy()), _bits(l))


def test_select_is_repeatable_and_leaves_its_workspace_zero(ops):
    rng = np.random.default_rng(5)
    P = 3 * CHUNK + 1
    _, dmap = _guarded(rng.uniform(0, 6, P).astype(np.float32))
    ws = ops.mining_workspace(DEV)
    recs = []
    for _ in range(3):
        rec = torch.zeros(8, dtype=torch.int32, device=DEV)
        ops.lib().topk_threshold(dmap.data_ptr(), P, 0.25, 0, None, 0, 0, ws.data_ptr(), rec.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        recs.append(rec.cpu().numpy())
        assert not ws[:1025].cpu().numpy().any()             # the four histograms and the zero count
    assert all(np.array_equal(recs[0], r) for r in recs[1:])


def test_k_is_computed_on_the_device_from_the_step_counter(ops):
    rng = np.random.default_rng(6)
    P, p, M = 1000, 0.25, 10
    l = rng.uniform(0, 6, P).astype(np.float32)
    _, dmap = _guarded(l)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for s in (0, 5, 10, 20, 3, 7):
        step.fill_(s)
        _assert_select_equals_rule(ops.topk_threshold(dmap, p, M, step_counter=step), l, p, M, s)
        step.fill_(s + 1)            # the training plan has already counted the step it is in
        _assert_select_equals_rule(ops.topk_threshold(dmap, p, M, step_counter=step, step_bias=-1), l, p, M, s)
    step.fill_(0)
    _assert_select_equals_rule(ops.topk_threshold(dmap, p, M, step_counter=step, step_bias=-1), l, p, M, 0)      # clamped at 0
    assert R.kept_count(P, p, M, 5) == 625


def test_bad_arguments_are_refused_before_any_launch(ops):
    L, E = ops.lib(), ops.Dl3pError
    st = torch.cuda.current_stream().cuda_stream
    z = torch.zeros((1, 2, 2, 8), dtype=torch.float32, device=DEV)
    lab = torch.zeros(16, dtype=torch.float32, device=DEV)
    out = torch.zeros(16 + 4, dtype=torch.float32, device=DEV)
    ws, rec = ops.mining_workspace(DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    zp, lp, op, wp, rp = z.data_ptr(), lab.data_ptr(), out.data_ptr(), ws.data_ptr(), rec.data_ptr()

    def loss_map(fn, zp=zp, ldz=8, lp=lp, kind=0, cw=None, op=op, wp=wp, N=1, h=2, w=2, C=5, H=4, W=4):
        fn(zp, ldz, lp, 255, kind, cw, 0.0, 0.0, None, op, wp, N, h, w, C, H, W, st)
    for fn in (L.pixel_loss_map, L.nearest_pixel_loss_map):
        loss_map(fn)                                          # the good call, and the select that takes its histogram
        ops.topk_threshold(out[:16], 0.5, workspace=ws, record=rec)
        for bad in (dict(N=2048, H=1024, W=1024), dict(ldz=6), dict(ldz=4), dict(zp=zp + 4), dict(op=op + 4), dict(wp=wp + 4),
                    dict(C=0), dict(C=257, ldz=260), dict(kind=1), dict(kind=3), dict(lp=None), dict(op=None), dict(wp=None),
                    dict(zp=None), dict(N=0)):
            with pytest.raises(E):
                loss_map(fn, **bad)
    with pytest.raises(E):
        loss_map(L.pixel_loss_map, h=5, H=4)                  # the bilinear head upsamples
    with pytest.raises(E):
        loss_map(L.nearest_pixel_loss_map, H=5)               # H = r h
    with pytest.raises(E):
        loss_map(L.nearest_pixel_loss_map, h=1, w=1, H=9, W=9)      # r <= 8
    out2 = torch.zeros(16, dtype=torch.float32, device=DEV)
    L.mining_weights(op, None, rp, out2.data_ptr(), 16, st)
    for bad in (dict(P=0), dict(P=1 << 31), dict(p=0.0), dict(p=1.5), dict(M=-1), dict(mp=op + 4), dict(wp=wp + 4), dict(rp=rp + 4),
                dict(mp=None), dict(wp=None), dict(rp=None)):
        a = dict(mp=op, P=16, p=0.5, M=0, wp=wp, rp=rp)
        a.update(bad)
        with pytest.raises(E):
            L.topk_threshold(a['mp'], a['P'], a['p'], a['M'], None, 0, 0, a['wp'], a['rp'], st)
    for bad in (dict(P=0), dict(P=1 << 31), dict(mp=op + 4), dict(bp=op + 4), dict(rp=rp + 4), dict(out=op + 4), dict(mp=None),
                dict(rp=None), dict(out=None)):
        a = dict(mp=op, bp=None, rp=rp, out=out2.data_ptr(), P=16)
        a.update(bad)
        with pytest.raises(E):
            L.mining_weights(a['mp'], a['bp'], a['rp'], a['out'], a['P'], st)
    torch.cuda.synchronize()
    assert not ws.cpu().numpy()[:1025].any()


# ------------------------------------------------------------------------------------------------ the loss maps of the two heads
KINDS = [('ce',), ('weighted', 'random'), ('weighted', 'ones'), ('focal', 2.0, 0.25)]


def _head_case(N, h, w, C, H, W, seed, ignored, pixel_weighted):
    rng = np.random.default_rng(seed)
    cp = (C + 3) // 4 * 4
    z = (rng.standard_normal((N, h, w, cp)) * 3).astype(np.float32)
    y = rng.integers(0, C, (N, H, W)).astype(np.float32)
    if ignored:
        y[rng.uniform(size=y.shape) < 0.3] = 255
    pw = rng.uniform(0.2, 4.0, N * H * W).astype(np.float32) if pixel_weighted else None
    cw = rng.uniform(0.5, 2.0, C).astype(np.float32)
    return z, y, pw, cw


def _check_maps(ops, nearest, N, h, w, C, H, W, kinds=KINDS, variants=((0, 0), (0, 1), (1, 0), (1, 1))):
    cp = (C + 3) // 4 * 4
    for ignored, pixel_weighted in variants:
        z, y, pw, cw = _head_case(N, h, w, C, H, W, 7 * C + h, ignored, pixel_weighted)
        wide = torch.full((N, h, w, cp + 8), float('nan'), dtype=torch.float32, device=DEV)       # row stride > C
        dz = wide[..., :cp]
        dz.copy_(torch.from_numpy(z))
        dy = torch.from_numpy(y.reshape(-1)).to(DEV)
        dpw = None if pw is None else torch.from_numpy(pw).to(DEV)
        full = R.nearest_logits(z[..., :C], H // h) if nearest else R.bilinear_logits(z[..., :C], H, W)
        for kind in kinds:
            weights = None
            if kind[0] == 'weighted':
                weights = cw if kind[1] == 'random' else np.ones(C, np.float32)
            spec = ('weighted', weights) if weights is not None else kind
            dspec = ('weighted', torch.from_numpy(weights).to(DEV)) if weights is not None else kind
            want = R.pixel_losses(full, y, spec, 255, pw)
            whole, out = _guarded(np.zeros(N * H * W, np.float32))
            ws = ops.mining_workspace(DEV)
            ops.pixel_loss_map(dz, C, H, W, dy, 255, dspec, dpw, nearest=nearest, out=out, workspace=ws)
            got = out.cpu().numpy()
            assert _guard_intact(whole, N * H * W)
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            assert err.max() < TOL, (kind[0], ignored, pixel_weighted, float(err.max()))
            assert not np.signbit(got[got == 0]).any()
            assert (got[y.reshape(-1) == 255] == 0).all()
            # the same launch left the first histogram: the select that uses it is exact on the device's own map
            rec = ops.topk_threshold(out, 0.25, workspace=ws)
            keep, scale = _assert_select_equals_rule(rec, got, 0.25)
            assert not ws.cpu().numpy()[:1025].any()
            wgt = ops.mining_weights(out, rec, base=dpw)
            base = np.float32(1.0) if pw is None else pw
            assert np.array_equal(_bits(wgt.cpu().numpy()), _bits(np.where(keep, base * scale, np.float32(0)).astype(np.float32)))
    return True


@pytest.mark.parametrize('C', [2, 21, 40])
@pytest.mark.parametrize('h,w,H,W', [(3, 4, 5, 7), (17, 17, 65, 65), (16, 16, 16, 16)])
def test_bilinear_loss_map(ops, h, w, H, W, C):
    assert _check_maps(ops, False, 2, h, w, C, H, W)


def test_bilinear_loss_map_past_the_grids_first_wave(ops):
    assert 520 * 520 > 1024 * 256                              # one thread per pixel, 4 workgroups per CU
    assert _check_maps(ops, False, 1, 16, 16, 21, 520, 520, kinds=[('ce',)], variants=((1, 1),))


@pytest.mark.parametrize('C', [2, 21, 40])
@pytest.mark.parametrize('r', [1, 8])
def test_nearest_loss_map(ops, r, C):
    assert _check_maps(ops, True, 2, 2, 3, C, 2 * r, 3 * r)


def _check_map_is_the_heads_loss(ops, nearest, N, h, w, C, H, W):
    """map[i] == the head's reduced loss under pixel weights that are 1.0 at pixel i and 0 elsewhere, with inv_count = 1: every
    other term of the head's sums is an exact zero, so the two share all 32 bits where they share the per-pixel expression"""
    P = N * H * W
    z, y, _, cw = _head_case(N, h, w, C, H, W, 7 * C + h, True, False)
    y = y.reshape(-1)
    ignored_px = 1
    pixels = [0, P - 1, H * W, H * W + W - 1, P - W, P - 1, (H // 2) * W + W // 2]     # first, last, image 1's corners, interior
    assert ignored_px not in pixels
    rng = np.random.default_rng(3)
    for i in pixels:
        if y[i] == 255:
            y[i] = rng.integers(0, C)
    y[ignored_px] = 255
    dz, dy = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    full = R.nearest_logits(z[..., :C], H // h) if nearest else R.bilinear_logits(z[..., :C], H, W)
    st = torch.cuda.current_stream().cuda_stream
    partial = torch.zeros(ops.MAX_STAT_ROWS, dtype=torch.float32, device=DEV)
    total = torch.empty(1, dtype=torch.float32, device=DEV)
    for kind, spec, dspec, args in ((0, ('ce',), ('ce',), (None, 0.0, 0.0)),
                                    (1, ('weighted', cw), ('weighted', torch.from_numpy(cw).to(DEV)), None),
                                    (2, ('focal', 2.0, 0.25), ('focal', 2.0, 0.25), (None, 2.0, 0.25))):
        if args is None:
            args = (dspec[1].data_ptr(), 0.0, 0.0)
        want = R.pixel_losses(full, y.reshape(N, H, W), spec, 255, None)
        assert all(np.isfinite(want[i]) and want[i] > 0 for i in pixels), (spec[0], [want[i] for i in pixels])
        lmap = ops.pixel_loss_map(dz, C, H, W, dy, 255, dspec, None, nearest=nearest)[0].cpu().numpy()
        for i in pixels + [ignored_px]:
            onehot = torch.zeros(P, dtype=torch.float32, device=DEV)
            onehot[i] = 1.0
            rows = ctypes.c_int(0)
            if nearest:
                ops.lib().nearest_head_train(dz.data_ptr(), dz.shape[-1], dy.data_ptr(), 255, 1.0, kind, *args, onehot.data_ptr(), None,
                                             0, 0, partial.data_ptr(), ctypes.byref(rows), N, h, w, C, H, W, st)
            else:
                ops.lib().upsample_softmax_loss(dz.data_ptr(), dz.shape[-1], dy.data_ptr(), 255, 1.0, kind, *args, onehot.data_ptr(),
                                                None, None, None, dz.shape[-1], partial.data_ptr(), ctypes.byref(rows), N, h, w, C,
                                                H, W, st)
            ops.lib().reduce_rows(partial.data_ptr(), rows.value, 1, total.data_ptr(), 0, st)
            head = total.cpu().numpy()
            print('%s C %d %s pixel %d: head %.9g map %.9g' % ('nearest' if nearest else 'bilinear', C, spec[0], i, head[0], lmap[i]))
            assert _bits(head)[0] == _bits(lmap[i:i + 1])[0], (spec[0], i, float(head[0]), float(lmap[i]))
            if i == ignored_px:
                assert _bits(head)[0] == 0 and _bits(lmap[i:i + 1])[0] == 0
    return True


@pytest.mark.parametrize('C', [2, 21, 40])
def test_bilinear_loss_map_is_the_heads_loss_bit_for_bit(ops, C):
    assert _check_map_is_the_heads_loss(ops, False, 2, 3, 4, C, 5, 7)


@pytest.mark.parametrize('C', [2, 21, 40])
@pytest.mark.parametrize('r', [1, 8])
def test_nearest_loss_map_is_the_heads_loss_bit_for_bit(ops, r, C):
    assert _check_map_is_the_heads_loss(ops, True, 2, 2, 3, C, 2 * r, 3 * r)


def test_the_weighted_head_reports_the_rules_loss(ops):
    """map -> select -> weights -> dl3p_upsample_softmax_loss / dl3p_nearest_head_train: the head's sum of l_i w_i / P is the rule's
    sum over the kept / max(m+, 1), which holds by construction (w_i carries P / m+)"""
    for nearest, (h, w, H, W) in ((False, (17, 17, 65, 65)), (True, (4, 6, 32, 48))):
        N, C = 2, 21
        z, y, pw, _ = _head_case(N, h, w, C, H, W, 11, True, True)
        dz, dy, dpw = torch.from_numpy(z).to(DEV), torch.from_numpy(y.reshape(-1)).to(DEV), torch.from_numpy(pw).to(DEV)
        lmap, ws = ops.pixel_loss_map(dz, C, H, W, dy, 255, ('ce',), dpw, nearest=nearest)
        wgt = ops.mining_weights(lmap, ops.topk_threshold(lmap, 0.25, workspace=ws), base=dpw)
        if nearest:
            total, _ = ops.nearest_head_train(dz, C, H, W, dy, 255, ('ce',), pixel_weights=wgt, want_grad=False)
        else:
            partial = torch.zeros(ops.MAX_STAT_ROWS, dtype=torch.float32, device=DEV)
            rows = ctypes.c_int(0)
            st = torch.cuda.current_stream().cuda_stream
            ops.lib().upsample_softmax_loss(dz.data_ptr(), dz.shape[-1], dy.data_ptr(), 255, 1.0 / (N * H * W), 0, None, 0.0, 0.0,
                                            wgt.data_ptr(), None, None, None, dz.shape[-1], partial.data_ptr(), ctypes.byref(rows),
                                            N, h, w, C, H, W, st)
            total = torch.empty(1, dtype=torch.float32, device=DEV)
            ops.lib().reduce_rows(partial.data_ptr(), rows.value, 1, total.data_ptr(), 0, st)
        want = R.mined_loss(lmap.cpu().numpy(), 0.25, 0, 0)
        assert abs(float(total.item()) - want) < TOL * max(1.0, abs(want)), (nearest, float(total.item()), want)


# ------------------------------------------------------------------------------------------------ through a model
P_MINE = 0.25
SEEDS = {'mobilenetv2_lite': 1, 'unet_lite': 0}          # batches whose oracle losses leave the window around the threshold empty


def _batch(N, H, W, C, seed):
    x, y = _data(N, H, W, C, seed=seed)
    sw = np.exp2(np.random.default_rng(seed + 100).uniform(-16.0, 0.0, (N, H * W))).astype(np.float32)
    return x, y, sw


def _mined_train_step(model_type, seed, measure_only=False):
    """one eager step with p = 0.25 against the oracle on the weights the rule derives from the oracle's own per-pixel losses"""
    pkg = load_pkg()
    C, N = 21, 2
    if model_type == 'unet_lite':
        from test_unet_gpu import _pair as _unet_pair
        from unet_oracle import relu_derivs
        H = W = 32
        m, o = _unet_pair(model_type, H, W, C)
    else:
        H = W = 65
        m, o = _deeplab_pair(model_type, H, W, C)
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255, top_k_percent_pixels=P_MINE),
              sample_weight_mode='temporal')
    m.use_graphs = False
    x, y, sw = _batch(N, H, W, C, seed)
    loss = m.train_on_batch(x, y, sample_weight=sw)
    ex = m._executor(N, True)
    assert ex.mining == (P_MINE, 0) and not ex.graphed
    drops = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0]
    if model_type == 'unet_lite':
        masks = {'dropout': ex.dropout_mask(drops[0]).cpu().numpy(), 'dropout_1': ex.dropout_mask(drops[1]).cpu().numpy()}
        o.net.act_derivs = relu_derivs(m, ex)
    else:
        masks = {'aspp_dropout': ex.dropout_mask(drops[0]).cpu().numpy()}
        o.net.act_derivs = _act_derivs(m, ex, o.net.params)
        o.net.act_derivs_seq = _act_derivs_seq(m, ex, o.net.act_derivs)
    _, _, logits = o.loss_and_grads(x, y, masks, sample_weight=sw)
    P = N * H * W
    l = R.pixel_losses(logits, y.reshape(N, H, W), ('ce',), 255, sw)
    k, theta, keep, kept, m_plus, _ = R.rule(l, P_MINE, 0, 0)
    near = int(((np.abs(l - theta) <= 1e-3 * abs(theta)) & (l != theta)).sum())
    print('%s seed %d: k %d theta %.6g kept %d nonzero %d, oracle losses within 1e-3 of theta: %d' % (model_type, seed, k, theta, kept,
                                                                                                     m_plus, near))
    if measure_only:
        return near
    assert theta > 0 and near == 0, near         # the precondition: the two kept sets cannot differ
    w = keep * sw.reshape(-1).astype(np.float64) * (P / max(m_plus, 1))
    _, data_loss, _ = o.loss_and_grads(x, y, masks, sample_weight=w.reshape(N, H * W))
    want = R.mined_loss(l, P_MINE, 0, 0)
    print('loss', loss, 'oracle', data_loss, 'rule', want)
    assert abs(data_loss - want) < 1e-9 * max(1.0, abs(want))         # the oracle's weighted mean IS the rule's loss
    assert abs(loss - data_loss) < TOL * max(1.0, abs(data_loss)), (loss, data_loss)
    lm = m.last_mining
    assert (lm['k'], lm['kept'], lm['nonzero']) == (k, kept, m_plus), (lm, k, kept, m_plus)
    assert abs(lm['threshold'] - theta) < TOL * max(1.0, abs(theta))
    # the device kept the pixels the oracle kept, and the user's weights are still what was set
    dev_keep = ex.mining_weights.cpu().numpy() != 0
    assert np.array_equal(dev_keep, keep)
    assert np.array_equal(ex.pixel_weights.cpu().numpy(), sw.reshape(-1))
    o.sgd_step(0.01, 0.9)
    wts = m.get_weights_by_name()
    worst = max((float(np.abs(v - o.net.params[kk]).max() / max(1.0, np.abs(o.net.params[kk]).max())), kk) for kk, v in wts.items())
    print('worst weight', worst)
    assert worst[0] < TOL, worst
    return near


@pytest.mark.parametrize('model_type', ['mobilenetv2_lite', 'unet_lite'])
def test_train_step_matches_oracle_on_the_rules_weights(model_type):
    _mined_train_step(model_type, SEEDS[model_type])


def _plain_model(loss, seed=0, H=65, W=65, C=21):
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', C, (H, W), 16, seed=seed)
    m.compile(optimizer=pkg.SGD(0.01), loss=loss)
    return m


def test_replayed_steps_follow_the_ramp_and_evaluate_does_not_advance_it():
    pkg = load_pkg()
    N, C, H, W, M = 2, 21, 65, 65, 2
    P = N * H * W
    m = _plain_model(pkg.SparseCategoricalCrossEntropy(ignore_index=255, top_k_percent_pixels=P_MINE, hard_example_mining_step=M))
    assert m.last_mining is None
    ks, losses = [], []
    for s in range(3):
        x, y = _data(N, H, W, C, seed=20 + s)
        losses.append(m.train_on_batch(x, y))
        lm = m.last_mining
        ks.append(lm['k'])
        assert lm['kept'] >= lm['k'] >= 1 and lm['nonzero'] <= lm['kept']
        ex = m._executor(N, True)
        # the reported loss is the rule's on the map the device selected from
        l = ex.loss_map.cpu().numpy()
        assert abs(losses[-1] - R.mined_loss(l, P_MINE, M, s)) < TOL * max(1.0, losses[-1])
        if s == 0:
            # one step completed: evaluate() mines at r = 1/2 and leaves the counter alone (twice: the same bits)

            class Gen:
                def __len__(self):
                    return 1
                def __getitem__(self, i):
                    return x, y
            ev = [m.evaluate(Gen()), m.evaluate(Gen())]
            evx = m._executor(N, False)
            rec = _record(evx.mining_record)
            le = evx.loss_map.cpu().numpy()
            assert rec['k'] == R.kept_count(P, P_MINE, M, 1) and ev[0] == ev[1]
            assert abs(ev[0] - R.mined_loss(le, P_MINE, M, 1)) < TOL * max(1.0, ev[0])
    assert m._executor(N, True).graphed
    assert ks == [P, int((0.5 * P_MINE + 0.5) * P), int(P_MINE * P)] == [8450, 5281, 2112], ks
    assert np.isfinite(losses).all()


def test_top_k_percent_pixels_of_one_changes_nothing():
    pkg = load_pkg()
    N, C, H, W = 2, 21, 65, 65
    x, y = _data(N, H, W, C, seed=30)
    out = []
    for kw in ({}, dict(top_k_percent_pixels=1.0, hard_example_mining_step=5)):
        m = _plain_model(pkg.SparseCategoricalCrossEntropy(ignore_index=255, **kw))
        m.use_graphs = False
        loss = np.float32(m.train_on_batch(x, y))
        ex = m._executor(N, True)
        assert ex.mining is None and ex.loss_map is None and m.last_mining is None
        out.append((loss, [ex.fwd.labels, ex.bwd.labels, ex.opt.labels], m.get_weights_by_name()))
    (la, pa, wa), (lb, pb, wb) = out
    assert pa == pb and not any('mining' in name or 'loss_map' in name or 'topk' in name for plan in pa for name, _ in plan)
    assert _bits(la)[()] == _bits(lb)[()], (la, lb)
    for k in wa:
        assert np.array_equal(_bits(wa[k]), _bits(wb[k])), k
    # ... and with mining on the three stages stand in front of the weighted head, off the fused one
    m = _plain_model(pkg.SparseCategoricalCrossEntropy(ignore_index=255, top_k_percent_pixels=P_MINE))
    m.use_graphs = False
    m.train_on_batch(x, y)
    ex = m._executor(N, True)
    names = [name for name, _ in ex.fwd.labels]
    i = names.index('dl3p_pixel_loss_map')
    assert names[i:i + 4] == ['dl3p_pixel_loss_map', 'dl3p_topk_threshold', 'dl3p_mining_weights', 'dl3p_upsample_softmax_loss']
    assert not ex.fused_head and not ex.fused_head_rows and ex.pixel_weights is None


def test_fast_scnn_step_mines_behind_the_nearest_head():
    """256 x 256, N = 2 (P = 131072: far too many losses for the oracle precondition above to hold, so this checks the plan and the
    reported loss against the rule on the device's own map)"""
    pkg = load_pkg()
    N, C, H, W = 2, 21, 256, 256
    m = pkg.get_fast_scnn_model('fast_scnn', C, (H, W))
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseSoftmaxFocalLoss(ignore_index=255, top_k_percent_pixels=P_MINE))
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=40)
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    names = [name for name, _ in ex.fwd.labels]
    i = names.index('dl3p_nearest_pixel_loss_map')
    assert names[i:i + 4] == ['dl3p_nearest_pixel_loss_map', 'dl3p_topk_threshold', 'dl3p_mining_weights', 'dl3p_nearest_head_train']
    l = ex.loss_map.cpu().numpy()
    keep, scale = _assert_select_equals_rule(ex.mining_record, l, P_MINE)
    assert np.array_equal(_bits(ex.mining_weights.cpu().numpy()), _bits(np.where(keep, scale, np.float32(0)).astype(np.float32)))
    want = R.mined_loss(l, P_MINE, 0, 0)
    assert abs(loss - want) < TOL * max(1.0, abs(want)), (loss, want)
    lm = m.last_mining
    assert lm['k'] == int(P_MINE * N * H * W) and lm['kept'] == int(keep.sum())
