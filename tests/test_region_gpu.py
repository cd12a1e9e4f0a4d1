"""Region losses on the MI355X (csrc/region_loss.hip) against tests/region_rules.py.

Op level: the sums, the record and the head gradient against the float64 rule on bilinear logits of the same fp32 z.  Counts are exact.
I_c, P_c and rho R are sums of positive terms that pass through fewer than 100 fp32 additions before the float64 stage, held to a
relative 1e-5.  The gradient is compared as max |device - rule| <= 2e-4 max |rule| over the tensor: p (g - p.g) cancels, so single
near-zero elements carry no relative precision, while a wrong coefficient moves the result by O(1) of the scale.  Model level: the
float64 oracle backpropagates base_weight * (its own loss gradient) + the rule's gradient from its own logits."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_pkg
import region_rules as R
from test_model_gpu import TOL, _pair as _deeplab_pair, _data, _act_derivs, _act_derivs_seq

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
SUM_RTOL = 1e-5                 # issue: fewer than ~100 fp32 additions of positive terms, 100 * 2^-24 = 6e-6
GRAD_RTOL = 2e-4                # of the tensor's scale: the rtol test_head_optional_losses gives dlogits
# base_weight * base + rho R after dl3p_reduce_rows: per-pixel terms good to a few fp32 ulps (v_exp_f32, logf), summed over at most
# 2048 rows of positive fp32 partials: 2048 * 2^-24 = 1.2e-4 at worst, a tenth of that on the 2 .. 1057 rows used here
LOSS_RTOL = 1e-4
IGNORE = 255
KINDS = {'dice': (0.5, 0.5, 1.0, 1.0), 'jaccard': (1.0, 1.0, 0.5, 2.0), 'tversky': (0.3, 0.7, 1.0, 0.7)}       # alpha, beta, smooth, rho


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _guarded(n, fill=float('nan')):
    whole = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    view = whole[GUARD:GUARD + n]
    view.fill_(fill)
    return whole, view


def _guard_intact(whole, n):
    w = whole.cpu().numpy()
    return bool(np.isnan(w[:GUARD]).all() and np.isnan(w[GUARD + n:]).all())


@functools.lru_cache(maxsize=None)
def _case(N, h, w, C, H, W):
    """-> z (N,h,w,C) fp32, labels (N,H,W), pixel weights, class weights, the float64 full-resolution logits (computed once, read-only)"""
    rng = np.random.default_rng(1000 * C + H)
    z = (rng.standard_normal((N, h, w, C)) * 3).astype(np.float32)
    z[0, 0, 0, 1 % C] = 60.0                                 # one saturated logit
    y = rng.integers(0, C, (N, H, W)).astype(np.float32)
    gone = C - 1
    y[y == gone] = 0                                         # one class in no label
    y[rng.uniform(size=y.shape) < 0.3] = IGNORE
    flat = y.reshape(-1)
    flat[rng.integers(0, flat.size, 3)] = -1
    flat[rng.integers(0, flat.size, 3)] = C
    flat[0] = flat[-1] = 0                                   # (the first and the last pixel count)
    pw = rng.uniform(0.2, 4.0, N * H * W).astype(np.float32)
    cw = rng.uniform(0.5, 2.0, C).astype(np.float32)
    full = R.bilinear_logits(z, H, W)
    for a in (z, y, pw, cw, full):
        a.setflags(write=False)
    return z, y, pw, cw, full, gone


def _device_logits(z, C):
    """a view with row stride > Cpad and NaN beyond the classes"""
    N, h, w, _ = z.shape
    cp = (C + 3) // 4 * 4
    wide = torch.full((N, h, w, cp + 8), float('nan'), dtype=torch.float32, device=DEV)
    wide[..., :C] = torch.from_numpy(z.copy())
    return wide[..., :cp]


def _run_sums(ops, dz, C, H, W, dy, kind):
    alpha, beta, smooth, rho = KINDS[kind]
    nws = ops.lib().region_workspace(C) // 4
    nrec = 4 + 3 * ((C + 3) // 4 * 4)
    ws_whole, ws = _guarded(nws)
    rec_whole, rec = _guarded(nrec)
    _, rows = ops.region_sums(dz, C, H, W, dy, IGNORE, workspace=ws)
    ops.region_finalize(ws, rows, C, alpha, beta, smooth, rho, record=rec)
    assert _guard_intact(ws_whole, nws) and _guard_intact(rec_whole, nrec)
    return ws, rows, rec


def _check_record(ops, ws, rows, rec, C, want, tag):
    cp = (C + 3) // 4 * 4
    sums = ops.region_partial_sums(ws, rows, C)
    f = ops.region_record_fields(rec, C)
    assert np.array_equal(sums[2], want['Y']), tag
    worst = 0.0
    for got, ref in ((sums[0], want['I']), (sums[1], want['P'])):
        err = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
        worst = max(worst, float(err.max()))
    err_loss = abs(f['loss'] - want['loss']) / abs(want['loss'])
    S = want['Y'] > 0
    err_t = float(np.abs(f['score'][S] - want['score'][S]).max())
    print('%s: rows %d, worst relative error of I/P %.3g, of rho R %.3g, of T %.3g' % (tag, rows, worst, err_loss, err_t))
    assert worst <= SUM_RTOL and err_loss <= SUM_RTOL and err_t <= SUM_RTOL, tag
    assert f['present'] == want['present'] == int(S.sum()), tag
    assert np.isnan(f['score'][~S]).all() and not f['A'][~S].any() and not f['B'][~S].any(), tag
    # A and B are quotients of the sums with D squared below: three times the sums' bound
    assert np.allclose(f['A'], want['A'], rtol=3 * SUM_RTOL, atol=0) and np.allclose(f['B'], want['B'], rtol=3 * SUM_RTOL, atol=0), tag
    h = rec.cpu().numpy()
    assert h[2] == 0 and h[3] == 0 and np.isnan(h[4 + C:4 + cp]).all()
    assert not h[4 + cp + C:4 + 2 * cp].any() and not h[4 + 2 * cp + C:].any()


BASES = [None, ('ce',), ('weighted',), ('focal', 2.0, 0.25)]


def _check_case(ops, N, h, w, C, H, W, ld_big, kind, variants):
    z, y, pw, cw, full, gone = _case(N, h, w, C, H, W)
    alpha, beta, smooth, rho = KINDS[kind]
    dz = _device_logits(z, C)
    dy = torch.from_numpy(y.reshape(-1).copy()).to(DEV)
    dpw, dcw = torch.from_numpy(pw.copy()).to(DEV), torch.from_numpy(cw.copy()).to(DEV)
    want = R.region(full, y, alpha, beta, smooth, rho, IGNORE)
    assert want['Y'][gone] == 0 and 1 <= want['present'] <= C - 1
    tag = '%s N%d %dx%d->%dx%d C%d ld%d' % (kind, N, h, w, H, W, C, ld_big)
    ws, rows, rec = _run_sums(ops, dz, C, H, W, dy, kind)
    _check_record(ops, ws, rows, rec, C, want, tag)
    _, valid = R.valid_pixels(y, C, IGNORE)
    n = N * H * W * ld_big
    for base, weighted, bw in variants:
        spec = ('weighted', cw) if base == ('weighted',) else base
        dspec = ('weighted', dcw) if base == ('weighted',) else base
        whole, flat = _guarded(n, fill=7.0)
        out = flat.view(N, H, W, ld_big)
        loss, _ = ops.region_head_grad(dz, C, H, W, dy, rec, IGNORE, dspec, bw, dpw if weighted else None, out=out)
        assert _guard_intact(whole, n), tag
        got = out.cpu().numpy().reshape(-1, ld_big)
        rule, want_loss = want['grad'].reshape(-1, C), want['loss']
        if base is not None:
            bl, bg = R.base_gradient(full, y, spec, IGNORE, pw if weighted else None)
            rule, want_loss = rule + bw * bg.reshape(-1, C), want_loss + bw * bl
        scale = np.abs(rule).max()
        err = float(np.abs(got[:, :C] - rule).max() / scale)
        err_loss = abs(float(loss.item()) - want_loss) / max(1.0, abs(want_loss))
        print('%s base %s weighted %d: max |dev - rule| = %.3g of the scale %.3g; loss %.7g rule %.7g' % (
            tag, base and base[0], weighted, err, scale, float(loss.item()), want_loss))
        assert err <= GRAD_RTOL, (tag, base, weighted, err)
        assert err_loss <= LOSS_RTOL, (tag, base, weighted, float(loss.item()), want_loss)
        assert not got[:, C:].any(), tag                        # pad channels: exactly 0
        assert not got[~valid].any(), tag                       # rows of invalid pixels: exactly 0
        # the value-only form reports the same loss, bit for bit
        loss2, none = ops.region_head_grad(dz, C, H, W, dy, rec, IGNORE, dspec, bw, dpw if weighted else None, want_grad=False)
        assert none is None and (base is None or _bits(loss2.cpu().numpy())[0] == _bits(loss.cpu().numpy())[0]), tag
        if base is None:
            assert _bits(loss2.cpu().numpy())[0] == _bits(rec[:1].cpu().numpy())[0]
    return True


ALL_VARIANTS = [(b, wt, 0.5) for b in BASES for wt in (0, 1) if not (b is None and wt)] + [(('ce',), 0, 1.0)]
SHAPES = [(2, 3, 4, 5, 7), (2, 9, 9, 33, 33), (1, 16, 16, 16, 16)]


@pytest.mark.parametrize('C,ld_big', [(2, 4), (21, 24), (19, 24), (33, 36)])
@pytest.mark.parametrize('N,h,w,H,W', SHAPES)
def test_sums_record_and_gradient_match_the_rule(ops, N, h, w, H, W, C, ld_big):
    kind = ['dice', 'jaccard', 'tversky'][(C + H) % 3]
    assert _check_case(ops, N, h, w, C, H, W, ld_big, kind, ALL_VARIANTS)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_each_kind_at_21_classes_with_dense_rows(ops, kind):
    """ld_big == C = 21: rows that are no multiple of 4 leave channel by channel"""
    assert _check_case(ops, 2, 9, 9, 21, 33, 33, 21, kind, [(None, 0, 1.0), (('ce',), 1, 0.5)])


def test_past_the_row_cap(ops):
    assert 520 * 520 > 1024 * 256                   # the sums' grid is capped at 1024 workgroups: the grid-stride loop runs twice
    assert _check_case(ops, 1, 16, 16, 21, 520, 520, 24, 'dice', [(None, 0, 1.0), (('focal', 2.0, 0.25), 1, 0.5)])
    z, y, _, _, _, _ = _case(1, 16, 16, 21, 520, 520)
    _, rows = ops.region_sums(_device_logits(z, 21), 21, 520, 520, torch.from_numpy(y.reshape(-1).copy()).to(DEV), IGNORE)
    assert rows == 1024


def test_every_label_ignored_is_zero_with_zero_gradient(ops):
    z, _, _, _, _, _ = _case(2, 3, 4, 21, 5, 7)
    dz = _device_logits(z, 21)
    dy = torch.full((70,), float(IGNORE), dtype=torch.float32, device=DEV)
    out = ops.region_loss(dz, 21, 5, 7, dy, 0.5, 0.5, 1.0, 1.0, IGNORE)
    f = ops.region_record_fields(out['record'], 21)
    assert f['loss'] == 0.0 and f['present'] == 0 and np.isnan(f['score']).all() and not f['A'].any() and not f['B'].any()
    assert float(out['loss'].item()) == 0.0 and not out['dlogits'].cpu().numpy().any() and not out['sums'].any()


@pytest.mark.parametrize('C', [21, 33])
def test_two_runs_agree_bit_for_bit(ops, C):
    N, h, w, H, W = 2, 9, 9, 33, 33
    z, y, pw, _, _, _ = _case(N, h, w, C, H, W)
    dz, dy = _device_logits(z, C), torch.from_numpy(y.reshape(-1).copy()).to(DEV)
    dpw = torch.from_numpy(pw.copy()).to(DEV)
    runs = []
    for _ in range(2):
        ws, rows = ops.region_sums(dz, C, H, W, dy, IGNORE)
        rec = ops.region_finalize(ws, rows, C, 0.3, 0.7, 1.0, 0.7)
        loss, g = ops.region_head_grad(dz, C, H, W, dy, rec, IGNORE, ('focal', 2.0, 0.25), 0.5, dpw)
        cp = (C + 3) // 4 * 4
        runs.append((rows, _bits(ws[:rows * 3 * cp].cpu().numpy()), _bits(rec.cpu().numpy()), _bits(g.cpu().numpy()),
                     _bits(loss.cpu().numpy())))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert np.array_equal(a, b)


def test_bad_arguments_are_refused_before_any_launch(ops):
    import ctypes
    L, E = ops.lib(), ops.Dl3pError
    st = torch.cuda.current_stream().cuda_stream
    C = 5
    z = torch.zeros((1, 2, 2, 8), dtype=torch.float32, device=DEV)
    lab = torch.zeros(16, dtype=torch.float32, device=DEV)
    nws, nrec, ng = L.region_workspace(C) // 4, 4 + 3 * 8, 16 * 8
    ws_whole, ws = _guarded(nws, 3.0)
    rec_whole, rec = _guarded(nrec, 3.0)
    g_whole, g = _guarded(ng, 3.0)
    part_whole, part = _guarded(ops.MAX_STAT_ROWS, 3.0)
    cw = torch.ones(C, dtype=torch.float32, device=DEV)
    rows = ctypes.c_int(0)
    zp, lp, wp, rp, gp, pp = (t.data_ptr() for t in (z, lab, ws, rec, g, part))

    def sums(zp=zp, ldz=8, lp=lp, wp=wp, rows=ctypes.byref(rows), N=1, h=2, w=2, C=C, H=4, W=4):
        L.region_sums(zp, ldz, lp, 255, wp, rows, N, h, w, C, H, W, st)

    def finalize(wp=wp, rows=1, C=C, alpha=0.5, beta=0.5, smooth=1.0, rho=1.0, rp=rp):
        L.region_finalize(wp, rows, C, alpha, beta, smooth, rho, rp, st)

    def grad(zp=zp, ldz=8, lp=lp, kind=0, cw=None, bw=1.0, rp=rp, gp=gp, ld=8, pp=pp, rows=ctypes.byref(rows), N=1, h=2, w=2, C=C,
             H=4, W=4):
        L.region_head_grad(zp, ldz, lp, 255, 1.0 / 16, kind, cw, 0.0, 0.0, None, bw, rp, gp, ld, pp, rows, N, h, w, C, H, W, st)
    shape_bad = [dict(C=0), dict(C=257, ldz=260), dict(ldz=6), dict(ldz=4), dict(h=5), dict(w=5), dict(zp=None), dict(zp=zp + 4),
                 dict(lp=None), dict(N=0), dict(N=2048, H=1024, W=1024), dict(rows=None)]
    nan, inf = float('nan'), float('inf')
    for bad in shape_bad + [dict(wp=None), dict(wp=wp + 4)]:
        with pytest.raises(E):
            sums(**bad)
    for bad in (dict(wp=None), dict(wp=wp + 4), dict(rp=None), dict(rp=rp + 4), dict(C=0), dict(C=257), dict(rows=0),
                dict(rows=ops.MAX_STAT_ROWS + 1), dict(alpha=0.0), dict(alpha=-1.0), dict(beta=0.0), dict(smooth=-0.5), dict(rho=0.0),
                dict(alpha=nan), dict(beta=inf), dict(smooth=nan), dict(rho=inf)):
        with pytest.raises(E):
            finalize(**bad)
    for bad in shape_bad + [dict(kind=-2), dict(kind=3), dict(kind=1), dict(bw=-0.5), dict(bw=nan), dict(rp=None), dict(rp=rp + 4),
                            dict(gp=gp + 4), dict(ld=4), dict(pp=None)]:
        with pytest.raises(E):
            grad(**bad)
    torch.cuda.synchronize()
    for whole, view, n in ((ws_whole, ws, nws), (rec_whole, rec, nrec), (g_whole, g, ng), (part_whole, part, ops.MAX_STAT_ROWS)):
        assert _guard_intact(whole, n) and bool((view == 3.0).all())          # nothing was launched
    # ... and the good calls, the weighted base with its class weights included
    sums()
    finalize(rows=rows.value)
    grad(kind=1, cw=cw.data_ptr())
    grad(kind=-1)
    torch.cuda.synchronize()
    assert not bool((g == 3.0).any()) and all(_guard_intact(wh, n) for wh, n in ((ws_whole, nws), (rec_whole, nrec), (g_whole, ng)))


# ------------------------------------------------------------------------------------------------ through a model
def _gen(x, y):
    class Gen:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return x, y
    return Gen()


def _oracle_step(model_type, make_loss, seed=0, sample_weight=None):
    """one eager step of `make_loss(pkg)` -> (model, executor, oracle, oracle logits, x, y, device loss); the oracle has run its
    forward with the device's dropout masks and activation branches and waits for logits.g"""
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
    m.compile(optimizer=pkg.SGD(0.01), loss=make_loss(pkg), sample_weight_mode=None if sample_weight is None else 'temporal')
    m.use_graphs = False
    assert m.last_region is None
    x, y = _data(N, H, W, C, seed=seed)
    loss = m.train_on_batch(x, y, sample_weight=sample_weight)
    ex = m._executor(N, True)
    assert ex.region is not None and not ex.fused_head and not ex.graphed
    drops = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0]
    if model_type == 'unet_lite':
        masks = {'dropout': ex.dropout_mask(drops[0]).cpu().numpy(), 'dropout_1': ex.dropout_mask(drops[1]).cpu().numpy()}
        o.net.act_derivs = relu_derivs(m, ex)
    else:
        masks = {'aspp_dropout': ex.dropout_mask(drops[0]).cpu().numpy()}
        o.net.act_derivs = _act_derivs(m, ex, o.net.params)
        o.net.act_derivs_seq = _act_derivs_seq(m, ex, o.net.act_derivs)
    logits = o.forward_train(x, masks)
    return m, ex, o, logits, x, y, loss


def _assert_last_region(m, want):
    lr = m.last_region
    S = want['Y'] > 0
    assert lr['present'] == want['present']
    assert abs(lr['loss'] - want['loss']) < TOL * max(1.0, abs(want['loss'])), (lr['loss'], want['loss'])
    assert np.isnan(lr['score'][~S]).all() and np.abs(lr['score'][S] - want['score'][S]).max() < TOL


@pytest.mark.parametrize('model_type', ['mobilenetv2_lite', 'unet_lite'])
def test_train_step_matches_the_oracle_on_the_rules_gradient(model_type):
    from oracle import np_ops as O
    based = model_type == 'mobilenetv2_lite'
    bw = 0.5 if based else 1.0

    def make(pkg):
        if based:
            return pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy(ignore_index=255), base_weight=bw)
        return pkg.SparseJaccardLoss(ignore_index=255)
    m, ex, o, logits, x, y, loss = _oracle_step(model_type, make)
    N, H, W, C = logits.v.shape
    lab = y.reshape(N, H, W)
    alpha, beta = (0.5, 0.5) if based else (1.0, 1.0)
    want = R.region(logits.v, lab, alpha, beta, 1.0, 1.0, 255)
    total, grad = want['loss'], want['grad']
    if based:
        ce, _, g = O.loss_fwd_bwd(logits.v, lab, ('ce',), 255)
        total, grad = total + bw * ce, grad + bw * g
    logits.g = grad
    o.net.backward()
    o.sgd_step(0.01, 0.9)
    print('loss', loss, 'oracle', total, 'region', want['loss'], 'present', want['present'])
    assert abs(loss - total) < TOL * max(1.0, abs(total)), (loss, total)
    _assert_last_region(m, want)
    wts = m.get_weights_by_name()
    worst = max((float(np.abs(v - o.net.params[kk]).max() / max(1.0, np.abs(o.net.params[kk]).max())), kk) for kk, v in wts.items())
    print('worst weight', worst)
    assert worst[0] < TOL, worst
    # evaluate(): the same compiled loss on the inference forward, no gradient
    ev = m.evaluate(_gen(x, y))
    zi, _ = o.predict(x)
    wi = R.region(zi, lab, alpha, beta, 1.0, 1.0, 255)['loss']
    if based:
        wi += bw * O.loss_fwd_bwd(np.asarray(zi, np.float64), lab, ('ce',), 255)[0]
    print('evaluate', ev, 'oracle', wi)
    assert abs(ev - wi) < TOL * max(1.0, abs(wi)), (ev, wi)


def _region_model(loss, seed=0, H=65, W=65, C=21, **kw):
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', C, (H, W), 16, seed=seed)
    m.compile(optimizer=pkg.SGD(0.01), loss=loss, **kw)
    return m


def test_replayed_steps_reach_the_eager_weights_and_refresh_last_region():
    pkg = load_pkg()
    N, C, H, W = 2, 21, 65, 65
    out = []
    for graphs in (False, True):
        m = _region_model(pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy(ignore_index=255)))
        m.use_graphs = graphs
        seen = []
        for s in range(3):
            x, y = _data(N, H, W, C, seed=50 + s)
            loss = m.train_on_batch(x, y)
            lr = m.last_region
            seen.append((loss, lr['loss'], lr['present'], lr['score'].copy()))
        assert m._executor(N, True).graphed == graphs
        out.append((seen, m.get_weights_by_name()))
    (sa, wa), (sb, wb) = out
    for (la, ra, pa, ta), (lb, rb, pb, tb) in zip(sa, sb):
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la)) and abs(ra - rb) <= 1e-5 and pa == pb == C
        assert np.abs(ta - tb).max() <= 1e-5
    assert len({r for _, r, _, _ in sb}) == 3                  # refreshed every step, the replayed ones included
    worst = max(float(np.abs(wa[k] - wb[k]).max() / max(1.0, np.abs(wa[k]).max())) for k in wa)
    print('eager vs replayed after three steps:', worst)
    assert worst <= 1e-5, worst


def test_a_mining_base_reports_both_records():
    """CE mined at p = 0.25 under user sample weights (tests/test_mining_gpu.py's batch and seed, whose oracle losses leave the window
    around the threshold empty) plus Dice: the loss is base_weight * (the mined mean) + rho R from the oracle's logits"""
    import mining_rules as MR
    from test_mining_gpu import P_MINE, SEEDS
    seed, bw, rho = SEEDS['mobilenetv2_lite'], 0.5, 2.0
    sw = np.exp2(np.random.default_rng(seed + 100).uniform(-16.0, 0.0, (2, 65 * 65))).astype(np.float32)

    def make(pkg):
        return pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy(ignore_index=255, top_k_percent_pixels=P_MINE),
                                  base_weight=bw, region_weight=rho)
    m, ex, o, logits, x, y, loss = _oracle_step('mobilenetv2_lite', make, seed=seed, sample_weight=sw)
    assert ex.mining == (P_MINE, 0)
    names = [name for name, _ in ex.fwd.labels]
    i = names.index('dl3p_pixel_loss_map')
    assert names[i:i + 7] == ['dl3p_pixel_loss_map', 'dl3p_topk_threshold', 'dl3p_mining_weights', 'dl3p_region_sums',
                              'dl3p_region_finalize', 'dl3p_region_head_grad', 'dl3p_reduce_rows']
    N, H, W, C = logits.v.shape
    lab = y.reshape(N, H, W)
    l = MR.pixel_losses(logits.v, lab, ('ce',), 255, sw)
    k, theta, keep, kept, m_plus, _ = MR.rule(l, P_MINE, 0, 0)
    near = int(((np.abs(l - theta) <= 1e-3 * abs(theta)) & (l != theta)).sum())
    assert theta > 0 and near == 0, near                       # the precondition: the two kept sets cannot differ
    want = R.region(logits.v, lab, 0.5, 0.5, 1.0, rho, 255)
    total = bw * MR.mined_loss(l, P_MINE, 0, 0) + want['loss']
    print('loss', loss, 'rule', total)
    assert abs(loss - total) < TOL * max(1.0, abs(total)), (loss, total)
    lm = m.last_mining
    assert (lm['k'], lm['kept'], lm['nonzero']) == (k, kept, m_plus)
    _assert_last_region(m, want)


def test_a_bf16_model_trains_with_padded_class_rows():
    pkg = load_pkg()
    mp = pkg.mixed_precision
    N, C, H, W = 2, 19, 65, 65
    mp.set_policy(mp.Policy('mixed_bfloat16'))
    try:
        m = pkg.get_deeplabv3p_model('mobilenetv2_lite', C, (H, W), 16, training=True)
    finally:
        mp.set_policy(mp.Policy('float32'))
    assert m.bf16
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy(ignore_index=255)))
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=60)
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    assert np.isfinite(loss) and ex.cpad == 24 and ex.region is not None
    g = ex.dlogits_big.view(N * H * W, 24).cpu().numpy()
    assert g[:, :C].any() and not g[:, C:].any() and np.isfinite(g).all()
    lr = m.last_region
    assert lr['present'] == C and 0 < lr['loss'] < 1 and loss > lr['loss']


def test_fast_scnn_refuses_a_region_loss():
    pkg = load_pkg()
    m = pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256))
    with pytest.raises(ValueError, match='nearest'):
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseJaccardLoss(ignore_index=255))


def test_a_plain_loss_compiles_no_region_launch():
    pkg = load_pkg()
    N, C, H, W = 2, 21, 65, 65
    m = _region_model(pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=70)
    m.train_on_batch(x, y)
    ex = m._executor(N, True)
    assert ex.region is None and ex.region_ws is None and ex.region_record is None and m.last_region is None
    assert not any('region' in name for plan in (ex.fwd, ex.bwd, ex.opt) for name, _ in plan.labels)
    # ... and a region loss puts its three launches in front of the reduction, off the fused head
    m = _region_model(pkg.SparseTverskyLoss(0.3, 0.7, ignore_index=255))
    m.use_graphs = False
    m.train_on_batch(x, y)
    ex = m._executor(N, True)
    names = [name for name, _ in ex.fwd.labels]
    i = names.index('dl3p_region_sums')
    assert names[i:i + 4] == ['dl3p_region_sums', 'dl3p_region_finalize', 'dl3p_region_head_grad', 'dl3p_reduce_rows']
    assert 'dl3p_upsample_softmax_loss' not in names and not ex.fused_head and ex.region == (0.3, 0.7, 1.0, 1.0, 1.0, False)
