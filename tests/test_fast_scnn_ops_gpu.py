"""The nearest-upsampling kernels (csrc/nearest.hip, csrc/nearest_head.hip) per element against float64 NumPy, at the smallest shapes
that reach every edge: odd low-resolution maps, one float4 per pixel / one slab with idle lanes (C = 132 -> 33 channel lanes, 7 pixel
lanes), channel-slice views between NaN neighbours, both pooling kernels (windows of up to 16 taps / larger), an uncovered row.

Bounds (the rule of tests/ew_rules.py: k * U * sum of the magnitudes of the terms, U = 2^-24, k = fp32 roundings on the path + 1):
  upsample-add   one fma per prologue (2), the add (1), 2 more for a ReLU whose argument lies within 2 U T of 0 (it may take either
                 branch: the difference is that argument), + 1 -> 6 U (|a sa| + |ha| + |b sb| + |hb|)
  statistics     fp32 sums of n terms delivered in `rows` partial rows, against the float64 sums of the values the kernel WROTE:
                 (n + rows + 4) U sum|term|
  block sum      r r adds, the accumulate add, + 1 -> (r r + 2) U (sum|g| + |old|)
  window pool    any summation order of n terms is within (n - 1) U sum|term|; prologue fma, the division, + 1 -> (n + 2) U mean|term|;
                 backward: the division, the accumulate add, + 1 -> 3 U (|dy| / n + |old|); uncovered pixels exactly 0
The head keeps the tolerances of tests/test_unet_gpu.py::test_head_ops_with_logits_at_full_resolution."""
import numpy as np
import pytest
import torch

from oracle import np_ops as O
import ew_rules as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = R.U


def _wide(a, pad=4):
    """`a` (.., C) as the channel slice [pad, pad + C) of a NaN-filled buffer 2 pad wider -> (buffer, view)"""
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + 2 * pad,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[..., pad:pad + a.shape[-1]]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return buf, view


def _neighbours_untouched(buf, pad=4):
    assert bool(torch.isnan(buf[..., :pad]).all()) and bool(torch.isnan(buf[..., -pad:]).all())


def _within(got, ref, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= bound)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError('%s: %d of %d out of bound, first at %s: got %r want %r bound %.3g' % (
            what, bad.sum(), bad.size, tuple(i), got[tuple(i)], ref[tuple(i)], bound[tuple(i)]))


def _prologue(v, C, rng, on):
    """(scale, shift, act, float64 value, magnitude of its terms)"""
    if not on:
        return None, None, R.NONE, v.astype(np.float64), np.abs(v.astype(np.float64))
    sc = rng.uniform(0.5, 1.5, C).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    u = v.astype(np.float64) * sc + sh
    return sc, sh, R.RELU, np.maximum(u, 0.0), np.abs(v.astype(np.float64) * sc) + np.abs(sh)


@pytest.mark.parametrize('C', [4, 128, 132])
@pytest.mark.parametrize('r', [2, 4])
@pytest.mark.parametrize('pro', ['none', 'a', 'b', 'both'])
def test_upsample_add_and_its_statistics(ops, C, r, pro):
    N, h, w = 2, 3, 5
    H, W = r * h, r * w
    rng = np.random.default_rng(1000 * C + 10 * r + len(pro))
    a = rng.standard_normal((N, H, W, C)).astype(np.float32)
    b = rng.standard_normal((N, h, w, C)).astype(np.float32)
    asc, ash, aact, av, am = _prologue(a, C, rng, pro in ('a', 'both'))
    bsc, bsh, bact, bv, bm = _prologue(b, C, rng, pro in ('b', 'both'))
    up = lambda t: np.repeat(np.repeat(t, r, 1), r, 2)
    ref, mag = av + up(bv), am + up(bm)
    abuf, at = _wide(a)
    bbuf, bt = _wide(b)
    obuf, ot = _wide(np.zeros_like(a))
    ot.fill_(float('nan'))
    dev = lambda v: None if v is None else torch.from_numpy(v).to(DEV)
    partials = torch.full((R.MAX_STAT_ROWS * 2 * C,), float('nan'), dtype=torch.float32, device=DEV)
    _, rows = ops.upsample_add_fwd(at, bt, r, dev(asc), dev(ash), aact, dev(bsc), dev(bsh), bact, out=ot, partials=partials)
    _within(ot, ref, 6 * U * mag, 'out')
    for buf in (abuf, bbuf, obuf):
        _neighbours_untouched(buf)
    assert 1 <= rows <= R.MAX_STAT_ROWS
    got = ot.detach().cpu().numpy().astype(np.float64)
    sums = partials[:rows * 2 * C].view(rows, 2, C).double().sum(0).cpu().numpy()
    n = N * H * W
    _within(torch.from_numpy(sums[0]), got.sum((0, 1, 2)), (n + rows + 4) * U * np.abs(got).sum((0, 1, 2)), 'sum')
    _within(torch.from_numpy(sums[1]), (got * got).sum((0, 1, 2)), (n + rows + 4) * U * (got * got).sum((0, 1, 2)), 'sum of squares')
    assert bool(torch.isnan(partials[rows * 2 * C:]).all())          # no row past rows_out is written
    # without statistics the output is the same, bit for bit
    o2 = ops.upsample_add_fwd(at, bt, r, dev(asc), dev(ash), aact, dev(bsc), dev(bsh), bact)
    assert torch.equal(o2, ot)


@pytest.mark.parametrize('C', [4, 128, 132])
@pytest.mark.parametrize('r', [2, 4])
@pytest.mark.parametrize('accumulate', [False, True])
def test_block_sum(ops, C, r, accumulate):
    N, h, w = 2, 3, 5
    H, W = r * h, r * w
    rng = np.random.default_rng(77 * C + r + accumulate)
    g = rng.standard_normal((N, H, W, C)).astype(np.float32)
    old = rng.standard_normal((N, h, w, C)).astype(np.float32)
    g64 = g.astype(np.float64).reshape(N, h, r, w, r, C)
    ref, mag = g64.sum((2, 4)), np.abs(g64).sum((2, 4))
    if accumulate:
        ref, mag = ref + old, mag + np.abs(old)
    gbuf, gt = _wide(g)
    obuf, ot = _wide(old)
    if not accumulate:
        ot.fill_(float('nan'))
    ops.block_sum_bwd(gt, r, out=ot, accumulate=accumulate)
    _within(ot, ref, (r * r + 2) * U * mag, 'block sum')
    _neighbours_untouched(gbuf)
    _neighbours_untouched(obuf)


def _pool_ref(x, sc, sh, act, kh, kw):
    N, H, W, C = x.shape
    Ho, Wo = H // kh, W // kw
    u, T, _ = R.pro64(R.D(x), R.D(sc), R.D(sh))
    a, am = R.act64(u, act).numpy(), R.act_mag(T, act).numpy()
    win = lambda t: t[:, :Ho * kh, :Wo * kw].reshape(N, Ho, kh, Wo, kw, C)
    return win(a).mean((2, 4)), win(am).mean((2, 4))


# (H, W, kh, kw): a 9 x 10 map with a leftover row under (4, 5) = 20 taps (the workgroup kernel) and (2, 2); (1, 1); 16 taps, the last
# size of the one-thread kernel, and 17 = the first of the workgroup kernel; one 64 x 64 window over a 64 x 64 map
POOL_CASES = [(9, 10, 4, 5), (9, 10, 2, 2), (9, 10, 1, 1), (9, 16, 4, 4), (9, 17, 1, 17), (64, 64, 64, 64)]


@pytest.mark.parametrize('H,W,kh,kw', POOL_CASES)
@pytest.mark.parametrize('C', [4, 132])
@pytest.mark.parametrize('pro', [False, True])
def test_window_pooling_forward(ops, H, W, kh, kw, C, pro):
    N = 2
    rng = np.random.default_rng(H * W + kh * 131 + kw + C)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    sc = sh = None
    act = R.NONE
    if pro:
        # shifted well away from the ReLU kink for most elements; the few near it move the mean by less than the bound's own term
        sc, sh, act = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.5, 0.5, C).astype(np.float32), R.RELU
    ref, mag = _pool_ref(x, sc, sh, act, kh, kw)
    xbuf, xt = _wide(x)
    obuf, ot = _wide(np.zeros((N, H // kh, W // kw, C), np.float32))
    ot.fill_(float('nan'))
    dev = lambda v: None if v is None else torch.from_numpy(v).to(DEV)
    ops.winpool2d_fwd(xt, kh, kw, dev(sc), dev(sh), act, out=ot)
    n = kh * kw
    # a ReLU argument within 2 U T of 0 contributes at most that to the sum: 2 more roundings' worth on every term
    _within(ot, ref, (n + 2 + (2 if pro else 0)) * U * mag, 'mean')
    _neighbours_untouched(xbuf)
    _neighbours_untouched(obuf)


@pytest.mark.parametrize('H,W,kh,kw', POOL_CASES)
@pytest.mark.parametrize('C', [4, 132])
@pytest.mark.parametrize('accumulate', [False, True])
def test_window_pooling_backward(ops, H, W, kh, kw, C, accumulate):
    N = 2
    Ho, Wo = H // kh, W // kw
    rng = np.random.default_rng(H + W * 7 + kh * 131 + kw + C + accumulate)
    dy = rng.standard_normal((N, Ho, Wo, C)).astype(np.float32)
    old = rng.standard_normal((N, H, W, C)).astype(np.float32)
    n = kh * kw
    ref = np.zeros((N, H, W, C))
    ref[:, :Ho * kh, :Wo * kw] = np.repeat(np.repeat(dy.astype(np.float64), kh, 1), kw, 2) / n
    mag = np.abs(ref)
    if accumulate:
        ref, mag = ref + old, mag + np.abs(old)
    dbuf, dt = _wide(dy)
    gbuf, gt = _wide(old)
    if not accumulate:
        gt.fill_(float('nan'))
    ops.winpool2d_bwd(dt, (N, H, W, C), kh, kw, out=gt, accumulate=accumulate)
    _within(gt, ref, 3 * U * mag, 'gradient')
    # rows and columns no window covers: exactly 0 (exactly the old value with accumulate)
    got = gt.detach().cpu().numpy()
    want = old if accumulate else np.zeros_like(old)
    assert np.array_equal(got[:, Ho * kh:], want[:, Ho * kh:]) and np.array_equal(got[:, :, Wo * kw:], want[:, :, Wo * kw:])
    _neighbours_untouched(dbuf)
    _neighbours_untouched(gbuf)


# ------------------------------------------------------------------------------------------------ the head
HN, Hh, Hw, HR = 2, 3, 5, 8
HH, HW = Hh * HR, Hw * HR


def _head_case(C, seed):
    rng = np.random.default_rng(seed)
    cp = (C + 3) // 4 * 4
    z = np.zeros((HN, Hh, Hw, cp))
    z[..., :C] = rng.standard_normal((HN, Hh, Hw, C)) * 3
    z = z.astype(np.float32)
    lab = rng.integers(0, C, (HN, HH, HW)).astype(np.float64)
    lab[rng.uniform(size=lab.shape) < 0.1] = 255
    lab[0, HR:2 * HR, 2 * HR:3 * HR] = 255                    # the block of logit pixel (0, 1, 2): every label ignored
    sw = rng.uniform(0.5, 2.0, (HN, HH, HW)).astype(np.float32)
    return z, lab, sw, cp


def _up(z):
    return np.repeat(np.repeat(z, HR, 1), HR, 2)


def _close(got, want, rtol, atol, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    want = np.asarray(want, np.float64)
    scale = max(1.0, float(np.abs(want).max()))
    assert got.shape == want.shape and np.abs(got - want).max() <= (atol + rtol) * scale, what


def _spec(kind, C, dev=False):
    if kind == 'weighted':
        cw = np.linspace(0.5, 2.0, C).astype(np.float32)
        return ('weighted', torch.from_numpy(cw).to(DEV) if dev else cw.astype(np.float64))
    return ('focal', 2.0, 0.25) if kind == 'focal' else ('ce',)


@pytest.mark.parametrize('C', [2, 4, 21, 150])
@pytest.mark.parametrize('kind', ['ce', 'weighted', 'focal'])
@pytest.mark.parametrize('weights', [False, True])
def test_nearest_head_loss_and_gradient(ops, C, kind, weights):
    z, lab, sw, cp = _head_case(C, C)
    zf = _up(z.astype(np.float64))[..., :C]
    loss_ref, _, g_ref = O.loss_fwd_bwd(zf, lab, _spec(kind, C), 255, sw.astype(np.float64) if weights else None)
    g_low = g_ref.reshape(HN, Hh, HR, Hw, HR, C).sum((2, 4))
    zt = torch.from_numpy(z).to(DEV)
    labels = torch.from_numpy(lab.reshape(HN, HH * HW, 1).astype(np.float32)).to(DEV)
    pw = torch.from_numpy(sw.reshape(HN, HH * HW)).to(DEV) if weights else None
    loss, gz = ops.nearest_head_train(zt, C, HH, HW, labels, 255, loss=_spec(kind, C, dev=True), pixel_weights=pw)
    print('loss', float(loss), loss_ref, 'max |g - g_ref|', float(np.abs(gz[..., :C].cpu().numpy() - g_low).max()))
    _close(loss, [loss_ref], 1e-4, 2e-5, 'loss')
    _close(gz[..., :C], g_low, 1e-4, 1e-9, 'gradient')
    assert C == cp or float(gz[..., C:].abs().max()) == 0.0           # pad channels exactly 0
    assert float(gz[0, 1, 2].abs().max()) == 0.0                      # a block whose labels are all ignored
    # the loss alone, and the gradient added to what the buffer holds
    loss2, none = ops.nearest_head_train(zt, C, HH, HW, labels, 255, loss=_spec(kind, C, dev=True), pixel_weights=pw, want_grad=False)
    assert none is None and torch.equal(loss2, loss)
    old = torch.ones_like(gz)
    ops.nearest_head_train(zt, C, HH, HW, labels, 255, loss=_spec(kind, C, dev=True), pixel_weights=pw, out=old, accumulate=True)
    assert torch.equal(old, gz + 1.0)


@pytest.mark.parametrize('C', [2, 4, 21, 150])
@pytest.mark.parametrize('kind', ['ce', 'weighted', 'focal'])
def test_nearest_head_with_every_label_ignored(ops, C, kind):
    z, lab, sw, cp = _head_case(C, C + 1)
    zt = torch.from_numpy(z).to(DEV)
    labels = torch.full((HN, HH * HW, 1), 255.0, dtype=torch.float32, device=DEV)
    loss, gz = ops.nearest_head_train(zt, C, HH, HW, labels, 255, loss=_spec(kind, C, dev=True),
                                      pixel_weights=torch.from_numpy(sw.reshape(HN, HH * HW)).to(DEV))
    assert float(loss) == 0.0 and float(gz.abs().max()) == 0.0


@pytest.mark.parametrize('C', [2, 4, 21, 150])
def test_nearest_probabilities_argmax_and_counts(ops, C):
    z, lab, _, cp = _head_case(C, 3 * C)
    zf = _up(z)[..., :C]
    _, p_ref, _ = O.loss_fwd_bwd(zf.astype(np.float64), lab, None, 255)
    zt = torch.from_numpy(z).to(DEV)
    labels = torch.from_numpy(lab.reshape(HN, HH * HW, 1).astype(np.float32)).to(DEV)
    probs = ops.nearest_softmax_probs(zt, C, HH, HW)
    assert probs.shape == (HN, HH, HW, C)
    _close(probs, p_ref, 1e-4, 1e-6, 'probs')
    # every pixel of a block holds the block's vector, bit for bit
    pb = probs.view(HN, Hh, HR, Hw, HR, C)
    assert torch.equal(pb, pb[:, :, :1, :, :1].expand_as(pb))
    want = zf.argmax(-1)
    pred, cm = ops.nearest_argmax_confusion(zt, C, HH, HW, labels, want_mask=True)
    assert np.array_equal(pred.cpu().numpy(), want)
    assert np.array_equal(ops.nearest_argmax_confusion(zt, C, HH, HW, want_mask=True)[0].cpu().numpy(), want)
    ref_cm = np.zeros((C, C), np.int64)
    keep = lab != 255
    np.add.at(ref_cm, (lab[keep].astype(np.int64), want[keep]), 1)
    assert np.array_equal(cm.cpu().numpy(), ref_cm)
    counts = ops.nearest_class_counts(zt, C, HH, HW, labels).cpu().numpy()
    cls = np.arange(C)
    li = lab.astype(np.int64).reshape(HN, -1, 1)
    pi = want.reshape(HN, -1, 1)
    ref = np.stack([((li == cls) & (pi == cls)).sum(1), (li == cls).sum(1), (pi == cls).sum(1)], 1)
    assert np.array_equal(counts, ref)
