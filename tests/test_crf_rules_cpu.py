"""The dense-CRF rule of tests/crf_rules.py held to what can be known without a device (closed forms, symmetries, what a CRF is for),
the condition its shared cases have to meet for the GPU comparison to see anything, and the parts of the interface that run without a
GPU."""
import numpy as np
import pytest

import crf_rules
from conftest import load_pkg

CASES = range(len(crf_rules.CASES))


def _flat(H, W, value=128):
    return np.full((H, W, 3), value, np.uint8)


# ------------------------------------------------------------------------------------------------ the rule itself
def test_a_single_label_mask_comes_back_unchanged():
    imgs, masks = crf_rules.case_inputs(len(crf_rules.CASES) - 1)
    out, q = crf_rules.dense_crf(imgs[0], masks[0], 5)
    assert np.array_equal(out, masks[0]) and (q[..., 4] == 1).all() and q.sum() == masks[0].size


def test_class_ids_can_be_permuted_and_unused_classes_do_not_matter():
    imgs, masks = crf_rules.case_inputs(0)                       # classes {0, 2} of 3
    out, q = crf_rules.dense_crf(imgs[0], masks[0], 3)
    perm = np.array([5, 1, 2, 3, 4, 0, 6])                       # 0 <-> 5 among 7 classes
    out7, q7 = crf_rules.dense_crf(imgs[0], perm[masks[0]].astype(np.int32), 7)
    assert np.array_equal(out7, perm[out])
    assert np.allclose(q7[..., 5], q[..., 0], rtol=0, atol=1e-12) and np.allclose(q7[..., 2], q[..., 2], rtol=0, atol=1e-12)
    assert not q7[..., [0, 1, 3, 4, 6]].any()
    out21, q21 = crf_rules.dense_crf(imgs[0], masks[0], 21)      # C beyond the present classes
    assert np.array_equal(out21, out) and np.allclose(q21[..., :3], q, rtol=0, atol=1e-12) and not q21[..., 3:].any()


def test_two_pixels_in_closed_form():
    """pixels (0, 0) and (0, 1) with colours that differ by d in one channel, labels 0 and 1, one iteration"""
    d = 20
    img = np.array([[[100, 100, 100], [100 + d, 100, 100]]], np.uint8)
    mask = np.array([[0, 1]], np.int32)
    _, q = crf_rules.dense_crf(img, mask, 2, iterations=1)
    kg = np.exp(-0.5 / 9)
    kb = np.exp(-0.5 * (1 / 6400 + d * d / 169))
    want = []
    q0 = np.array([[0.7, 0.3], [0.3, 0.7]])
    logit = np.log(q0)
    for w, k in ((3, kg), (10, kb)):
        logit = logit + w * (q0 + k * q0[::-1]) / (1 + k)          # norm_i norm_j = 1 / (1 + k) for both pixels
    e = np.exp(logit)
    want = e / e.sum(1, keepdims=True)
    assert np.allclose(q[0], want, rtol=1e-12, atol=0)


def test_a_wrong_pixel_inside_a_flat_block_is_repaired():
    mask = np.zeros((12, 12), np.int32)
    mask[5, 2] = 1                                               # one wrong label deep inside a block of class 0
    out, q = crf_rules.dense_crf(_flat(12, 12), mask, 2)
    assert not out.any() and q[5, 2, 0] > 0.9


def test_two_blocks_of_distinct_colour_keep_their_border():
    img = _flat(12, 12, 60)
    img[:, 6:] = 160                                             # the colours differ by 100
    mask = np.zeros((12, 12), np.int32)
    mask[:, 6:] = 1
    out, q = crf_rules.dense_crf(img, mask, 2)
    assert np.array_equal(out, mask) and q.max(-1).min() > 0.99


def test_the_bound_on_q_tells_wiring_mistakes_apart():
    """each mistake moves some Q of case 1 by far more than the 2e-3 the device is held to"""
    N, H, W, C, _ = crf_rules.CASES[1]
    imgs, masks = crf_rules.case_inputs(1)
    _, q, _ = crf_rules.case_rule(1)
    for kw in (dict(iterations=4), dict(self_term=False), dict(symmetric=False), dict(count_absent=True)):
        moved = max(np.abs(crf_rules.dense_crf(imgs[b], masks[b], C, **kw)[1] - q[b]).max() for b in range(N))
        assert moved >= 0.05 > crf_rules.Q_ATOL, (kw, moved)


@pytest.mark.parametrize('i', CASES, ids=crf_rules.CASE_IDS)
def test_the_shared_cases_are_ambiguous_but_not_tied(i):
    """the inputs' side of the GPU comparison: Q does not saturate (a saturated Q hides every mistake), float32 arithmetic alone stays
    three orders below the bound, and few pixels are so close to a tie that the device may pick the other class"""
    N, H, W, C, present = crf_rules.CASES[i]
    imgs, masks = crf_rules.case_inputs(i)
    _, q, gap = crf_rules.case_rule(i)
    for b in range(N):
        assert set(np.unique(masks[b])) == present[b]
        if len(present[b]) > 1:
            share = ((q[b] > 0.02) & (q[b] < 0.98)).any(-1).mean()
            assert share >= crf_rules.AMBIGUOUS_MIN, (b, share)
        q32 = crf_rules.dense_crf(imgs[b], masks[b], C, dtype=np.float32)[1]
        assert np.abs(q32 - q[b]).max() <= 2e-6
    assert (gap < crf_rules.NEAR_TIE).mean() <= crf_rules.NEAR_TIE_CAP
    v = crf_rules.case_v(i)
    assert v.shape == (N, H * W, crf_rules.LP) and v.min() >= 0 and not v[..., C:].any()
    for b in range(N):
        assert not v[b][:, [c for c in range(C) if c not in present[b]]].any() and (v[b][:, sorted(present[b])] > 0).all()


def test_messages_are_the_kernel_matrix_products():
    imgs, _ = crf_rules.case_inputs(3)
    v = crf_rules.case_v(3)[0]
    g, b = crf_rules.messages(imgs[0], v)
    kg, kb = crf_rules.kernel_matrices(imgs[0])
    assert (np.diag(kg) == 1).all() and (np.diag(kb) == 1).all() and np.array_equal(kb, kb.T)
    assert np.array_equal(g, kg @ v.astype(np.float64)) and np.array_equal(b, kb @ v.astype(np.float64))
    assert kg[0, 3] == np.exp(-0.5) and (kb <= np.exp(-0.5 * ((np.arange(37)[:, None] - np.arange(37)[None, :]) / 80.0) ** 2)).all()


# ------------------------------------------------------------------------------------------------ the interface, without a device
@pytest.fixture
def classes_file(tmp_path):
    def make(n):
        p = tmp_path / ('classes%d.txt' % n)
        p.write_text('\n'.join('class%d' % c for c in range(n)) + '\n')
        return str(p)
    return make


def _kw(path):
    return dict(model_type='mobilenetv2_lite', model_input_shape=(65, 65), output_stride=16, classes_path=path, weights_path=None)


def test_more_than_32_classes_are_refused_where_the_crf_is_asked_for(classes_file):
    from deeplab import DeepLab
    with pytest.raises(ValueError, match='at most 32 classes'):
        DeepLab(dense_crf=True, **_kw(classes_file(33)))
    assert DeepLab(**_kw(classes_file(33))).crf_params is None           # without the CRF 33 classes are fine
    m = load_pkg().get_deeplabv3p_model('mobilenetv2_lite', 33, (65, 65), 16, training=False)
    with pytest.raises(ValueError, match='at most 32 classes'):
        m.evaluate_miou([], dense_crf=True)
    with pytest.raises(ValueError, match='sigma'):
        DeepLab(dense_crf={'sigma': 3}, **_kw(classes_file(21)))


def test_do_crf_points_to_dense_crf(classes_file):
    from deeplab import DeepLab
    with pytest.raises(ValueError, match='dense_crf=True') as e:
        DeepLab(do_crf=True, **_kw(classes_file(21)))
    assert 'lattice' in str(e.value) and 'not built' in str(e.value)


def test_the_defaults_keep_the_crf_off(classes_file):
    import inspect
    from deeplab import DeepLab
    assert DeepLab._defaults['dense_crf'] is False and DeepLab._defaults['do_crf'] is False
    d = DeepLab(**_kw(classes_file(21)))
    assert d.dense_crf is False and d.crf_params is None
    assert DeepLab(dense_crf=True, **_kw(classes_file(21))).crf_params == {}
    assert DeepLab(dense_crf={'iterations': 3}, **_kw(classes_file(21))).crf_params == {'iterations': 3}
    model = load_pkg('model')
    assert inspect.signature(model.DeeplabModel.evaluate_miou).parameters['dense_crf'].default is False
    ops = load_pkg('ops')
    sig = inspect.signature(ops.dense_crf).parameters
    want = dict(iterations=5, gt_prob=0.7, sxy_gaussian=(3, 3), compat_gaussian=3, sxy_bilateral=80, srgb=13, compat_bilateral=10,
                want_q=False)
    assert {k: sig[k].default for k in want} == want


# ------------------------------------------------------------------------------------------------ the edge cases and their bounds
# (tests/test_crf_edges_gpu.py holds the device to these; here the inputs meet their conditions, honest float32 arithmetic in two
# summation orders stays inside every per-element bound, and each planted mistake leaves it by a factor of ten or more)
EDGES = range(len(crf_rules.EDGE_CASES))
F32 = np.float32


def _ambiguous_share(q):
    return ((q > 0.02) & (q < 0.98)).any(-1).mean()


@pytest.mark.parametrize('i', EDGES, ids=crf_rules.EDGE_IDS)
def test_the_edge_cases_are_ambiguous_but_not_tied(i):
    """as test_the_shared_cases_are_ambiguous_but_not_tied; the float32 rule stays two orders below Q_ATOL"""
    N, H, W, C, present, kw = crf_rules.EDGE_CASES[i]
    imgs, masks = crf_rules.edge_inputs(i)
    _, q, gap = crf_rules.edge_rule(i)
    for b in range(N):
        assert set(np.unique(masks[b])) == present[b]
        assert _ambiguous_share(q[b]) >= crf_rules.AMBIGUOUS_MIN, (b, _ambiguous_share(q[b]))
        q32 = crf_rules.dense_crf(imgs[b], masks[b], C, dtype=np.float32, **kw)[1]
        assert np.abs(q32 - q[b]).max() <= 2e-5
    assert (gap < crf_rules.NEAR_TIE).mean() <= crf_rules.NEAR_TIE_CAP


def test_the_scene_with_ids_outside_the_classes_meets_the_same_conditions():
    N, H, W, C, present, kw = crf_rules.EDGE_CASES[crf_rules.OUTSIDE_BASE]
    imgs, masks = crf_rules.outside_inputs()
    out, q, gap = crf_rules.outside_rule()
    outside = (masks < 0) | (masks >= C)
    assert outside.sum() == 12 and set(np.unique(masks[outside])) == set(crf_rules.OUTSIDE_IDS)
    assert _ambiguous_share(q[0]) >= crf_rules.AMBIGUOUS_MIN and (gap < crf_rules.NEAR_TIE).mean() <= crf_rules.NEAR_TIE_CAP
    assert ((out >= 0) & (out < C)).all()                                 # every pixel gets a class, those included
    assert np.abs(crf_rules.dense_crf(imgs[0], masks[0], C, dtype=np.float32, **kw)[1] - q[0]).max() <= 2e-5
    # the planted mistake: the pixel counted as a class (n_labels = 3 where 2 are present)
    moved = np.abs(crf_rules.dense_crf(imgs[0], masks[0], C, count_outside=True, **kw)[1] - q[0]).max()
    assert moved >= 10 * crf_rules.Q_ATOL, moved
    # fewer than two present classes: unchanged, such ids included
    one = np.where(outside[0], masks[0], 1).astype(np.int32)
    back, q1 = crf_rules.dense_crf(imgs[0], one, C, **kw)
    assert np.array_equal(back, one) and (q1[..., 1] == 1).all() and not q1[..., 0].any()
    none = np.full_like(one, 255)
    back, q0 = crf_rules.dense_crf(imgs[0], none, C, **kw)
    assert np.array_equal(back, none) and not q0.any()


def _sequential(terms):
    """(rows, n, L) float32 -> the sums over axis 1 added front to back and back to front, in float32"""
    assert terms.dtype == F32
    return np.cumsum(terms, axis=1, dtype=F32)[:, -1], np.cumsum(terms[:, ::-1], axis=1, dtype=F32)[:, -1]


def _gauss_k32(H, W, sx, sy):
    """the Gaussian kernel as float32 arithmetic forms it: two table entries exp(-(d d) fl(1 / 2 s^2)) and their product"""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    dx, dy = np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :])
    tx = np.exp(-(dx * dx).astype(F32) * F32(0.5 / (sx * sx)))
    ty = np.exp(-(dy * dy).astype(F32) * F32(0.5 / (sy * sy)))
    assert tx.dtype == F32
    return tx * ty


def _bilateral_k32(img, sxy, srgb):
    """the bilateral kernel in float32: exact integer distances, two scalings to base 2, their sum, exp2"""
    H, W, _ = img.shape
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1).astype(np.int64), y.reshape(-1).astype(np.int64)
    rgb = img.reshape(-1, 3).astype(np.int64)
    d2 = ((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2).astype(F32)
    c2 = ((rgb[:, None, :] - rgb[None, :, :]) ** 2).sum(-1).astype(F32)
    log2e = 1.4426950408889634
    k = np.exp2(c2 * F32(-0.5 * log2e / (srgb * srgb)) + d2 * F32(-0.5 * log2e / (sxy * sxy)))
    assert k.dtype == F32
    return k


def _inside(got, want, bound):
    """the largest |got - want| / bound; elements with a zero bound must be met exactly"""
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bound == 0] == 0).all()
    return (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0


def _norm32(s):
    return F32(1) / np.sqrt(s + F32(1e-20))


COLS = list(crf_rules.PRESENT_COLUMNS)


@pytest.mark.parametrize('k', range(len(crf_rules.GAUSS_SHAPES)), ids=['%dx%d' % s[:2] for s in crf_rules.GAUSS_SHAPES])
def test_float32_gaussian_messages_and_normalisers_stay_inside_their_bounds(k):
    H, W, sx, sy = crf_rules.GAUSS_SHAPES[k]
    n = H * W
    a = crf_rules.gauss_exponents(H, W, (sx, sy))
    k32 = _gauss_k32(H, W, sx, sy)
    worst = 0.0
    for v in crf_rules.message_v(300 + k, 2, n):                      # the inputs of the device test
        for scale in (None, crf_rules.message_scale(400 + k, n)):
            want = np.exp(a) @ crf_rules._scaled(v, scale)
            bound = crf_rules.message_bound(a, v, scale)
            sv = v[:, COLS] if scale is None else v[:, COLS] * scale[:, None]
            for got in _sequential(k32[:, :, None] * sv[None]):
                worst = max(worst, _inside(got, want[:, COLS], bound[:, COLS]))
    nrm = max(_inside(_norm32(s[:, 0]), crf_rules.gauss_norm(H, W, (sx, sy)), crf_rules.norm_bound(a))
              for s in _sequential(k32[:, :, None]))
    print('%d x %d: float32 message error / bound %.3f, normaliser %.3f' % (H, W, worst, nrm))
    assert worst <= 1 and nrm <= 1


@pytest.mark.parametrize('kind', sorted(crf_rules.BILATERAL_KINDS))
@pytest.mark.parametrize('k', range(len(crf_rules.BILATERAL_SHAPES)), ids=['%dx%d' % s for s in crf_rules.BILATERAL_SHAPES])
def test_float32_bilateral_messages_and_normalisers_stay_inside_their_bounds(k, kind):
    H, W = crf_rules.BILATERAL_SHAPES[k]
    n = H * W
    sxy, srgb = crf_rules.BILATERAL_KINDS[kind]
    img = crf_rules.bilateral_image(kind, 500 + k, 2, H, W)
    v = crf_rules.message_v(600 + k, 2, n)
    scale = crf_rules.message_scale(700 + k, 2, n)
    worst = nrm = 0.0
    for b in range(2):
        a = crf_rules.bilateral_exponents(img[b], sxy, srgb)
        k32 = _bilateral_k32(img[b], sxy, srgb)
        assert np.isfinite(k32).all()
        want = np.exp(a) @ crf_rules._scaled(v[b], scale[b])
        bound = crf_rules.message_bound(a, v[b], scale[b])
        for got in _sequential(k32[:, :, None] * (v[b][:, COLS] * scale[b][:, None])[None]):
            worst = max(worst, _inside(got, want[:, COLS], bound[:, COLS]))
        for s in _sequential(k32[:, :, None]):
            nrm = max(nrm, _inside(_norm32(s[:, 0]), crf_rules.bilateral_norm(img[b], sxy, srgb), crf_rules.norm_bound(a)))
    print('%d x %d %s: float32 message error / bound %.3f, normaliser %.3f' % (H, W, kind, worst, nrm))
    assert worst <= 1 and nrm <= 1


def _update32(mask, C, fg, ng, fb, nb, wg, wb, gt, reverse):
    """one update in float32, the sum of the exponentials front to back or back to front"""
    m = mask.astype(np.int64)
    n = m.size
    inside, present = crf_rules._present(m, C)
    nl = int(present.sum())
    logit = np.full((n, C), np.log(F32(F32(1) - F32(gt)) / F32(nl - 1)), F32)
    logit[np.arange(n)[inside], m[inside]] = np.log(F32(gt))
    logit = logit + (F32(wg) * ng)[:, None] * fg[:, :C]
    logit = logit + (F32(wb) * nb)[:, None] * fb[:, :C]
    x = logit[:, present] - logit[:, present].max(axis=1, keepdims=True)
    e = np.exp2(x * F32(1.4426950408889634))
    s = np.cumsum(e[:, ::-1] if reverse else e, axis=1, dtype=F32)[:, -1:]
    q = np.zeros((n, C), F32)
    q[:, present] = e / s
    assert logit.dtype == F32 and e.dtype == F32
    return q


@pytest.mark.parametrize('name', sorted(crf_rules.UPDATE_CASES))
def test_float32_updates_stay_inside_their_bounds_and_few_pixels_are_near_ties(name):
    N, n, C, ids, gt, wg, wb = crf_rules.UPDATE_CASES[name]
    mask, fg, ng, fb, nb = crf_rules.update_inputs(name)
    for b in range(N):
        assert set(np.unique(mask[b])) == set(ids[b])
        args = (mask[b], C, fg[b], ng, fb[b], nb[b], wg, wb, gt)
        q, arg, gap = crf_rules.update(*args)
        bound = crf_rules.update_bound(*args)
        present = sorted(c for c in ids[b] if 0 <= c < C)
        absent = [c for c in range(C) if c not in present]
        assert not q[:, absent].any() and not bound[:, absent].any()
        if len(present) < 2:
            assert np.array_equal(arg, mask[b]) and np.isinf(gap).all() and (q[:, present] == 1).all()
            continue
        assert np.allclose(q.sum(1), 1, rtol=0, atol=1e-12) and ((arg >= 0) & (arg < C)).all()
        worst = max(_inside(_update32(*args, reverse=r), q, bound) for r in (False, True))
        near = (gap <= 2 * bound.max(axis=1)).mean()
        print('%s image %d: float32 error / bound %.3f; near-tie share %.2e; largest bound %.2e' % (name, b, worst, near, bound.max()))
        assert worst <= 1 and near <= crf_rules.NEAR_TIE_CAP
        # the planted mistake: the two weights swapped
        moved = np.abs(crf_rules.update(mask[b], C, fg[b], ng, fb[b], nb[b], wb, wg, gt)[0] - q) / np.maximum(bound, 1e-300)
        assert moved[:, present].max() >= 10


def test_a_gt_prob_below_one_half_moves_the_unary_argmax_off_the_pixels_own_class():
    N, n, C, ids, gt, wg, wb = crf_rules.UPDATE_CASES['gt-0.3']
    mask = crf_rules.update_inputs('gt-0.3')[0][0]
    q, arg, gap = crf_rules.update(mask, C, None, None, None, None, 0, 0, gt)
    lo, hi = ids[0]
    assert np.array_equal(arg, np.where(mask == lo, hi, lo)) and np.allclose(gap, 0.4, rtol=0, atol=1e-12)
    assert np.allclose(q[np.arange(n), mask], 0.3, rtol=0, atol=1e-12)
    assert np.array_equal(crf_rules.dense_crf(np.zeros((1, n, 3), np.uint8), mask[None], C, iterations=0, gt_prob=gt)[0][0], arg)
    assert np.array_equal(crf_rules.dense_crf(np.zeros((1, n, 3), np.uint8), mask[None], C, iterations=0)[0][0], mask)


def test_update_is_one_step_of_the_rule():
    i = 1                                                           # 70 x 6, one iteration
    N, H, W, C, present, kw = crf_rules.EDGE_CASES[i]
    imgs, masks = crf_rules.edge_inputs(i)
    _, want, _ = crf_rules.edge_rule(i)
    m = masks[0].reshape(-1)
    q0 = crf_rules.update(m, C, None, None, None, None, 0, 0, 0.7)[0]
    ng, nb = crf_rules.gauss_norm(H, W, kw['sxy_gaussian']), crf_rules.bilateral_norm(imgs[0])
    fg, fb = crf_rules.messages(imgs[0], q0, scale=(ng, nb), sxy_gaussian=kw['sxy_gaussian'])
    q1, arg, gap = crf_rules.update(m, C, fg, ng, fb, nb, 3, 10, 0.7)
    assert np.allclose(q1.reshape(H, W, C), want[0], rtol=0, atol=1e-14)
    assert np.array_equal(gap.reshape(H, W), crf_rules.top_two_gap(q1).reshape(H, W))


# ---- planted mistakes: each moves some checked element by at least ten times its bound on the case meant to catch it
def _moved(wrong, want, bound, cols=COLS):
    return (np.abs(wrong - want)[:, cols] / bound[:, cols]).max()


def test_swapped_sigmas_leave_the_bounds():
    N, H, W, C, present, kw = crf_rules.EDGE_CASES[0]                # 5 x 70: sx, sy = 5, 2; sxy_bilateral, srgb = 40, 20
    img = crf_rules.edge_inputs(0)[0][0]
    n = H * W
    v = crf_rules.message_v(800, 1, n)[0]
    sg, sb, srgb = kw['sxy_gaussian'], kw['sxy_bilateral'], kw['srgb']
    g, b = crf_rules.messages(img, v, sxy_gaussian=sg, sxy_bilateral=sb, srgb=srgb)
    wg, wb = crf_rules.messages(img, v, sxy_gaussian=sg[::-1], sxy_bilateral=srgb, srgb=sb)
    rel = np.abs(wg - g)[:, COLS] / g[:, COLS]
    print('sx <-> sy moves the 5 x 70 Gaussian message by %.2f .. %.2f per element' % (rel.min(), rel.max()))
    assert rel.min() >= 0.05
    assert _moved(wg, g, crf_rules.message_bound(crf_rules.gauss_exponents(H, W, sg), v)) >= 10
    assert _moved(wb, b, crf_rules.message_bound(crf_rules.bilateral_exponents(img, sb, srgb), v)) >= 10
    a = crf_rules.gauss_exponents(H, W, sg)
    assert (np.abs(crf_rules.gauss_norm(H, W, sg[::-1]) - crf_rules.gauss_norm(H, W, sg)) / crf_rules.norm_bound(a)).max() >= 10
    a = crf_rules.bilateral_exponents(img, sb, srgb)
    assert (np.abs(crf_rules.bilateral_norm(img, srgb, sb) - crf_rules.bilateral_norm(img, sb, srgb)) / crf_rules.norm_bound(a)).max() >= 10
    # every Gaussian shape of the device test with two sides tells the two sigmas apart
    for H, W, sx, sy in crf_rules.GAUSS_SHAPES:
        if H > 1 and W > 1:
            a = crf_rules.gauss_exponents(H, W, (sx, sy))
            v = crf_rules.message_v(801, 1, H * W)[0]
            assert _moved(np.exp(crf_rules.gauss_exponents(H, W, (sy, sx))) @ v, np.exp(a) @ v, crf_rules.message_bound(a, v)) >= 10


@pytest.mark.parametrize('k', range(1, len(crf_rules.BILATERAL_SHAPES)), ids=['%dx%d' % s for s in crf_rules.BILATERAL_SHAPES[1:]])
def test_a_wrong_scale_leaves_the_bounds(k):
    """dropped, applied to pixel i where it belongs to pixel j, image 0's used for image 1 -- on the inputs of the device test"""
    H, W = crf_rules.BILATERAL_SHAPES[k]
    n = H * W
    for kind, (sxy, srgb) in sorted(crf_rules.BILATERAL_KINDS.items()):
        img = crf_rules.bilateral_image(kind, 500 + k, 2, H, W)
        v = crf_rules.message_v(600 + k, 2, n)[1].astype(np.float64)
        scale = crf_rules.message_scale(700 + k, 2, n).astype(np.float64)
        a = crf_rules.bilateral_exponents(img[1], sxy, srgb)
        K = np.exp(a)
        want, bound = K @ (v * scale[1][:, None]), crf_rules.message_bound(a, v, scale[1])
        for wrong in (K @ v, scale[1][:, None] * (K @ v), K @ (v * scale[0][:, None])):
            assert _moved(wrong, want, bound) >= 10
    # the Gaussian's scale on its own shapes
    for j, (H, W, sx, sy) in enumerate(crf_rules.GAUSS_SHAPES[1:], 1):
        a = crf_rules.gauss_exponents(H, W, (sx, sy))
        v = crf_rules.message_v(300 + j, 2, H * W)[0].astype(np.float64)
        s = crf_rules.message_scale(400 + j, H * W).astype(np.float64)
        want, bound = np.exp(a) @ (v * s[:, None]), crf_rules.message_bound(a, v, s)
        for wrong in (np.exp(a) @ v, s[:, None] * (np.exp(a) @ v)):
            assert _moved(wrong, want, bound) >= 10


def test_a_source_position_dropped_at_the_chunk_boundary_leaves_the_bounds():
    """position t = 64 of a line, the first of the second chunk, left out of the sum"""
    for k, (H, W, sx, sy) in enumerate(crf_rules.GAUSS_SHAPES):
        if max(H, W) <= 64:
            continue
        y, x = np.mgrid[0:H, 0:W]
        along = (x if W > 64 else y).reshape(-1)
        a = crf_rules.gauss_exponents(H, W, (sx, sy))
        v = crf_rules.message_v(300 + k, 2, H * W)[0].astype(np.float64)
        K = np.exp(a)
        dropped = K.copy()
        dropped[:, along == 64] = 0
        assert _moved(dropped @ v, K @ v, crf_rules.message_bound(a, v)) >= 10, (H, W)


def test_swapped_weights_and_a_missing_iteration_leave_the_end_to_end_bound():
    for i in EDGES:
        N, H, W, C, present, kw = crf_rules.EDGE_CASES[i]
        imgs, masks = crf_rules.edge_inputs(i)
        _, q, _ = crf_rules.edge_rule(i)
        full = dict(dict(iterations=5, compat_gaussian=3, compat_bilateral=10), **kw)
        wrongs = [dict(full, iterations=full['iterations'] - 1),
                  dict(full, compat_gaussian=full['compat_bilateral'], compat_bilateral=full['compat_gaussian'])]
        for wrong in wrongs:
            moved = max(np.abs(crf_rules.dense_crf(imgs[b], masks[b], C, **wrong)[1] - q[b]).max() for b in range(N))
            assert moved >= 10 * crf_rules.Q_ATOL, (crf_rules.EDGE_IDS[i], wrong, moved)
