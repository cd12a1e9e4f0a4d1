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
