"""Dense-CRF post-processing on the device against the float64 rule of tests/crf_rules.py: the two message sums per element, the
mean-field result end to end, exact ties and single-label masks, bitwise identities between ways of launching it, and the Python layers
(DeepLab(dense_crf=True), evaluate_miou(dense_crf=True)) on a small random model."""
import numpy as np
import pytest
import torch

import crf_rules
from conftest import load_pkg

pytestmark = pytest.mark.gpu
CASES = range(len(crf_rules.CASES))
LP = crf_rules.LP
SENTINEL = -7.25


def _dev(i):
    imgs, masks = crf_rules.case_inputs(i)
    return torch.from_numpy(imgs.copy()).cuda(), torch.from_numpy(masks.copy()).cuda()


# ------------------------------------------------------------------------------------------------ messages, per element
@pytest.mark.parametrize('i', CASES, ids=crf_rules.CASE_IDS)
def test_messages_equal_the_kernel_matrix_product(ops, i):
    """rtol (n + 64) 2^-24, no atol: every term is non-negative, so a length-n fp32 accumulation is within n 2^-24 of its sum; the 64
    covers a few ulp each for the feature arithmetic and the exp"""
    N, H, W, C, present = crf_rules.CASES[i]
    n = H * W
    imgs, _ = crf_rules.case_inputs(i)
    v = crf_rules.case_v(i)
    wide = torch.full((N, n, LP + 8), SENTINEL, dtype=torch.float32, device='cuda')       # V is the first 32 columns of 40
    wide[..., :LP] = torch.from_numpy(v).cuda()
    guard = 256
    bufs = [torch.full((N * n * LP + guard,), SENTINEL, dtype=torch.float32, device='cuda') for _ in range(2)]
    out = tuple(b[:N * n * LP].view(N, n, LP) for b in bufs)
    g, b = ops.crf_messages(torch.from_numpy(imgs.copy()).cuda(), wide[..., :LP], out=out)
    assert g.data_ptr() == bufs[0].data_ptr() and b.data_ptr() == bufs[1].data_ptr()
    rtol = (n + 64) * 2.0 ** -24
    for name, got, buf in (('gaussian', g, bufs[0]), ('bilateral', b, bufs[1])):
        got = got.cpu().numpy().astype(np.float64)
        for k in range(N):
            want = crf_rules.messages(imgs[k], v[k])[0 if name == 'gaussian' else 1]
            cols = sorted(present[k])
            rel = np.abs(got[k][:, cols] - want[:, cols]) / want[:, cols]
            print('case %s image %d %s: max relative error %.3e (bound %.3e)' % (crf_rules.CASE_IDS[i], k, name, rel.max(), rtol))
            assert (want[:, cols] > 0).all() and rel.max() <= rtol
            absent = [c for c in range(LP) if c not in present[k]]
            assert not got[k][:, absent].any()                      # absent and padding columns: exactly 0
        assert (buf[N * n * LP:] == SENTINEL).all()                 # the guard band behind the output
    assert (wide[..., LP:] == SENTINEL).all()                       # columns of V beyond the 32


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('i', CASES, ids=crf_rules.CASE_IDS)
def test_q_and_mask_follow_the_rule(ops, i):
    """|Q_device - Q_rule| <= 2e-3 on every entry (worst-case linear bound 1/4 * 13 * 3 (n + 64) 2^-24 ~ 6.5e-4 per step at n ~ 1000,
    5 steps; 4 iterations instead of 5, a dropped self term, an asymmetric normalisation or absent classes counted in n_labels move Q
    by 0.05 to 0.98: test_crf_rules_cpu).  The masks agree wherever the rule's two best Q are at least NEAR_TIE apart."""
    N, H, W, C, _ = crf_rules.CASES[i]
    want_mask, want_q, gap = crf_rules.case_rule(i)
    img, mask = _dev(i)
    got_mask, got_q = ops.dense_crf(img, mask, C, want_q=True)
    assert got_mask.shape == (N, H, W) and got_mask.dtype == torch.int32 and got_q.shape == (N, H, W, C)
    got_q = got_q.cpu().numpy()
    err = np.abs(got_q - want_q)
    clear = gap >= crf_rules.NEAR_TIE
    got_mask = got_mask.cpu().numpy()
    print('case %s: max |Q - rule| %.3e; near-tie share %.2e, mask mismatch share %.2e' % (
        crf_rules.CASE_IDS[i], err.max(), 1 - clear.mean(), (got_mask != want_mask).mean()))
    assert err.max() <= crf_rules.Q_ATOL
    assert 1 - clear.mean() <= crf_rules.NEAR_TIE_CAP
    assert np.array_equal(got_mask[clear], want_mask[clear])
    assert np.array_equal(ops.dense_crf(img, mask, C).cpu().numpy(), got_mask)              # without Q: the same mask


def test_absent_and_padding_columns_of_q_are_exactly_zero(ops):
    i = 1
    N, H, W, C, present = crf_rules.CASES[i]
    img, mask = _dev(i)
    _, q = ops.dense_crf(img, mask, C, want_q=True)
    q = q.cpu().numpy()
    for k in range(N):
        absent = [c for c in range(C) if c not in present[k]]
        assert not q[k][..., absent].any() and (q[k][..., sorted(present[k])] > 0).all()
    assert np.allclose(q.sum(-1), 1, atol=1e-6)


# ------------------------------------------------------------------------------------------------ ties and degenerate masks
@pytest.mark.parametrize('lo,hi,C', [(3, 7, 21), (0, 1, 2)], ids=['3-7-of-21', '0-1-of-2'])
def test_an_exact_tie_gives_the_lower_class_id(ops, lo, hi, C):
    """a left/right-symmetric grey image, the left half labelled `hi` and the right half `lo` (mirrored evidence), with gt_prob = 0.5:
    the unary term then ties the two present classes exactly, their columns of every message hold the same numbers summed in the same
    order, and Q stays (0.5, 0.5) bit for bit at every pixel.  (With the default gt_prob no pixel can tie bit for bit: a pixel is never
    its own mirror image in both classes, and the messages of two mirrored pixels add the same terms in opposite orders.)"""
    H, W = 12, 16
    img = np.full((H, W, 3), 128, np.uint8)
    img[:, 3:5] = img[:, W - 5:W - 3] = 90
    mask = np.full((H, W), hi, np.int32)
    mask[:, W // 2:] = lo
    got, q = ops.dense_crf(torch.from_numpy(img)[None].cuda(), torch.from_numpy(mask)[None].cuda(), C, gt_prob=0.5, want_q=True)
    q = q[0].cpu().numpy()
    assert np.array_equal(q[..., lo], q[..., hi]) and (q[..., lo] == 0.5).all()
    assert (got.cpu().numpy() == lo).all()


def test_a_single_label_mask_comes_back_bit_for_bit(ops):
    i = len(crf_rules.CASES) - 1
    N, H, W, C, present = crf_rules.CASES[i]
    img, mask = _dev(i)
    got, q = ops.dense_crf(img, mask, C, want_q=True)
    assert torch.equal(got, mask) and got.data_ptr() != mask.data_ptr()
    q = q.cpu().numpy()
    only = next(iter(present[0]))
    assert (q[..., only] == 1).all() and q.sum() == N * H * W


def test_more_than_32_classes_are_refused(ops):
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device='cuda')
    mask = torch.zeros((1, 4, 4), dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='32'):
        ops.dense_crf(img, mask, 33)


# ------------------------------------------------------------------------------------------------ launch variants
def test_a_batch_equals_its_images_run_alone(ops):
    i = 1
    N, H, W, C, _ = crf_rules.CASES[i]
    img, mask = _dev(i)
    both, qb = ops.dense_crf(img, mask, C, want_q=True)
    for k in range(N):
        one, q1 = ops.dense_crf(img[k:k + 1].contiguous(), mask[k:k + 1].contiguous(), C, want_q=True)
        assert torch.equal(one[0], both[k]) and torch.equal(q1[0].view(torch.int32), qb[k].view(torch.int32))


def test_another_stream_and_a_reused_workspace_change_no_bit(ops):
    i = 2
    N, H, W, C, _ = crf_rules.CASES[i]
    img, mask = _dev(i)
    first, q1 = ops.dense_crf(img, mask, C, want_q=True)
    again, q2 = ops.dense_crf(img, mask, C, want_q=True)                # the buffers of the first call
    assert torch.equal(first, again) and torch.equal(q1.view(torch.int32), q2.view(torch.int32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other, q3 = ops.dense_crf(img, mask, C, want_q=True)
    side.synchronize()
    assert torch.equal(first, other) and torch.equal(q1.view(torch.int32), q3.view(torch.int32))


# ------------------------------------------------------------------------------------------------ front end
NC, H0, W0 = 21, 65, 65
FRAME = (48, 80)


def _randomise(m, seed=3):
    """non-trivial BatchNorm parameters, moving statistics and biases, so that the random model predicts several classes"""
    rng = np.random.default_rng(seed)
    w = m.get_weights_by_name()
    for k, v in w.items():
        if k.endswith('/gamma') or k.endswith('/moving_variance'):
            w[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith('/beta') or k.endswith('/moving_mean') or k.endswith('/bias'):
            w[k] = (rng.standard_normal(v.shape) * 0.1).astype(np.float32)
    m.set_weights_by_name(w)


@pytest.fixture(scope='module')
def front(ops, tmp_path_factory):
    """a DeepLab with the CRF, one without it on the same weights, one frame, its resized bytes, and the rule's kernel matrices"""
    inf = load_pkg('inference')
    classes = tmp_path_factory.mktemp('crf') / 'classes.txt'
    classes.write_text('\n'.join('class%d' % c for c in range(NC)) + '\n')
    kw = dict(model_type='mobilenetv2_lite', model_input_shape=(H0, W0), output_stride=16, classes_path=str(classes), weights_path=None)
    d = inf.DeepLab(dense_crf=True, **kw)
    m = d.deeplab_model
    _randomise(m)
    # a soft two-tone frame with noise: the colours must not decide every pixel
    rng = np.random.default_rng(21)
    frame = np.full(FRAME + (3,), 120.0)
    frame[:, FRAME[1] // 2:] += 14
    frame = np.clip(np.rint(frame + rng.normal(0, 10, frame.shape)), 0, 255).astype(np.uint8)
    resized = load_pkg('augment').pil_resize(torch.from_numpy(frame)[None].cuda(), (H0, W0))
    # a random model's logits are one constant vector plus a small spatial part, so it predicts one class everywhere and the CRF has
    # nothing to do: take the mean log-probability of every class out of the last bias, and the spatial part decides
    w = m.get_weights_by_name()
    w['conv_upsample/bias'] = w['conv_upsample/bias'] - np.log(m.predict(resized)).reshape(-1, NC).mean(0).astype(np.float32)
    m.set_weights_by_name(w)
    plain = inf.DeepLab(**kw)
    plain.deeplab_model.set_weights(m.get_weights())
    kernels = crf_rules.kernel_matrices(resized[0].cpu().numpy())
    return inf, d, plain, frame, resized, kernels


def _rule_at_frame_size(inf, resized, ids, kernels):
    """mask_resize of the rule on (resized bytes, class ids), and of the pixels the rule decides clearly"""
    want, q = crf_rules.dense_crf(resized[0].cpu().numpy(), ids, NC, kernels=kernels)
    clear = crf_rules.top_two_gap(q) >= crf_rules.NEAR_TIE
    size = (FRAME[1], FRAME[0])
    return inf.mask_resize(want, size), inf.mask_resize(clear.astype(np.int32), size).astype(bool), want, clear


def test_predict_and_segment_batch_refine_the_models_class_ids(front):
    inf, d, plain, frame, resized, kernels = front
    ids = d.deeplab_model.predict_mask(resized)[0]
    assert len(np.unique(ids)) >= 2, 'the random model predicts one class: the CRF has nothing to do'
    want, clear, want_small, clear_small = _rule_at_frame_size(inf, resized, ids, kernels)
    print('classes %s; near-tie share %.2e; the CRF changes %.3f of the pixels' % (np.unique(ids), 1 - clear_small.mean(),
                                                                               (want_small != ids).mean()))
    assert 1 - clear_small.mean() <= crf_rules.NEAR_TIE_CAP
    got = d.predict(resized, FRAME)
    assert got.shape == FRAME and got.dtype == np.uint8 and np.array_equal(got[clear], want[clear])
    masks, overlays = d.segment_batch(frame[None])
    assert np.array_equal(masks[0].cpu().numpy(), got) and overlays.shape == (1,) + FRAME + (3,)
    # normalised float32 input: the bytes come back by denormalize_image, truncation included
    x = resized.cpu().numpy().astype(np.float32) / np.float32(127.5) - np.float32(1)
    back = (x * np.float32(127.5) + np.float32(127.5)).astype(np.uint8)
    ops = load_pkg('ops')
    assert np.array_equal(ops.denormalize_u8(torch.from_numpy(x).cuda()).cpu().numpy(), back)
    refined = ops.dense_crf(torch.from_numpy(back).cuda(), torch.from_numpy(d.deeplab_model.predict_mask(x)).cuda(), NC)
    assert np.array_equal(d.predict(x, FRAME), inf.mask_resize(refined[0].cpu().numpy(), (FRAME[1], FRAME[0])))


def test_the_crf_refines_the_multi_scale_mask(front):
    inf, d, plain, frame, resized, kernels = front
    kw = dict(scales=(0.5, 1.0), flip=True)
    ids = d.deeplab_model.class_ids(resized, **kw)[0].cpu().numpy()
    want, clear, _, clear_small = _rule_at_frame_size(inf, resized, ids, kernels)
    assert 1 - clear_small.mean() <= crf_rules.NEAR_TIE_CAP
    d.scales, d.flip = d.deeplab_model.tta_scales(kw['scales']), True
    try:
        got = d.predict(resized, FRAME)
    finally:
        d.scales, d.flip = (1.0,), False
    assert np.array_equal(got[clear], want[clear])


def test_evaluate_miou_counts_the_refined_masks(front, ops):
    inf, d, plain, frame, resized, kernels = front
    m = d.deeplab_model
    frames = np.concatenate([resized.cpu().numpy(), resized.cpu().numpy()[:, ::-1].copy()])
    lab = np.random.default_rng(6).integers(0, NC, (2, H0 * W0, 1)).astype(np.uint8)
    lab[0, :50, 0] = 255
    refined = ops.dense_crf(torch.from_numpy(frames).cuda(), m.class_ids(frames), NC).cpu().numpy().reshape(-1)
    want = np.zeros((NC, NC), np.int64)
    ok = lab.reshape(-1) < NC
    np.add.at(want, (lab.reshape(-1)[ok].astype(np.int64), refined[ok]), 1)
    res = m.evaluate_miou([(frames, lab)], dense_crf=True)
    assert np.array_equal(res['confusion_matrix'], want.astype(np.float64)) and want.sum() == 2 * H0 * W0 - 50
    with pytest.raises(ValueError, match='uint8'):
        m.evaluate_miou([(frames.astype(np.float32), lab)], dense_crf=True)


def test_without_dense_crf_nothing_changes(front):
    inf, d, plain, frame, resized, kernels = front
    assert plain.dense_crf is False and plain.crf_params is None
    m = plain.deeplab_model
    ids = m.predict_mask(resized)
    assert np.array_equal(plain.predict(resized, FRAME), inf.mask_resize(ids[0], (FRAME[1], FRAME[0])))
    frames = resized.cpu().numpy()
    lab = np.random.default_rng(5).integers(0, NC, (1, H0 * W0, 1)).astype(np.uint8)
    cm = torch.zeros(NC * NC, dtype=torch.int64, device='cuda')
    ex = m._executor(1, False)
    ex.set_inputs(frames, lab)
    ex.eval_step(cm)
    today = cm.view(NC, NC).cpu().numpy().astype(np.float64)
    for kw in ({}, dict(dense_crf=False)):
        assert np.array_equal(m.evaluate_miou([(frames, lab)], **kw)['confusion_matrix'], today)
