"""The inference front end on the device, bit for bit against tests/pil_rules.py (which tests/test_infer_io_cpu.py holds to Pillow):
augment.pil_resize = PIL's Image.resize(size, BICUBIC), dl3p_mask_overlay_u8 = mask_resize + colour map + blend in one launch, and
DeepLab.segment_batch / predict / segment_image against the host chain around the same forward pass.  No tolerances anywhere.

Sizes are the smallest at which each path can go wrong: taps cut at both borders with fewer taps than coefficients, a non-integer
shrink, each pass alone, the copy, output rows of 3 W bytes that are and are not a multiple of 4 (the vertical pass and the overlay read
32 bits per lane where alignment allows, bytes otherwise), widths that are no multiple of the 64-column tile, and 65 coefficients."""
import numpy as np
import pytest
import torch

import pil_rules
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CASE_IDS = ['%dx%d-%dx%d' % (hw + HW) for hw, HW in pil_rules.CASES]
_want = {}


def want(hw, HW, kind, seed=0):
    """the restated resize of a seeded input, computed once per session"""
    key = (hw, HW, kind, seed)
    if key not in _want:
        x = pil_rules.case_input(hw, kind, seed)
        _want[key] = (x, pil_rules.resize_bicubic(x, HW))
    return _want[key]


@pytest.fixture(scope='module')
def aug(ops):
    return load_pkg('augment')


# ------------------------------------------------------------------------------------------------ pil_resize
@pytest.mark.parametrize('kind', pil_rules.KINDS)
@pytest.mark.parametrize('hw,HW', pil_rules.CASES, ids=CASE_IDS)
def test_pil_resize_equals_the_restatement(aug, hw, HW, kind):
    x, ref = want(hw, HW, kind)
    got = aug.pil_resize(torch.from_numpy(x)[None].cuda(), HW)
    assert got.shape == (1,) + HW + (3,) and got.dtype == torch.uint8
    assert np.array_equal(got[0].cpu().numpy(), ref)
    if kind == 'binary' and hw[0] < HW[0]:
        assert ref.min() == 0 and ref.max() == 255                        # the overshoot reached both clamps


@pytest.mark.parametrize('hw,HW', [((37, 53), (16, 12)), ((33, 50), (13, 17))], ids=['37x53-16x12', '33x50-13x17'])
def test_pil_resize_of_a_batch_of_three(aug, hw, HW):
    pairs = [want(hw, HW, ('uniform', 'binary', 'uniform')[n], seed=n) for n in range(3)]
    got = aug.pil_resize(torch.from_numpy(np.stack([p[0] for p in pairs])).cuda(), HW).cpu().numpy()
    for n in range(3):
        assert np.array_equal(got[n], pairs[n][1]), n


@pytest.mark.parametrize('hw,HW', [((37, 53), (16, 12)), ((40, 64), (20, 64)), ((40, 64), (40, 32)), ((24, 24), (24, 24))],
                         ids=['two-passes', 'vertical-only', 'horizontal-only', 'copy'])
def test_pil_resize_reads_a_crop_window_of_a_larger_tensor(aug, hw, HW):
    """rows of the source are 3 * 71 = 213 bytes apart (no multiple of 4) and start at an odd byte"""
    x, ref = want(hw, HW, 'uniform')
    big = torch.full((hw[0] + 9, 71, 3), 0x5A, dtype=torch.uint8)
    big[5:5 + hw[0], 3:3 + hw[1]] = torch.from_numpy(x)
    big = big.cuda()
    window = big[5:5 + hw[0], 3:3 + hw[1]][None]
    assert not window.is_contiguous()
    assert np.array_equal(aug.pil_resize(window, HW)[0].cpu().numpy(), ref)


def test_pil_resize_writes_one_slot_of_a_batch_and_nothing_else(aug):
    hw, HW = (33, 50), (13, 17)
    x, ref = want(hw, HW, 'binary')
    batch = torch.full((3,) + HW + (3,), 0xA5, dtype=torch.uint8, device='cuda')
    aug.pil_resize(torch.from_numpy(x)[None].cuda(), HW, out=batch[1])
    got = batch.cpu().numpy()
    assert np.array_equal(got[1], ref)
    assert (got[0] == 0xA5).all() and (got[2] == 0xA5).all()


def test_pil_resize_refuses_a_shrink_beyond_sixteen_before_any_launch(aug):
    with pytest.raises(ValueError, match='coefficients'):
        aug.pil_resize(torch.zeros((1, 8, 340, 3), dtype=torch.uint8, device='cuda'), (8, 19))


# ------------------------------------------------------------------------------------------------ mask overlay
def _overlay_case(HW, hw0, N=2, seed=0):
    rng = np.random.default_rng([77, HW[0], hw0[0], seed])
    pred = rng.integers(0, 25, (N,) + HW).astype(np.int32)                # 21 valid classes: 21..24 are above n_valid - 1
    pred[rng.uniform(size=pred.shape) < 0.05] = 253
    pred[:, 0, 0], pred[:, -1, -1] = 253, 24
    frames = rng.integers(0, 256, (N,) + hw0 + (3,), dtype=np.uint8)
    masks = np.stack([pil_rules.nearest_resize(p, hw0) for p in pred])
    overlays = np.stack([pil_rules.overlay(f, m, 21) for f, m in zip(frames, masks)])
    return pred, frames, masks.astype(np.uint8), overlays


def _run_overlay(pred, frames, HW, hw0, want_mask=True, want_overlay=True, n_valid=21, alpha=179):
    """the raw entry point with 64 sentinel bytes behind each output"""
    inf, L = load_pkg('inference'), load_pkg('_lib').lib()
    N = pred.shape[0]
    nm, no = N * hw0[0] * hw0[1], N * hw0[0] * hw0[1] * 3
    m = torch.full((nm + 64,), 0xC3, dtype=torch.uint8, device='cuda')
    o = torch.full((no + 64,), 0xC3, dtype=torch.uint8, device='cuda')
    p, f = torch.from_numpy(pred).cuda(), torch.from_numpy(frames).cuda()
    tab = torch.from_numpy(inf.overlay_tables(HW[0], HW[1], hw0[0], hw0[1])).cuda()
    cmap = torch.from_numpy(pil_rules.colormap()).cuda()
    L.mask_overlay_u8(p.data_ptr(), f.data_ptr() if want_overlay else None, m.data_ptr() if want_mask else None,
                      o.data_ptr() if want_overlay else None, tab.data_ptr(), cmap.data_ptr() if want_overlay else None, n_valid, alpha, N,
                      HW[0], HW[1], hw0[0], hw0[1], torch.cuda.current_stream().cuda_stream)
    m, o = m.cpu().numpy(), o.cpu().numpy()
    return m[:nm].reshape((N,) + hw0), m[nm:], o[:no].reshape((N,) + hw0 + (3,)), o[no:]


OVERLAY_CASES = [((16, 24), (37, 53)), ((65, 65), (48, 80))]               # bytes per lane (53 % 4 != 0), 32 bits per lane (80 % 4 == 0)


@pytest.mark.parametrize('HW,hw0', OVERLAY_CASES, ids=['16x24-37x53', '65x65-48x80'])
def test_mask_overlay_equals_the_restated_rules(ops, HW, hw0):
    pred, frames, masks, overlays = _overlay_case(HW, hw0)
    assert (masks == 253).any() and (masks == 24).any() and (masks < 21).any()
    m, m_tail, o, o_tail = _run_overlay(pred, frames, HW, hw0)
    assert np.array_equal(m, masks) and np.array_equal(o, overlays)
    assert (m_tail == 0xC3).all() and (o_tail == 0xC3).all()


@pytest.mark.parametrize('HW,hw0', OVERLAY_CASES, ids=['16x24-37x53', '65x65-48x80'])
def test_mask_overlay_with_either_output_missing(ops, HW, hw0):
    pred, frames, masks, overlays = _overlay_case(HW, hw0, seed=1)
    m, m_tail, o, o_tail = _run_overlay(pred, frames, HW, hw0, want_overlay=False)
    assert np.array_equal(m, masks) and (m_tail == 0xC3).all() and (o == 0xC3).all() and (o_tail == 0xC3).all()
    m, m_tail, o, o_tail = _run_overlay(pred, frames, HW, hw0, want_mask=False)
    assert np.array_equal(o, overlays) and (o_tail == 0xC3).all() and (m == 0xC3).all() and (m_tail == 0xC3).all()


def test_mask_resize_is_the_restated_nearest_rule(ops):
    inf = load_pkg('inference')
    mask = np.random.default_rng(5).integers(0, 254, (65, 65)).astype(np.uint8)
    for hw0 in ((48, 80), (130, 131), (65, 65)):
        got = inf.mask_resize(mask, hw0[::-1])
        assert got.dtype == np.uint8 and np.array_equal(got, pil_rules.nearest_resize(mask, hw0))


# ------------------------------------------------------------------------------------------------ DeepLab end to end
@pytest.fixture(scope='module')
def e2e(ops, tmp_path_factory):
    """the DeepLab of the CPU test on 2 frames of 48 x 80 noise, and the host chain around the same forward pass:
    restated Pillow resize -> model.predict_mask(uint8 batch) -> restated nearest resize -> restated blend"""
    from deeplab import DeepLab
    p = tmp_path_factory.mktemp('classes') / 'classes.txt'
    p.write_text('\n'.join('class%d' % i for i in range(21)) + '\n')
    d = DeepLab(model_type='mobilenetv2_lite', model_input_shape=(65, 65), output_stride=16, classes_path=str(p), weights_path=None)
    frames = np.random.default_rng(11).integers(0, 256, (2, 48, 80, 3), dtype=np.uint8)
    resized = np.stack([pil_rules.resize_bicubic(f, (65, 65)) for f in frames])
    small = d.deeplab_model.predict_mask(resized)
    masks = np.stack([pil_rules.nearest_resize(m, (48, 80)) for m in small]).astype(np.uint8)
    overlays = np.stack([pil_rules.overlay(f, m, 21) for f, m in zip(frames, masks)])
    return d, frames, resized, masks, overlays


def test_segment_batch_equals_the_host_chain(e2e):
    d, frames, _, masks, overlays = e2e
    m, o = d.segment_batch(frames)
    assert m.is_cuda and o.is_cuda and m.dtype == torch.uint8 and o.dtype == torch.uint8
    assert np.array_equal(m.cpu().numpy(), masks)
    assert np.array_equal(o.cpu().numpy(), overlays)
    assert len(np.unique(masks)) > 1                                       # (a random network still separates some pixels)


def test_a_cuda_tensor_and_a_numpy_array_give_the_same_bytes(e2e):
    d, frames = e2e[0], e2e[1]
    m0, o0 = d.segment_batch(frames)
    m1, o1 = d.segment_batch(torch.from_numpy(frames).cuda())
    assert torch.equal(m0, m1) and torch.equal(o0, o1)


def test_predict_and_segment_image_agree_with_segment_batch(e2e):
    Image = pytest.importorskip('PIL.Image')
    inf = load_pkg('inference')
    d, frames, resized = e2e[:3]
    m, o = d.segment_batch(frames[:1])                                     # the same frame, the same batch-1 forward
    masks, overlays = m.cpu().numpy(), o.cpu().numpy()
    image_data = inf.preprocess_image(Image.fromarray(frames[0]), (65, 65))
    assert image_data.shape == (1, 65, 65, 3) and image_data.dtype == np.float32
    assert np.array_equal(image_data[0], resized[0].astype(np.float32) / 127.5 - 1)
    assert np.array_equal(inf.preprocess_image(frames[0], (65, 65)), image_data)
    got = d.predict(image_data, (48, 80))
    assert got.dtype == np.uint8 and np.array_equal(got, masks[0])
    assert np.array_equal(d.predict(resized[:1], (48, 80)), masks[0])
    out = d.segment_image(Image.fromarray(frames[0]))
    assert out.size == (80, 48) and np.array_equal(np.asarray(out), overlays[0])


def test_predict_mask_takes_cuda_bytes_as_they_are(e2e):
    d, _, resized, _, _ = e2e
    assert np.array_equal(d.deeplab_model.predict_mask(torch.from_numpy(resized).cuda()), d.deeplab_model.predict_mask(resized))
