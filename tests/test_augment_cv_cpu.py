"""The OpenCV steps of the input pipeline without a device: known answers of the NumPy restatement (tests/cv_rules.py -- UNPINNED:
answers of the restated rules, not of OpenCV, which is not installed here), the host table builders of augment.py against the
restatement's tables, the order in which SegmentationGenerator.__getitem__ draws its random numbers, the refusals and the shim."""
import random
import types

import numpy as np
import pytest
import torch

import cv_rules as R
from conftest import load_pkg


# ------------------------------------------------------------------------------------------------------------ warp
def test_warp_identity_and_quarter_turns_on_an_odd_square():
    a = (np.arange(25).reshape(5, 5) + 1).astype(np.uint8)            # centre (2, 2)
    assert np.array_equal(R.warp_nn(a, 0, 1), a)
    assert np.array_equal(R.warp_nn(a, 90, 1), np.rot90(a, 1))
    assert np.array_equal(R.warp_nn(a, 180, 1), a[::-1, ::-1])


def test_warp_zoom_and_turn_on_an_even_rectangle():
    b = (np.arange(24).reshape(4, 6) + 1).astype(np.uint8)            # centre (3, 2)
    assert R.warp_nn(b, 0, 2).tolist() == [[9, 9, 10, 10, 11, 11], [15, 15, 16, 16, 17, 17], [15, 15, 16, 16, 17, 17],
                                           [21, 21, 22, 22, 23, 23]]
    assert R.warp_nn(b, 90, 1).tolist() == [[0, 6, 12, 18, 24, 0], [0, 5, 11, 17, 23, 0], [0, 4, 10, 16, 22, 0], [0, 3, 9, 15, 21, 0]]


def test_warp_moves_three_channels_like_one():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (9, 13, 3)).astype(np.uint8)
    out = R.warp_nn(img, 33.0, 0.9)
    for c in range(3):
        assert np.array_equal(out[..., c], R.warp_nn(np.ascontiguousarray(img[..., c]), 33.0, 0.9))


# ------------------------------------------------------------------------------------------------------------ CLAHE, YUV
@pytest.mark.parametrize('v, expect', [(0, 8), (3, 8), (128, 135), (255, 255)])
def test_clahe_of_a_constant_plane(v, expect):
    """64 x 64: tile 8 x 8, clip 1, one bin of 64 -> 63 clipped, batch 0, residual 63, step 4"""
    out = R.clahe_plane(np.full((64, 64), v, np.uint8))
    assert np.unique(out).tolist() == [expect]


def test_clahe_lut_entries_of_a_constant_tile():
    luts, (th, tw) = R.clahe_luts(np.full((64, 64), 128, np.uint8))
    assert (th, tw) == (8, 8)
    assert [int(luts[0, 0, i]) for i in (0, 1, 3, 4, 128, 248)] == [4, 4, 4, 8, 135, 255]
    assert all(np.array_equal(luts[0, 0], luts[ty, tx]) for ty in range(8) for tx in range(8))


def test_clahe_of_a_reflect_padded_constant_plane():
    plane = np.full((513, 513), 128, np.uint8)
    assert R.clahe_luts(plane)[1] == (65, 65)
    assert np.unique(R.clahe_plane(plane)).tolist() == [130]


def test_yuv_known_answers():
    px = lambda *c: np.array(c, np.uint8).reshape(1, 1, 3)
    assert R.bgr2yuv(px(255, 0, 0)).ravel().tolist() == [29, 239, 103]
    assert R.bgr2yuv(px(0, 255, 0)).ravel().tolist() == [150, 54, 0]
    assert R.bgr2yuv(px(10, 200, 90)).ravel().tolist() == [145, 62, 80]
    assert R.yuv2bgr(px(145, 62, 80)).ravel().tolist() == [11, 199, 90]
    for c in (0, 255):
        assert R.yuv2bgr(R.bgr2yuv(px(c, c, c))).ravel().tolist() == [c, c, c]


# ------------------------------------------------------------------------------------------------------------ resize
def test_resize_known_answers():
    s = np.array([[0, 100], [0, 100]], np.uint8)
    assert R.resize_linear(s, (4, 4)).tolist() == [[0, 25, 75, 100]] * 4
    rng = np.random.default_rng(0)
    q = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_linear(q, (64, 64)), q)
    i = q.astype(np.int64)
    area = ((i[0::2, 0::2] + i[0::2, 1::2] + i[1::2, 0::2] + i[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(R.resize_linear(q, (32, 32)), area)
    assert R.resize_nearest(np.arange(3, dtype=np.uint8).reshape(1, 3), (1, 7)).ravel().tolist() == [0, 0, 0, 1, 1, 2, 2]


def test_half_size_on_one_axis_is_the_linear_rule():
    """(64, 48) -> (32, 32): rows at scale 2 take the pair (2 y, 2 y + 1) with weights 1/2, 1/2; columns at scale 1.5 interpolate"""
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (64, 48)).astype(np.uint8)
    sx, x1, a0, a1 = R._linear_axis(32, 48, True)
    sy0, sy1, b0, b1 = R._linear_axis(32, 64, False)
    assert sy0.tolist() == list(range(0, 64, 2)) and sy1.tolist() == list(range(1, 64, 2)) and set(b0) == set(b1) == {1024}
    assert sx[:3].tolist() == [0, 1, 3] and a1[:3].tolist() == [512, 1536, 512]
    out = R.resize_linear(p, (32, 32))
    i = p.astype(np.int64)
    assert np.array_equal(R.resize_linear(p, (32, 24)), ((i[0::2, 0::2] + i[0::2, 1::2] + i[1::2, 0::2] + i[1::2, 1::2] + 2) >> 2))  # both halved
    T = i[:, sx] * a0 + i[:, x1] * a1
    assert np.array_equal(out, ((((b0[:, None] * (T[sy0] >> 4)) >> 16) + ((b1[:, None] * (T[sy1] >> 4)) >> 16) + 2) >> 2).astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------ host tables
def test_host_tables_equal_the_restatement_for_200_draws():
    A = load_pkg('augment')
    rng = np.random.default_rng(20)
    for _ in range(200):
        H, W, h, w = (int(v) for v in rng.integers(1, 600, 4))
        angle, scale = float(rng.normal(0, 60)), float(rng.normal(1, 0.4))
        assert np.array_equal(A.warp_tables(H, W, angle, scale), np.concatenate(R.warp_tables(H, W, angle, scale)))
        sx, x1, a0, a1 = R._linear_axis(W, w, True)
        sy0, sy1, b0, b1 = R._linear_axis(H, h, False)
        expect = np.concatenate([sx, x1, a0, a1, R._nearest_axis(W, w), sy0, sy1, b0, b1, R._nearest_axis(H, h)])
        t = A.resize_tables(h, w, H, W)
        assert t.dtype == np.int32 and np.array_equal(t, expect)
        assert 0 <= t[:2 * W].min() and t[:2 * W].max() < w and 0 <= t[4 * W:5 * W].min() and t[4 * W:5 * W].max() < w
        assert 0 <= t[5 * W:5 * W + 2 * H].min() and t[5 * W:5 * W + 2 * H].max() < h and t[5 * W + 4 * H:].max() < h


# ------------------------------------------------------------------------------------------------------------ draw order
class _Recorder:
    """stands in for the library: every entry point records its name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
        return fn


def _write_dataset(root, sizes):
    from PIL import Image
    (root / 'images').mkdir()
    (root / 'labels').mkdir()
    rng = np.random.default_rng(5)
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(root / 'images' / ('im%d.jpg' % k))
        lab = Image.fromarray(rng.integers(0, 21, (h, w)).astype(np.uint8), mode='P')
        lab.putpalette([v for c in range(256) for v in (c, 255 - c, (7 * c) % 256)])
        lab.save(root / 'labels' / ('im%d.png' % k))
    return ['im%d\n' % k for k in range(len(sizes))]


def _replay_draws(sizes, crop_shape):
    """the draws of deeplabv3p/data.py:72-106 through common/data_utils.py, in plain Python, for images of these sizes; -> the set of
    branches taken"""
    rand = lambda a=0, b=1: np.random.rand() * (b - a) + a
    seen = set()
    for h, w in sizes:
        rand()                                              # random_horizontal_flip
        rand()                                              # random_vertical_flip
        random.gauss(mu=0.0, sigma=30)                      # random_zoom_rotate: angle, scale, then the decision
        random.gauss(mu=1.0, sigma=0.2)
        if rand() < 0.3:
            seen.add('warp')
        if not np.random.rand() > 0.2:                      # Grid.__call__
            d = np.random.randint(w // 7, w // 3)
            np.random.randint(d)
            np.random.randint(d)
            np.random.randint(360)
            seen.add('grid')
        for _ in range(4):                                  # brightness, chroma, contrast, sharpness
            rand(.5, 1 / .5)
        rand()                                              # random_grayscale
        rand()                                              # random_blur
        if rand() < .1:                                     # random_crop
            if crop_shape[0] < h and crop_shape[1] < w:
                random.randrange(w - crop_shape[1])
                random.randrange(h - crop_shape[0])
                seen.add('crop')
            else:
                seen.add('crop_resize')
        if rand() < .2:                                     # random_histeq
            seen.add('histeq')
    return seen


def test_getitem_draws_in_the_reference_order(tmp_path, monkeypatch):
    A, D = load_pkg('augment'), load_pkg('data')
    sizes = [(40, 56), (72, 90), (64, 64), (100, 70)]
    ids = _write_dataset(tmp_path, sizes)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda: types.SimpleNamespace(cuda_stream=0))
    rec = _Recorder()
    monkeypatch.setattr(A, 'lib', lambda: rec)
    gen = D.SegmentationGenerator(str(tmp_path), ids, batch_size=4, input_shape=(64, 64))
    gen.device = 'cpu'
    seen = set()
    for seed in range(40):
        np.random.seed(seed)
        random.seed(seed)
        x, y = gen[0]
        after = np.random.get_state(), random.getstate()
        assert x.shape == (4, 64, 64, 3) and y.shape == (4, 64 * 64, 1) and x.dtype == y.dtype == torch.uint8
        np.random.seed(seed)
        random.seed(seed)
        seen |= _replay_draws(sizes, (64, 64))
        st = np.random.get_state()
        assert st[0] == after[0][0] and np.array_equal(st[1], after[0][1]) and st[2:] == after[0][2:], seed
        assert random.getstate() == after[1], seed
    assert seen == {'warp', 'grid', 'crop', 'crop_resize', 'histeq'}       # every branch that draws, or follows a draw, was walked
    assert {'aug_warp_nn_u8', 'aug_clahe_u8', 'aug_resize_u8', 'aug_gridmask_u8', 'aug_flip_crop_u8'} <= set(rec.calls)
    # without augmentation: nothing is drawn, one resize per image
    rec.calls.clear()
    gen.augment = False
    np.random.seed(7)
    before = np.random.get_state()
    gen[0]
    assert rec.calls == ['aug_resize_u8'] * 4 and np.array_equal(np.random.get_state()[1], before[1])


def test_the_two_gauss_draws_happen_whatever_prob_says(monkeypatch):
    A = load_pkg('augment')
    monkeypatch.setattr(A, 'lib', lambda: _Recorder())
    img, lab = torch.zeros((3, 8, 8, 3), dtype=torch.uint8), torch.zeros((3, 8, 8), dtype=torch.uint8)
    random.seed(3)
    np.random.seed(3)
    out = A.random_zoom_rotate(img, lab, prob=0.0)
    assert out[0] is img and out[1] is lab                               # nothing drawn: returned at once
    state = random.getstate()
    random.seed(3)
    for _ in range(3):
        random.gauss(0.0, 30)
        random.gauss(1.0, 0.2)
    assert random.getstate() == state
    np.random.seed(3)
    assert A.random_histeq(img, prob=0.0) is img


# ------------------------------------------------------------------------------------------------------------ refusals, contract
def test_value_errors(monkeypatch):
    A = load_pkg('augment')
    monkeypatch.setattr(A, 'lib', lambda: _Recorder())
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda: types.SimpleNamespace(cuda_stream=0))
    img = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='8 x 8'):
        A.random_histeq(img, size=4)
    for shape in ((1, 7, 16, 3), (1, 16, 7, 3)):
        with pytest.raises(ValueError, match='H, W >= 8'):
            A.clahe(torch.zeros(shape, dtype=torch.uint8), [1])
    with pytest.raises(ValueError, match='H, W >= 8'):
        R.clahe_luts(np.zeros((7, 16), np.uint8))
    A.clahe(img, [1])                                                      # 16 x 16 is fine
    with pytest.raises(ValueError, match='output'):
        load_pkg('data').SegmentationGenerator('.', [], output='tf')


def test_entry_points_check_their_arguments():
    """the argument checks of the three entry points answer before anything is launched"""
    L = load_pkg('_lib').lib()
    buf = torch.zeros(64 * 256, dtype=torch.uint8)
    p = buf.data_ptr()
    assert L.aug_warp_nn_u8.raw(p, p, None, None, p, p, 1, 8, 8, None) != 0          # output is the input
    assert L.aug_warp_nn_u8.raw(None, None, None, None, p, p, 1, 8, 8, None) != 0    # neither image nor label
    assert L.aug_clahe_u8.raw(p, p, p, p, 64 * 256, 1, 7, 8, None) != 0              # H < 8
    assert L.aug_clahe_u8.raw(p, p, p, p, 64 * 256 - 1, 1, 8, 8, None) != 0          # workspace too small
    assert L.aug_resize_u8.raw(p, 3 * 8 - 1, p + 1024, None, 0, None, p, 1, 8, 8, 4, 4, None) != 0   # pitch below one row
    assert L.aug_resize_u8.raw(p, 24, p, None, 0, None, p, 1, 8, 8, 4, 4, None) != 0               # output is the input
    with pytest.raises(load_pkg('_lib').Dl3pError, match='dl3p_aug_clahe_u8'):
        L.aug_clahe_u8(p, p, p, p, 64 * 256, 1, 8, 3, None)


def test_numpy_contract_and_balanced_weights():
    D = load_pkg('data')
    gen = D.SegmentationGenerator('.', [], num_classes=3, weighted_type='adaptive', output='numpy')
    img = np.array([0, 127, 128, 255, 1, 2], np.uint8).reshape(1, 1, 2, 3)
    lab = np.array([0, 0, 0, 2, 7, 255], np.uint8).reshape(1, 6, 1)
    x, y, w = gen.reference_contract(img, lab)
    assert x.dtype == y.dtype == np.float32 and np.array_equal(x, img.astype(np.float32) / 127.5 - 1)
    assert y.ravel().tolist() == [0, 0, 0, 2, 255, 255]                      # 7 > num_classes - 1 -> ignore_index
    # compute_class_weight('balanced'): n / (k count) with n = 6 pixels, k = 3 values present
    expect = np.array([6 / (3 * 3)] * 3 + [6 / (3 * 1)] + [6 / (3 * 2)] * 2, np.float64).astype(np.float32)
    assert list(w) == ['pred_mask'] and w['pred_mask'].dtype == np.float32 and np.array_equal(w['pred_mask'], expect[None])
    gen.weighted_type = None
    assert len(gen.reference_contract(img, lab)) == 2


def test_generator_bookkeeping_is_the_references(tmp_path):
    D = load_pkg('data')
    ids = ['a\n', ' b', 'c', 'd', 'e']
    gen = D.SegmentationGenerator(str(tmp_path), ids, batch_size=2, weighted_type='balanced')
    root = str(tmp_path.resolve())
    assert len(gen) == 2 and gen.get_weighted_type() == 'balanced'
    assert gen.get_batch_image_path(1) == [root + '/images/c.jpg', root + '/images/d.jpg']
    assert gen.get_batch_label_path(0) == [root + '/labels/a.png', root + '/labels/b.png']
    random.seed(1)
    gen.on_epoch_end()
    pairs = list(zip(gen.image_path_list, gen.label_path_list))
    assert sorted(p[0] for p in pairs) == sorted(root + '/images/%s.jpg' % k for k in 'abcde')
    assert all(i.replace('images', 'labels').replace('.jpg', '.png') == l for i, l in pairs)
    expect = [(root + '/images/%s.jpg' % k, root + '/labels/%s.png' % k) for k in 'abcde']
    random.seed(1)
    random.shuffle(expect)
    assert pairs == expect


def test_the_shim_resolves():
    from deeplabv3p.data import SegmentationGenerator
    assert SegmentationGenerator is load_pkg('data').SegmentationGenerator is load_pkg().SegmentationGenerator
