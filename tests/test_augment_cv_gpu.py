"""The OpenCV steps of the input pipeline on the device (csrc/augment_cv.hip) and SegmentationGenerator, bit for bit against the NumPy
restatement tests/cv_rules.py (UNPINNED: a restatement of OpenCV's published rules, not OpenCV) and, for the generator's other steps,
oracle/np_augment.py.  No tolerance anywhere: every comparison is array equality.  The kernels write into buffers with 0xA5 guard bytes
on both sides, which must survive."""
import functools
import random

import numpy as np
import pytest
import torch

import cv_rules as R
from conftest import load_pkg
from oracle import np_augment as NP

pytestmark = pytest.mark.gpu

GUARD = 4096


class Guarded:
    """`nbytes` of device memory between two guard regions of 0xA5 (the payload starts as 0xA5 too)"""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
        self.t = self.buf[GUARD:GUARD + nbytes]

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.n:] == 0xA5).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ warp
WARP_DRAWS = [None, (30, 0.8), (-75, 1.3), (0, 1), (180, 1), (12.5, 0.05)]        # the last: large negative coordinates (arithmetic shift)


@pytest.mark.parametrize('shape', [(3, 37, 53), (1, 8, 8), (2, 64, 1024), (2, 513, 513)])
def test_warp_matches_the_restatement(shape):
    A, L = load_pkg('augment'), load_pkg('_lib').lib()
    N, H, W = shape
    rng = np.random.default_rng(H * W)
    for first in range(0, len(WARP_DRAWS), N):                                   # every draw on every shape, N images per launch
        draws = [WARP_DRAWS[(first + n) % len(WARP_DRAWS)] for n in range(N)]
        img = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
        lab = rng.integers(0, 22, (N, H, W)).astype(np.uint8)
        lab[rng.uniform(size=lab.shape) < 0.1] = 255
        want = [(img[n], lab[n]) if dr is None else (R.warp_nn(img[n], *dr), R.warp_nn(lab[n], *dr)) for n, dr in enumerate(draws)]
        d_img, d_lab = _dev(img), _dev(lab)
        out, lout = Guarded(img.size), Guarded(lab.size)
        tab = np.zeros((N, 2 * W + 2 * H), np.int32)
        for n, dr in enumerate(draws):
            if dr is not None:
                tab[n] = A.warp_tables(H, W, *dr)
        fl = _dev(np.array([0 if dr is None else 1 for dr in draws], np.int32))
        d_tab = _dev(tab)
        L.aug_warp_nn_u8(d_img.data_ptr(), out.t.data_ptr(), d_lab.data_ptr(), lout.t.data_ptr(), fl.data_ptr(), d_tab.data_ptr(), N, H, W,
                         _stream())
        got, lgot = out.t.view(N, H, W, 3).cpu().numpy(), lout.t.view(N, H, W).cpu().numpy()
        assert out.intact() and lout.intact()
        for n in range(N):
            assert np.array_equal(got[n], want[n][0]), (shape, draws[n])
            assert np.array_equal(lgot[n], want[n][1]), (shape, draws[n])
        assert np.array_equal(d_img.cpu().numpy(), img) and np.array_equal(d_lab.cpu().numpy(), lab)       # a gather: inputs untouched
        wi, wl = A.warp_affine_nn(d_img, d_lab, draws)                           # the public call gives the same bytes
        assert np.array_equal(wi.cpu().numpy(), got) and np.array_equal(wl.cpu().numpy(), lgot)


# ------------------------------------------------------------------------------------------------------------ CLAHE
def _content(kind, N, H, W, rng):
    if kind == 'noise':
        return rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    if kind == 'band':                                   # low contrast: heavy clipping, the residual path
        return rng.integers(100, 111, (N, H, W, 3)).astype(np.uint8)
    if kind == 'constant':
        return np.broadcast_to(rng.integers(0, 256, (N, 1, 1, 3)), (N, H, W, 3)).astype(np.uint8)
    ramp = (np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(ramp[None, None, :, None], (N, H, W, 3)))


@pytest.mark.parametrize('kind', ['noise', 'band', 'constant', 'ramp'])
@pytest.mark.parametrize('shape', [(2, 64, 64), (1, 37, 53), (1, 8, 8), (2, 9, 16), (1, 513, 513)])
def test_clahe_matches_the_restatement(shape, kind):
    A, L = load_pkg('augment'), load_pkg('_lib').lib()
    N, H, W = shape
    img = _content(kind, N, H, W, np.random.default_rng(H + W))
    histeq = [R.histeq(img[n]) for n in range(N)]
    d_img = _dev(img)
    for flags in ([[1, 0], [0, 1]] if N == 2 else [[1], [0]]):                   # mixed: an unflagged image comes out untouched
        out, luts = Guarded(img.size), Guarded(N * 64 * 256)
        fl = _dev(np.array(flags, np.int32))
        L.aug_clahe_u8(d_img.data_ptr(), out.t.data_ptr(), fl.data_ptr(), luts.t.data_ptr(), luts.n, N, H, W, _stream())
        got = out.t.view(N, H, W, 3).cpu().numpy()
        assert out.intact() and luts.intact()
        for n in range(N):
            assert np.array_equal(got[n], histeq[n] if flags[n] else img[n]), (shape, kind, flags, n)
            if flags[n]:
                want_luts = R.clahe_luts(R.bgr2yuv(img[n])[..., 0])[0].reshape(64, 256)
                assert np.array_equal(luts.t.view(N, 64, 256)[n].cpu().numpy(), want_luts), (shape, kind, 'luts')
        assert np.array_equal(d_img.cpu().numpy(), img)
    pub = A.clahe(d_img, [1] * N)                                                # the public call; then in place
    assert all(np.array_equal(pub[n].cpu().numpy(), histeq[n]) for n in range(N))
    assert A.clahe(d_img, [1] * N, out=d_img) is d_img
    assert all(np.array_equal(d_img[n].cpu().numpy(), histeq[n]) for n in range(N))


# ------------------------------------------------------------------------------------------------------------ resize
RESIZES = [((5, 7), (8, 8)), ((1, 1), (4, 4)), ((37, 53), (16, 16)), ((64, 64), (32, 32)), ((64, 48), (32, 32)), ((24, 40), (24, 40)),
           ((375, 500), (512, 512))]


@pytest.mark.parametrize('src, dst', RESIZES, ids=['%dx%d-%dx%d' % (s + d) for s, d in RESIZES])
def test_resize_writes_slot_one_of_three(src, dst):
    A = load_pkg('augment')
    (h, w), (H, W) = src, dst
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    lab = rng.integers(0, 256, (h, w)).astype(np.uint8)
    batch, lbatch = Guarded(3 * H * W * 3), Guarded(3 * H * W)
    bi, bl = batch.t.view(3, H, W, 3), lbatch.t.view(3, H * W, 1)
    oi, ol = A.resize(_dev(img)[None], _dev(lab)[None], (H, W), out=(bi[1], bl[1]))
    assert oi.data_ptr() == bi[1].data_ptr() and ol.data_ptr() == bl[1].data_ptr()
    got, lgot = bi.cpu().numpy(), bl.cpu().numpy().reshape(3, H, W)
    assert batch.intact() and lbatch.intact()
    assert (got[0] == 0xA5).all() and (got[2] == 0xA5).all() and (lgot[0] == 0xA5).all() and (lgot[2] == 0xA5).all()
    assert np.array_equal(got[1], R.resize_linear(img, (H, W))), (src, dst)
    assert np.array_equal(lgot[1], R.resize_nearest(lab, (H, W))), (src, dst)


def test_resize_of_a_batch_and_of_a_pitched_window():
    A = load_pkg('augment')
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (2, 40, 60, 3)).astype(np.uint8)
    lab = rng.integers(0, 256, (2, 40, 60)).astype(np.uint8)
    oi, ol = A.resize(_dev(img), _dev(lab), (33, 47))
    for n in range(2):
        assert np.array_equal(oi[n].cpu().numpy(), R.resize_linear(img[n], (33, 47)))
        assert np.array_equal(ol[n].cpu().numpy(), R.resize_nearest(lab[n], (33, 47)))
    win_i, win_l = _dev(img)[:1, 3:36, 10:50], _dev(lab)[:1, 3:36, 10:50]            # rows 180 / 60 bytes apart, 120 / 40 used
    oi, ol = A.resize(win_i, win_l, (16, 20))
    assert np.array_equal(oi[0].cpu().numpy(), R.resize_linear(np.ascontiguousarray(img[0, 3:36, 10:50]), (16, 20)))
    assert np.array_equal(ol[0].cpu().numpy(), R.resize_nearest(np.ascontiguousarray(lab[0, 3:36, 10:50]), (16, 20)))


# ------------------------------------------------------------------------------------------------------------ generator
SIZES = [(80, 100), (48, 72), (64, 64), (90, 70)]
SHAPE = (64, 64)
SEEDS = range(6)


@functools.lru_cache(maxsize=None)
def _dataset(root):
    from pathlib import Path
    from PIL import Image
    root = Path(root)
    (root / 'images').mkdir(parents=True)
    (root / 'labels').mkdir()
    rng = np.random.default_rng(5)
    for k, (h, w) in enumerate(SIZES):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(yy * 255 // h), (xx * 255 // w), ((yy + xx) * 255 // (h + w))], -1)
        noisy = np.clip(smooth + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(root / 'images' / ('im%d.jpg' % k), quality=90)
        lab = rng.integers(0, 21, (h // 8 + 1, w // 8 + 1)).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        lab[rng.uniform(size=lab.shape) < 0.05] = 255                           # the void label of a VOC palette PNG
        lab[rng.uniform(size=lab.shape) < 0.02] = 30                            # above num_classes - 1
        p = Image.fromarray(np.ascontiguousarray(lab), mode='P')
        p.putpalette([v for c in range(256) for v in (c, 255 - c, (7 * c) % 256)])
        p.save(root / 'labels' / ('im%d.png' % k))
    return ['im%d\n' % k for k in range(len(SIZES))]


def _host_replay(image, label, shape, seen):
    """deeplabv3p/data.py:72-111 for one decoded image: the reference's draws in the reference's order, each step by its restatement"""
    rand = lambda a=0, b=1: np.random.rand() * (b - a) + a
    image, label = NP.flip_crop(image, label, 1 if rand() < .5 else 0)
    image, label = NP.flip_crop(image, label, 2 if rand() < .5 else 0)
    angle, scale = random.gauss(mu=0.0, sigma=30), random.gauss(mu=1.0, sigma=0.2)
    if rand() < 0.3:
        image, label = R.warp_nn(image, angle, scale), R.warp_nn(label, angle, scale)
        seen.add('warp')
    h, w = label.shape
    if not np.random.rand() > 0.2:
        d = np.random.randint(w // 7, w // 3)
        st_h, st_w, r = np.random.randint(d), np.random.randint(d), np.random.randint(360)
        keep = NP.gridmask_keep(h, w, int(d), int(st_h), int(st_w), int(r))
        image, label = image * keep[..., None], label * keep
        seen.add('grid')
    for op in (NP.BRIGHTNESS, NP.COLOR, NP.CONTRAST, NP.SHARPNESS):
        image = NP.enhance(image, op, float(np.float32(rand(.5, 1 / .5))))
    image = NP.gray_blur(image, 1 if rand() < .2 else 0)
    image = NP.gray_blur(image, 2 if rand() < .5 else 0)
    if rand() < .1:
        if shape[0] < h and shape[1] < w:
            x = random.randrange(w - shape[1])
            y = random.randrange(h - shape[0])
            image, label = NP.flip_crop(image, label, 0, (y, x), shape)
            seen.add('crop')
        else:
            image, label = R.resize_linear(image, shape), R.resize_nearest(label, shape)
            seen.add('crop_resize')
    if rand() < .2:
        image = R.histeq(image)
        seen.add('histeq')
    return R.resize_linear(image, shape), R.resize_nearest(label, shape)


def test_generator_batches_equal_a_host_replay(tmp_path):
    D = load_pkg('data')
    ids = _dataset(str(tmp_path / 'set'))
    gen = D.SegmentationGenerator(str(tmp_path / 'set'), ids, batch_size=2, num_classes=21, input_shape=SHAPE)
    ref = D.SegmentationGenerator(str(tmp_path / 'set'), ids, batch_size=2, num_classes=21, input_shape=SHAPE, weighted_type='adaptive',
                                  output='numpy')
    assert len(gen) == 2
    decoded = [gen.decode(i, l) for i, l in zip(gen.image_path_list, gen.label_path_list)]
    assert [d[1].shape for d in decoded] == SIZES and all(d[1].dtype == np.uint8 and d[1].max() == 255 for d in decoded)
    seen = set()
    for seed in SEEDS:
        for i in range(2):
            np.random.seed(seed)                                    # seeded after construction (the constructor seeds by the clock)
            random.seed(seed)
            x, y = gen[i]
            after = np.random.get_state()[1].copy(), random.getstate()
            assert x.is_cuda and y.is_cuda and x.dtype == y.dtype == torch.uint8 and x.shape == (2, 64, 64, 3) and y.shape == (2, 4096, 1)
            got, lgot = x.cpu().numpy(), y.cpu().numpy()
            np.random.seed(seed)
            random.seed(seed)
            want = [_host_replay(*decoded[2 * i + n], SHAPE, seen) for n in range(2)]
            assert np.array_equal(np.random.get_state()[1], after[0]) and random.getstate() == after[1]
            for n in range(2):
                assert np.array_equal(got[n], want[n][0]), (seed, i, n)
                assert np.array_equal(lgot[n].reshape(64, 64), want[n][1]), (seed, i, n)
            # output='numpy': the reference's contract, computed here from that batch
            np.random.seed(seed)
            random.seed(seed)
            xf, yf, sw = ref[i]
            lab = lgot.astype('int32').reshape(2, -1)
            lab[lab > 20] = 255
            assert xf.dtype == np.float32 and np.array_equal(xf, got.astype(np.float32) / 127.5 - 1)
            assert yf.dtype == np.float32 and yf.shape == (2, 4096, 1) and np.array_equal(yf[..., 0], lab.astype(np.float32))
            w = np.zeros((2, 4096), np.float32)
            for n in range(2):
                classes, counts = np.unique(lab[n], return_counts=True)
                for c, k in zip(classes, counts):
                    np.putmask(w[n], lab[n] == c, 4096 / (len(classes) * np.float64(k)))
            assert list(sw) == ['pred_mask'] and np.array_equal(sw['pred_mask'], w)
    assert seen == {'warp', 'grid', 'crop', 'crop_resize', 'histeq'}, seen      # (SEEDS walk every branch of the chain)
    # two alternating batches: the one handed out last is not the one written next
    a = gen[0][0]
    b = gen[1][0]
    assert a.data_ptr() != b.data_ptr() and gen[0][0].data_ptr() == a.data_ptr()
    # no augmentation: decode, upload, resize
    gen.augment = False
    x, y = gen[1]
    for n in range(2):
        assert np.array_equal(x[n].cpu().numpy(), R.resize_linear(decoded[2 + n][0], SHAPE))
        assert np.array_equal(y[n].cpu().numpy().reshape(64, 64), R.resize_nearest(decoded[2 + n][1], SHAPE))


# ------------------------------------------------------------------------------------------------------------ the model side
def _model(pkg, **kw):
    torch.manual_seed(0)
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', 21, SHAPE, 16, training=True)
    m.compile(optimizer=pkg.SGD(0.01, momentum=0.9), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255), **kw)
    return m


def test_model_runs_from_the_device_generator(tmp_path):
    pkg, D = load_pkg(), load_pkg('data')
    ids = _dataset(str(tmp_path / 'set'))
    gen = D.SegmentationGenerator(str(tmp_path / 'set'), ids, batch_size=2, num_classes=21, input_shape=SHAPE)
    np.random.seed(11)
    random.seed(11)
    x, y = gen[0]
    # one step on the CUDA tensors and one on their host copies: the same loss, bit for bit, from models of the same seed
    on_dev = _model(pkg).train_on_batch(x, y)
    on_host = _model(pkg).train_on_batch(x.cpu().numpy(), y.cpu().numpy())
    assert np.isfinite(on_dev) and on_dev == on_host, (on_dev, on_host)
    # fit from the device generator = train_on_batch on downloads of the same batches
    m, ref = _model(pkg), _model(pkg)
    np.random.seed(12)
    random.seed(12)
    want = []
    for i in range(2):
        bx, by = gen[i]
        want.append(ref.train_on_batch(bx.cpu().numpy(), by.cpu().numpy()))
    np.random.seed(12)
    random.seed(12)
    gen.on_epoch_end = lambda: None                                 # (keep the order for the evaluation below)
    hist = m.fit(gen, steps_per_epoch=2, epochs=1, verbose=0)
    assert hist['loss'][0] == float(np.mean(want)), (hist['loss'][0], want)
    w, w_ref = m.get_weights_by_name(), ref.get_weights_by_name()
    assert all(np.array_equal(w[k], w_ref[k]) for k in w_ref)
    # adaptive weights: the third item is the string, the weights are made on the device
    agen = D.SegmentationGenerator(str(tmp_path / 'set'), ids, batch_size=2, num_classes=21, input_shape=SHAPE, weighted_type='adaptive',
                                   augment=False)
    assert agen[0][2] == 'adaptive'
    ma, ra = _model(pkg, sample_weight_mode='temporal'), _model(pkg, sample_weight_mode='temporal')
    bx, by, _ = agen[0]
    ha = ma.fit(agen, steps_per_epoch=1, epochs=1, verbose=0)
    assert ha['loss'][0] == ra.train_on_batch(bx.cpu().numpy(), by.cpu().numpy(), sample_weight='adaptive')
    # evaluation and prediction from CUDA uint8 tensors equal those from their host copies
    egen = D.SegmentationGenerator(str(tmp_path / 'set'), ids, batch_size=2, num_classes=21, input_shape=SHAPE, augment=False)
    host = [(bx.cpu().numpy(), by.cpu().numpy()) for bx, by in (egen[0], egen[1])]
    r_dev, r_host = m.evaluate_miou(egen), m.evaluate_miou(host)
    assert np.array_equal(r_dev['confusion_matrix'], r_host['confusion_matrix']) and r_dev['mIoU'] == r_host['mIoU']
    assert r_dev['confusion_matrix'].sum() > 0
    assert m.evaluate(egen) == m.evaluate(host)
    bx = egen[0][0]
    assert np.array_equal(m.predict(bx), m.predict(bx.cpu().numpy()))
