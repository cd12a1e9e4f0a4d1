"""The byte-level steps of the reference's deeplab.py restated in NumPy: PIL's Image.resize(size, Image.BICUBIC) on 8-bit RGB as
preprocess_image calls it, cv2.resize(mask, size, interpolation=INTER_NEAREST) as mask_resize calls it, the PASCAL colour map and the
overlay blend.  The oracle of tests/test_infer_io_gpu.py; nothing here is shared with the product code (it imports none of it).

PINNED: `resize_bicubic` restates Pillow's ImagingResample for 8 bits per channel and is held bit for bit to Pillow itself, live where
PIL imports and through tests/golden/pil_bicubic.npz everywhere (tests/test_infer_io_cpu.py).
`nearest_resize` is the INTER_NEAREST rule tests/cv_rules.py states (UNPINNED: OpenCV is not installed where this suite runs), and
`overlay` is this project's own integer blend: neither is checked against a library."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# ((h, w), (H, W)) of the small cases whose Pillow outputs tests/golden/pil_bicubic.npz holds (make_pil_bicubic.py), each on uniform
# noise and on 0 / 255 noise (the bicubic overshoot then reaches both clamps): an upscale whose taps are cut at both borders, a
# non-integer shrink, one pass only (each way), a copy, odd output sizes, and a shrink by 15.8 (65 coefficients, the kernel's cap)
CASES = (((7, 9), (16, 24)), ((37, 53), (16, 12)), ((40, 64), (20, 64)), ((40, 64), (40, 32)), ((24, 24), (24, 24)),
         ((33, 50), (13, 17)), ((8, 300), (8, 19)))
KINDS = ('uniform', 'binary')


def case_input(hw, kind, seed=0):
    """the seeded (h, w, 3) uint8 input of a case: 'uniform' noise, or 'binary' = every byte 0 or 255"""
    rng = np.random.default_rng([2026, hw[0], hw[1], KINDS.index(kind), seed])
    if kind == 'uniform':
        return rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    return (rng.integers(0, 2, (hw[0], hw[1], 3), dtype=np.uint8) * 255).astype(np.uint8)


def bicubic(x):
    """Keys' cubic with a = -0.5, in the order of operations of Pillow's C"""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_tables(in_size, out_size):
    """-> (xmin[out], cnt[out], k[out][ksize]) int32: the first source sample, the number of taps and the coefficients in 22-bit
    fixed point of every output sample along one axis; all float64 (Python floats), sample by sample"""
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmins = np.zeros(out_size, np.int32)
    cnts = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)              # int() truncates towards zero, like the C cast
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmins[xx], cnts[xx] = xmin, xmax
    return xmins, cnts, kk


def _pass(src, tables):
    """one pass along axis 0 of src (in, ...) uint8 -> (out, ...) uint8"""
    xmins, cnts, kk = tables
    out = np.empty((len(xmins),) + src.shape[1:], np.uint8)
    s = src.astype(np.int64)
    for xx in range(len(xmins)):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(int(cnts[xx])):
            acc += s[xmins[xx] + x] * int(kk[xx, x])
        assert np.all(np.abs(acc) < (1 << 31))          # Pillow accumulates in a C int
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic(img, shape):
    """Image.fromarray(img).resize(shape[::-1], Image.BICUBIC) for img (h, w, 3) uint8, shape = (H, W): the horizontal pass if the
    width changes, rounded to bytes, then the vertical pass if the height changes; neither -> a copy"""
    h, w = img.shape[:2]
    H, W = shape
    out = img
    if w != W:
        out = np.swapaxes(_pass(np.swapaxes(out, 0, 1), axis_tables(w, W)), 0, 1)
    if h != H:
        out = _pass(out, axis_tables(h, H))
    return np.ascontiguousarray(out).copy()


def nearest_index(dst, src):
    """cv2.INTER_NEAREST: source index of every destination index, min(floor(d * (1 / (dst / src))), src - 1) in float64"""
    scale = 1.0 / (float(dst) / src)
    return np.array([min(int(math.floor(d * scale)), src - 1) for d in range(dst)], np.int64)


def nearest_resize(mask, shape):
    """cv2.resize(mask, shape[::-1], interpolation=cv2.INTER_NEAREST) for mask (H, W), shape = (h0, w0)"""
    ny, nx = nearest_index(shape[0], mask.shape[0]), nearest_index(shape[1], mask.shape[1])
    return mask[ny][:, nx]


def colormap():
    """the PASCAL VOC colour map: bit j of channel c of entry i, counted from the top, is bit 3 j + c of i"""
    cm = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for c in range(3):
            v = 0
            for j in range(8):
                v |= ((i >> (3 * j + c)) & 1) << (7 - j)
            cm[i, c] = v
    return cm


def overlay(img, mask, n_valid, alpha=0.7):
    """img (h0, w0, 3) uint8, mask (h0, w0) integer class ids at the frame's size -> the composite (h0, w0, 3) uint8:
    ids above n_valid - 1 show as the class n_valid; (img (256 - A) + colour A + 128) >> 8 with A = rint(alpha * 256)"""
    A = int(np.rint(alpha * 256))
    d = mask.astype(np.int64)
    if n_valid > 0:
        d = np.where(d > n_valid - 1, n_valid, d)
    col = colormap()[d].astype(np.int64)
    return ((img.astype(np.int64) * (256 - A) + col * A + 128) >> 8).astype(np.uint8)
