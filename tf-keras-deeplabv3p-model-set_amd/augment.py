"""Device-side counterparts of the byte-level augmentations in the reference's generator (deeplabv3p/data.py:72-104,
common/data_utils.py).  Same names and argument meaning as the reference functions, applied to a BATCH that already
sits on the GPU as bytes: images (N,H,W,3) uint8, labels (N,H,W) uint8 torch tensors.  The random draws are made on the
host exactly as the reference makes them (`rand() < prob` per image, `rand(jitter, 1/jitter)` per image); the kernels
(csrc/augment.hip) reproduce PIL / NumPy bit for bit for a given draw.

random_gridmask is here too: its rotation is PIL's (Image.rotate, NEAREST), restated from Pillow's 16.16 fixed-point affine
map and pinned against PIL itself.

random_grayscale and random_blur are here as UNPINNED restatements of OpenCV's published 8-bit arithmetic (cv2 is not in this image:
the kernels are held to oracle/np_augment.py's restatement of the same formulas, not to OpenCV itself).

random_zoom_rotate (cv2.warpAffine, INTER_NEAREST), random_histeq (BGR2YUV, CLAHE on Y, YUV2BGR) and the generator's final cv2.resize
(`resize`: INTER_LINEAR image, INTER_NEAREST label) are here under the same UNPINNED label (csrc/augment_cv.hip): the rules are written
out in DESIGN.md section 7 and restated in NumPy by tests/cv_rules.py, which is what the kernels are held to bit for bit.  Their float64
parts (the inverted rotation matrix, the resize scales) are evaluated here, on the host, into small integer tables that are uploaded
with the call (warp_tables, resize_tables).

pil_resize is the inference front end's resize (common/data_utils.py:436-454, preprocess_image): PIL's Image.resize(size, BICUBIC),
Pillow's antialiased 8-bit resampler restated in integers and PINNED against Pillow (tests/pil_rules.py, tests/golden/pil_bicubic.npz);
its float64 filter weights become 22-bit fixed-point tables on the host (pil_resize_tables).

Not here: the decode (PIL, on the host: data.py) and warpAffine / resize with any other interpolation than the reference's.
"""
import functools

import numpy as np
import torch

from ._lib import lib

BRIGHTNESS, COLOR, CONTRAST, SHARPNESS = 0, 1, 2, 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rand(a=0, b=1):
    return np.random.rand() * (b - a) + a


def enhance(images, op, factors, out=None):
    """PIL ImageEnhance.{Brightness, Color, Contrast, Sharpness}(img).enhance(factors[n]) for every image of the batch"""
    N, H, W, C = images.shape
    assert images.dtype == torch.uint8 and C == 3 and images.is_contiguous()
    f = torch.as_tensor(np.asarray(factors, np.float32).reshape(N)).to(images.device)
    out = torch.empty_like(images) if out is None else out
    sums = torch.zeros(N, dtype=torch.int64, device=images.device) if op == CONTRAST else None
    lib().aug_enhance_u8(images.data_ptr(), out.data_ptr(), f.data_ptr(), op, sums.data_ptr() if sums is not None else None,
                         N, H, W, _stream())
    return out


def flip_crop(images, labels, flags=None, yx=None, hw=None):
    """flags[n] bit 0 / 1 = horizontal / vertical flip; yx[n] = top-left of an hw = (h, w) window of the flipped image"""
    N, H, W, _ = images.shape
    assert images.dtype == torch.uint8 and labels.dtype == torch.uint8 and labels.shape == (N, H, W)
    h, w = (H, W) if hw is None else hw
    dev = images.device
    fl = None if flags is None else torch.as_tensor(np.asarray(flags, np.int32).reshape(N)).to(dev)
    off = None if yx is None else torch.as_tensor(np.asarray(yx, np.int32).reshape(N, 2)).to(dev)
    out = torch.empty((N, h, w, 3), dtype=torch.uint8, device=dev)
    lout = torch.empty((N, h, w), dtype=torch.uint8, device=dev)
    lib().aug_flip_crop_u8(images.data_ptr(), out.data_ptr(), labels.data_ptr(), lout.data_ptr(),
                           fl.data_ptr() if fl is not None else None, off.data_ptr() if off is not None else None, N, H, W, h, w,
                           _stream())
    return out, lout


# ---- the reference's function names (common/data_utils.py), batched
def random_horizontal_flip(images, labels, prob=.5):
    return flip_crop(images, labels, [1 if rand() < prob else 0 for _ in range(images.shape[0])])


def random_vertical_flip(images, labels, prob=.5):
    return flip_crop(images, labels, [2 if rand() < prob else 0 for _ in range(images.shape[0])])


def random_brightness(images, jitter=.5):
    return enhance(images, BRIGHTNESS, [rand(jitter, 1 / jitter) for _ in range(images.shape[0])])


def random_chroma(images, jitter=.5):
    return enhance(images, COLOR, [rand(jitter, 1 / jitter) for _ in range(images.shape[0])])


def random_contrast(images, jitter=.5):
    return enhance(images, CONTRAST, [rand(jitter, 1 / jitter) for _ in range(images.shape[0])])


def random_sharpness(images, jitter=.5):
    return enhance(images, SHARPNESS, [rand(jitter, 1 / jitter) for _ in range(images.shape[0])])


def gray_blur(images, flags, out=None):
    """flags[n] bit 0: cv2.cvtColor(BGR2GRAY) + GRAY2BGR; bit 1: cv2.GaussianBlur(image, (5, 5), 0) (grayscale first, as the generator
    applies them)"""
    N, H, W, C = images.shape
    assert images.dtype == torch.uint8 and C == 3 and images.is_contiguous()
    fl = torch.as_tensor(np.asarray(flags, np.int32).reshape(N)).to(images.device)
    out = torch.empty_like(images) if out is None else out
    lib().aug_gray_blur_u8(images.data_ptr(), out.data_ptr(), fl.data_ptr(), N, H, W, _stream())
    return out


def random_grayscale(images, prob=.2):
    return gray_blur(images, [1 if rand() < prob else 0 for _ in range(images.shape[0])])


def random_blur(images, prob=.5, size=5):
    if size != 5:
        raise ValueError('the device kernel restates the 5 x 5 table of cv2.GaussianBlur (the generator\'s default size)')
    return gray_blur(images, [2 if rand() < prob else 0 for _ in range(images.shape[0])])


def gridmask_params(h, w, d, st_h, st_w, r, ratio=0.5):
    """the 16 integers dl3p_aug_gridmask_u8 takes for one image, from the reference's draws (Grid.__call__,
    common/data_utils.py:288-339): hh = ceil(sqrt(h^2 + w^2)), band width l = ceil(d ratio), and Pillow's rotate as it
    computes it -- transpose fast paths at 0 / 90 / 180 / 270 degrees, otherwise the affine matrix of -r (entries rounded to 15
    decimals, centre (hh/2, hh/2) fixed) in 16.16 fixed point, FIX(v) = floor(65536 v + 0.5), half-pixel offset folded in"""
    import math
    hh = math.ceil(math.sqrt(h * h + w * w))
    l = math.ceil(d * ratio)
    r = r % 360
    kind = {0: 0, 90: 1, 180: 2, 270: 3}.get(r, 4)
    a0 = a1 = a2 = a3 = a4 = a5 = 0
    if kind == 4:
        ang = -math.radians(r)
        a = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
        c = hh / 2.0
        a[2] = a[0] * -c + a[1] * -c + a[2] + c
        a[5] = a[3] * -c + a[4] * -c + a[5] + c
        fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
        a0, a1, a3, a4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
        a2 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5)
        a5 = fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
    return [1, hh, d, l, st_h, st_w, kind, a0, a1, a2, a3, a4, a5, (hh - h) // 2, (hh - w) // 2, 0]


def gridmask(images, labels, draws):
    """apply GridMask IN PLACE; draws[n] = None (image left alone) or (d, st_h, st_w, r)"""
    N, H, W, _ = images.shape
    assert images.dtype == torch.uint8 and labels.dtype == torch.uint8 and labels.shape == (N, H, W)
    assert images.is_contiguous() and labels.is_contiguous()
    rows = [[0] * 16 if dr is None else gridmask_params(H, W, *dr) for dr in draws]
    prm = torch.as_tensor(np.asarray(rows, np.int32)).to(images.device)
    lib().aug_gridmask_u8(images.data_ptr(), labels.data_ptr(), prm.data_ptr(), N, H, W, _stream())
    return images, labels


def random_gridmask(images, labels, prob=0.2):
    """random_gridmask (common/data_utils.py:342-361) for a batch, in place.  Per image, in the reference's order:
    np.random.rand() > prob -> untouched; d = randint(W // 7, W // 3); st_h = randint(d); st_w = randint(d); r = randint(360)"""
    N, H, W, _ = images.shape
    draws = []
    for _ in range(N):
        if np.random.rand() > prob:
            draws.append(None)
            continue
        d = np.random.randint(W // 7, W // 3)
        st_h = np.random.randint(d)
        st_w = np.random.randint(d)
        draws.append((int(d), int(st_h), int(st_w), int(np.random.randint(360))))
    return gridmask(images, labels, draws)


def random_crop(images, labels, crop_shape, prob=.1, resize_small=False):
    """the crop branch of the reference's random_crop (common/data_utils.py:364-400) for a batch.  DEVIATION, by
    construction: the reference decides `rand() < prob` per image; a batch tensor needs one output shape, so the decision is
    drawn ONCE for the batch.  Within a cropping batch the window of every image is drawn as the reference draws it -- x
    (`randrange(W - crop_w)`) first, then y (data_utils.py:390-391) -- so a seeded `random` yields the reference's windows.
    Returns the inputs unchanged when the draw says no or the window is not smaller than the image (the reference then
    resizes with cv2: `resize`, which resize_small=True applies here, as the generator asks for; called per image, N = 1, this is
    the reference's function, per-image decision included)."""
    import random
    N, H, W, _ = images.shape
    if not (rand() < prob):
        return images, labels
    if not (crop_shape[0] < H and crop_shape[1] < W):
        return resize(images, labels, crop_shape) if resize_small else (images, labels)
    yx = []
    for _ in range(N):
        x = random.randrange(W - crop_shape[1])
        y = random.randrange(H - crop_shape[0])
        yx.append((y, x))
    return flip_crop(images, labels, None, yx, tuple(crop_shape))


# ---- the OpenCV steps (csrc/augment_cv.hip).  UNPINNED restatements: see the module docstring
def _round_i32(v):
    """cvRound with saturation: round half to even, to int32"""
    return np.clip(np.rint(v), -2147483648.0, 2147483647.0).astype(np.int64)


def warp_tables(H, W, angle, scale):
    """the 2 W + 2 H integers dl3p_aug_warp_nn_u8 takes for one image, {adelta[W], bdelta[W], X0[H], Y0[H]}: cv2.getRotationMatrix2D
    about (W // 2, H // 2) in float64, inverted as warpAffine inverts it (its order of operations), then the 22.10 fixed-point column
    and row terms of the inverse map (the rounding half, 512, goes into the row terms)"""
    import math
    a = angle * math.pi / 180.0
    al, be = scale * math.cos(a), scale * math.sin(a)
    cx, cy = float(W // 2), float(H // 2)
    m0, m1, m2, m3, m4, m5 = al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy
    D = m0 * m4 - m1 * m3
    D = 1.0 / D if D != 0 else 0.0
    m0, m4 = m4 * D, m0 * D
    m1 *= -D
    m3 *= -D
    m2, m5 = -m0 * m2 - m1 * m5, -m3 * m2 - m4 * m5
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    t = np.concatenate([_round_i32(m0 * x * 1024), _round_i32(m3 * x * 1024), _round_i32((m1 * y + m2) * 1024) + 512,
                        _round_i32((m4 * y + m5) * 1024) + 512])
    return t.astype(np.int32)


def warp_affine_nn(images, labels, draws):
    """cv2.warpAffine(flags=INTER_NEAREST, borderMode=BORDER_CONSTANT, borderValue=0) of image and label by the matrix of
    cv2.getRotationMatrix2D((W // 2, H // 2), angle, scale); draws[n] = None (image copied through) or (angle, scale)"""
    N, H, W, _ = images.shape
    assert images.dtype == torch.uint8 and labels.dtype == torch.uint8 and labels.shape == (N, H, W)
    assert images.is_contiguous() and labels.is_contiguous()
    dev = images.device
    tab = np.zeros((N, 2 * W + 2 * H), np.int32)
    for n, dr in enumerate(draws):
        if dr is not None:
            tab[n] = warp_tables(H, W, *dr)
    fl = torch.as_tensor(np.asarray([0 if dr is None else 1 for dr in draws], np.int32).reshape(N)).to(dev)
    tab = torch.as_tensor(tab).to(dev)
    out, lout = torch.empty_like(images), torch.empty_like(labels)
    lib().aug_warp_nn_u8(images.data_ptr(), out.data_ptr(), labels.data_ptr(), lout.data_ptr(), fl.data_ptr(), tab.data_ptr(), N, H, W,
                         _stream())
    return out, lout


def random_zoom_rotate(images, labels, rotate_range=30, zoom_range=0.2, prob=0.3):
    """random_zoom_rotate (common/data_utils.py:241-273) for a batch.  Per image, in the reference's order: random.gauss(0,
    rotate_range), random.gauss(1, zoom_range) -- both drawn whatever `prob` decides -- then rand() < prob"""
    import random
    draws = []
    for _ in range(images.shape[0]):
        angle = random.gauss(mu=0.0, sigma=rotate_range) if rotate_range else 0.0
        scale = random.gauss(mu=1.0, sigma=zoom_range) if zoom_range else 1.0
        warp = rand() < prob
        draws.append((angle, scale) if warp and (rotate_range or zoom_range) else None)
    if all(dr is None for dr in draws):
        return images, labels
    return warp_affine_nn(images, labels, draws)


def clahe(images, flags, out=None):
    """cv2.cvtColor(BGR2YUV), cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply on channel 0, cv2.cvtColor(YUV2BGR) for the
    images whose flags[n] are set; the others are copied.  out may be images"""
    N, H, W, C = images.shape
    assert images.dtype == torch.uint8 and C == 3 and images.is_contiguous()
    if H < 8 or W < 8:
        raise ValueError('CLAHE on an 8 x 8 tile grid needs H, W >= 8, got %d x %d' % (H, W))
    fl = torch.as_tensor(np.asarray(flags, np.int32).reshape(N)).to(images.device)
    out = torch.empty_like(images) if out is None else out
    luts = torch.empty(N * 64 * 256, dtype=torch.uint8, device=images.device)
    lib().aug_clahe_u8(images.data_ptr(), out.data_ptr(), fl.data_ptr(), luts.data_ptr(), luts.numel(), N, H, W, _stream())
    return out


def random_histeq(images, size=8, prob=.2):
    if size != 8:
        raise ValueError('the device kernel restates CLAHE on the 8 x 8 tile grid (the generator\'s default size)')
    flags = [1 if rand() < prob else 0 for _ in range(images.shape[0])]
    if not any(flags):
        return images
    return clahe(images, flags)


def nearest_axis(dst, src):
    """cv2.INTER_NEAREST: the source index of every destination index, min(floor(d * scale), src - 1), scale = 1 / (dst / src)"""
    scale = 1.0 / (float(dst) / src)
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * scale), src - 1)


def _linear_axis(dst, src, zero_at_edges):
    scale = 1.0 / (float(dst) / src)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if zero_at_edges:                                       # horizontal: the weight goes to the clamped pixel alone
        edge = (s < 0) | (s >= src - 1)
        f = np.where(edge, np.float32(0), f).astype(np.float32)
        s = np.clip(s, 0, src - 1)
        s1 = np.minimum(s + 1, src - 1)
    else:                                                   # vertical: the weights stay, the two rows are clamped
        s, s1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    w0 = np.clip(np.rint((np.float32(1) - f) * np.float32(2048)), -32768, 32767)
    w1 = np.clip(np.rint(f * np.float32(2048)), -32768, 32767)
    return [s, s1, w0, w1, nearest_axis(dst, src)]


def resize_tables(h, w, H, W):
    """the 5 W + 5 H integers dl3p_aug_resize_u8 takes, {sx, x1, a0, a1, nx}[W] then {sy0, sy1, b0, b1, ny}[H]: cv2.resize's
    INTER_LINEAR source indices and 11-bit weights from scale = 1 / (dst / src) in float64 (weights formed in float32), and the
    INTER_NEAREST indices min(floor(d * scale), src - 1)"""
    return np.concatenate(_linear_axis(W, w, True) + _linear_axis(H, h, False)).astype(np.int32)


def _rows_of(t, row_bytes):
    """the row pitch in bytes of a (N, h, w[, 3]) uint8 tensor whose rows are dense and whose images follow each other h rows apart"""
    N, h = t.shape[0], t.shape[1]
    assert t.dtype == torch.uint8 and (t.dim() == 3 or (t.stride(3) == 1 and t.stride(2) == 3)) and (t.dim() == 4 or t.stride(2) == 1)
    pitch = t.stride(1)
    assert pitch >= row_bytes and (N == 1 or t.stride(0) == h * pitch), 'resize: images must lie h rows apart'
    return pitch


def resize(images, labels, shape, out=None):
    """cv2.resize(image, shape[::-1]) (INTER_LINEAR) and cv2.resize(label, shape[::-1], interpolation=INTER_NEAREST) for a batch;
    shape = (H, W).  The inputs may be row-pitched views (a crop window).  out = (images_out, labels_out): dense uint8 tensors of
    N * H * W * 3 and N * H * W bytes to write into, e.g. one slot of a batch; made here when None"""
    N, h, w, _ = images.shape
    H, W = shape
    assert labels.shape == (N, h, w)
    dev = images.device
    if out is None:
        out = (torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev), torch.empty((N, H, W), dtype=torch.uint8, device=dev))
    oi, ol = out
    assert oi.dtype == torch.uint8 and ol.dtype == torch.uint8 and oi.is_contiguous() and ol.is_contiguous()
    assert oi.numel() == N * H * W * 3 and ol.numel() == N * H * W
    tab = torch.as_tensor(resize_tables(h, w, H, W)).to(dev)
    lib().aug_resize_u8(images.data_ptr(), _rows_of(images, 3 * w), oi.data_ptr(), labels.data_ptr(), _rows_of(labels, w), ol.data_ptr(),
                        tab.data_ptr(), N, h, w, H, W, _stream())
    return oi, ol


# ------------------------------------------------------------------------------------------------ PIL Image.resize (BICUBIC)
PIL_MAX_KSIZE = 65          # coefficients per output sample the kernel holds: a shrink by up to 16


def _bicubic(v):
    """Pillow's bicubic_filter (a = -0.5) on a float64 array, each operation rounded once in the order Pillow's C evaluates it"""
    a = -0.5
    t = np.abs(v)
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def _pil_axis(src, dst):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis -> (min[dst], cnt[dst], k[dst][ksize]) int32"""
    scale = float(src) / float(dst)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    if ksize > PIL_MAX_KSIZE:
        raise ValueError('pil_resize: %d -> %d needs %d coefficients per sample; the kernel holds %d (a shrink by up to 16)'
                         % (src, dst, ksize, PIL_MAX_KSIZE))
    ss = 1.0 / fs
    center = (np.arange(dst, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)              # (int) truncates towards zero, like astype
    cnt = np.minimum((center + support + 0.5).astype(np.int64), src) - lo
    tap = np.arange(ksize, dtype=np.int64)
    live = tap[None, :] < cnt[:, None]
    w = np.where(live, _bicubic(((tap[None, :] + lo[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(dst, np.float64)
    for t in range(ksize):                                                      # Pillow sums in tap order (np.sum would pair up)
        ww = ww + w[:, t]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << 22))
    return lo.astype(np.int32), cnt.astype(np.int32), np.where(live, k, 0).astype(np.int32)


def pil_resize_tables(h, w, H, W, filter='bicubic'):
    """the integers dl3p_pil_resize_u8 takes for Image.resize((W, H), BICUBIC) of an (h, w) image -> (tables, kx, ky): per axis
    {min[out], cnt[out], k[out][ksize]} -- first source sample, number of taps, and Pillow's coefficients in 22-bit fixed point from
    scale = in / out in float64 -- the horizontal axis first; an axis that keeps its length has no pass, no section and ksize 0"""
    if filter != 'bicubic':
        raise ValueError("pil_resize_tables: only 'bicubic' is built (got %r)" % (filter,))
    parts, ks = [], []
    for src, dst in ((w, W), (h, H)):
        if src == dst:
            ks.append(0)
            continue
        lo, cnt, k = _pil_axis(src, dst)
        parts += [lo, cnt, k.reshape(-1)]
        ks.append(k.shape[1])
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), ks[0], ks[1]


@functools.lru_cache(maxsize=8)
def _pil_tables_on(device, h, w, H, W):
    """pil_resize_tables on `device`; kept per size pair, so a stream of equal frames builds and uploads its tables once"""
    tables, kx, ky = pil_resize_tables(h, w, H, W)
    return (torch.as_tensor(tables).to(device) if tables.size else None), kx, ky


def pil_resize(images, shape, out=None):
    """PIL's Image.fromarray(image).resize(shape[::-1], Image.BICUBIC) for a batch (N, h, w, 3) of CUDA uint8 images, bit for bit;
    shape = (H, W).  The input may be a row-pitched view (a crop window).  out: a dense uint8 tensor of N * H * W * 3 bytes to write
    into, e.g. one slot of a batch; made here when None.  Raises ValueError for a shrink by more than 16 along either axis."""
    N, h, w, _ = images.shape
    H, W = int(shape[0]), int(shape[1])
    if H < 1 or W < 1:
        raise ValueError('pil_resize: the output size must be at least 1 x 1 (got %r)' % ((H, W),))
    dev = images.device
    tab, kx, ky = _pil_tables_on(dev, h, w, H, W)
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == N * H * W * 3
    L = lib()
    nws = L.pil_resize_workspace(N, h, w, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    L.pil_resize_u8(images.data_ptr(), _rows_of(images, 3 * w), out.data_ptr(), ws.data_ptr() if nws else None, nws,
                    tab.data_ptr() if tab is not None else None, kx, ky, N, h, w, H, W, _stream())
    return out
