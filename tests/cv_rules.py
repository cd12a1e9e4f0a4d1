"""The OpenCV steps of the reference's generator restated in NumPy: cv2.warpAffine (INTER_NEAREST, BORDER_CONSTANT 0) as
random_zoom_rotate calls it, cvtColor(BGR2YUV) + createCLAHE(2.0, (8, 8)).apply + cvtColor(YUV2BGR) as random_histeq calls them, and
cv2.resize (INTER_LINEAR image, INTER_NEAREST label).  The oracle of tests/test_augment_cv_gpu.py; nothing here is shared with the
product code.

UNPINNED: OpenCV is not installed where this suite runs, so nothing checks these functions against OpenCV itself.  They restate its
published 8-bit algorithms (imgproc: imgwarp.cpp, clahe.cpp, color_yuv, resize.cpp) rule by rule, as DESIGN.md section 7 writes the
rules out, and the known answers of tests/test_augment_cv_cpu.py are answers of THIS restatement."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _round_i32(v):
    """cvRound to int32 with saturation: round half to even"""
    return np.clip(np.rint(np.asarray(v, np.float64)), I32_MIN, I32_MAX).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- warpAffine
def rotation_matrix(center, angle, scale):
    """cv2.getRotationMatrix2D in float64"""
    a = np.float64(angle) * np.pi / 180.0
    alpha, beta = np.float64(scale) * np.cos(a), np.float64(scale) * np.sin(a)
    cx, cy = np.float64(center[0]), np.float64(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def invert_affine(M):
    """warpAffine without WARP_INVERSE_MAP inverts the 2 x 3 matrix in place, in this order of operations"""
    m = [np.float64(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else np.float64(0.0)
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] = m[1] * -D
    m[3] = m[3] * -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def warp_tables(H, W, angle, scale):
    """(adelta[W], bdelta[W], X0[H], Y0[H]) int32 of a rotation by `angle` degrees and zoom `scale` about (W // 2, H // 2)"""
    m = invert_affine(rotation_matrix((W // 2, H // 2), angle, scale))
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    adelta = _round_i32(m[0] * x * 1024)
    bdelta = _round_i32(m[3] * x * 1024)
    X0 = _round_i32((m[1] * y + m[2]) * 1024) + 512
    Y0 = _round_i32((m[4] * y + m[5]) * 1024) + 512
    return tuple(np.asarray(t).astype(np.int32) for t in (adelta, bdelta, X0, Y0))     # (+ 512 wraps like an int addition)


def warp_nn(img, angle, scale):
    """img (H, W) or (H, W, C) uint8"""
    H, W = img.shape[:2]
    adelta, bdelta, X0, Y0 = warp_tables(H, W, angle, scale)
    X = np.clip((X0[:, None] + adelta[None, :]) >> 10, -32768, 32767)           # int32 sum (wraps), arithmetic shift, sat16
    Y = np.clip((Y0[:, None] + bdelta[None, :]) >> 10, -32768, 32767)
    ok = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    src = img[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)]
    return np.where(ok if img.ndim == 2 else ok[..., None], src, 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- cvtColor, CLAHE
def _descale(v):
    return (v + 8192) >> 14


def bgr2yuv(img):
    c = img.astype(np.int64)
    c0, c2 = c[..., 0], c[..., 2]
    Y = np.clip(_descale(c0 * 1868 + c[..., 1] * 9617 + c2 * 4899), 0, 255)
    U = np.clip(_descale((c0 - Y) * 8061 + (128 << 14)), 0, 255)
    V = np.clip(_descale((c2 - Y) * 14369 + (128 << 14)), 0, 255)
    return np.stack([Y, U, V], -1).astype(np.uint8)


def yuv2bgr(yuv):
    c = yuv.astype(np.int64)
    Y, U, V = c[..., 0], c[..., 1] - 128, c[..., 2] - 128
    c0 = Y + _descale(U * 33292)
    c1 = Y + _descale(U * -6472 + V * -9519)
    c2 = Y + _descale(V * 18678)
    return np.clip(np.stack([c0, c1, c2], -1), 0, 255).astype(np.uint8)


def clahe_luts(plane, clip_limit=2.0):
    """(8, 8, 256) uint8 LUTs of an (H, W) uint8 plane, and the tile size (th, tw)"""
    H, W = plane.shape
    if H < 8 or W < 8:
        raise ValueError('an 8 x 8 tile grid needs H, W >= 8')
    ph, pw = (8 - H % 8) % 8, (8 - W % 8) % 8
    ext = np.pad(plane, ((0, ph), (0, pw)), mode='reflect') if (ph or pw) else plane          # numpy 'reflect' = BORDER_REFLECT_101
    th, tw = ext.shape[0] // 8, ext.shape[1] // 8
    area = th * tw
    clip = max(int(clip_limit * area / 256), 1)
    lut_scale = np.float32(255.0) / np.float32(area)
    luts = np.zeros((8, 8, 256), np.uint8)
    for ty in range(8):
        for tx in range(8):
            h = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            clipped = int(np.maximum(h - clip, 0).sum())
            h = np.minimum(h, clip)
            batch = clipped // 256
            residual = clipped - 256 * batch
            h += batch
            if residual != 0:
                step = max(256 // residual, 1)
                i = 0
                while i < 256 and residual > 0:
                    h[i] += 1
                    i += step
                    residual -= 1
            s = np.cumsum(h).astype(np.float32) * lut_scale                    # float32 product, rounded once
            luts[ty, tx] = np.clip(np.rint(s), 0, 255).astype(np.uint8)
    return luts, (th, tw)


def clahe_plane(plane):
    H, W = plane.shape
    luts, (th, tw) = clahe_luts(plane)
    f32 = np.float32

    def axis(n, t):
        tf = np.arange(n, dtype=f32) * (f32(1.0) / f32(t)) - f32(0.5)
        t1 = np.floor(tf)
        a = tf - t1
        t1 = t1.astype(np.int64)
        return np.maximum(t1, 0), np.minimum(t1 + 1, 7), f32(1.0) - a, a
    ty1, ty2, ya1, ya = axis(H, th)
    tx1, tx2, xa1, xa = axis(W, tw)
    v = plane.astype(np.int64)
    L = luts.astype(f32)
    g = lambda ty, tx: L[ty[:, None], tx[None, :], v]
    top = g(ty1, tx1) * xa1[None, :] + g(ty1, tx2) * xa[None, :]               # float32 throughout, one rounding per operation
    bot = g(ty2, tx1) * xa1[None, :] + g(ty2, tx2) * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def histeq(img):
    """random_histeq's three calls on an (H, W, 3) uint8 image"""
    yuv = bgr2yuv(img)
    yuv[..., 0] = clahe_plane(yuv[..., 0])
    return yuv2bgr(yuv)


# ---------------------------------------------------------------------------------------------------- resize
def _linear_axis(dst, src, zero_at_edges):
    """source index, its neighbour and the 11-bit weights of INTER_LINEAR along one axis"""
    scale = 1.0 / (np.float64(dst) / src)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if zero_at_edges:
        lo, hi = s < 0, s >= src - 1
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        s1 = np.minimum(s + 1, src - 1)
    else:
        s, s1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    w0 = np.clip(np.rint((np.float32(1.0) - f) * np.float32(2048)), -32768, 32767).astype(np.int64)
    w1 = np.clip(np.rint(f * np.float32(2048)), -32768, 32767).astype(np.int64)
    return s, s1, w0, w1


def _nearest_axis(dst, src):
    scale = 1.0 / (np.float64(dst) / src)
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * scale).astype(np.int64), src - 1)


def resize_linear(img, shape):
    """cv2.resize(img, (W, H)) of an (h, w[, C]) uint8 image, shape = (H, W)"""
    h, w = img.shape[:2]
    H, W = shape
    if (h, w) == (H, W):
        return img.copy()
    s = img.astype(np.int64)
    if h == 2 * H and w == 2 * W:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, x1, a0, a1 = _linear_axis(W, w, True)
    sy0, sy1, b0, b1 = _linear_axis(H, h, False)
    ex = (slice(None), slice(None)) + (None,) * (img.ndim - 2)
    T = s[:, sx] * a0[ex[1:]] + s[:, x1] * a1[ex[1:]]
    b0, b1 = b0[(slice(None), None) + (None,) * (img.ndim - 2)], b1[(slice(None), None) + (None,) * (img.ndim - 2)]
    out = (((b0 * (T[sy0] >> 4)) >> 16) + ((b1 * (T[sy1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def resize_nearest(label, shape):
    h, w = label.shape[:2]
    return label[_nearest_axis(shape[0], h)][:, _nearest_axis(shape[1], w)].copy()
