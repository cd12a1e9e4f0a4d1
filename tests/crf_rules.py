"""The dense-CRF rule in float64 NumPy, by brute force over all pixel pairs, and the cases the CPU and GPU tests share.

The rule is the reference's deeplabv3p/postprocess_np.py (crf_postprocess with zero_unsure=False: unary_from_labels, one Gaussian and
one bilateral pairwise term) with pydensecrf's defaults DIAG_KERNEL, NORMALIZE_SYMMETRIC and Potts compatibility -- except that the
filter is the exact sum over all pixels where pydensecrf approximates it on a permutohedral lattice:

  present classes     those that occur in the mask; n_labels their count (np.unique's compaction; an absent class has U = +inf, Q = 0)
  unary               U_i(l) = -log(gt_prob) where m_i == l, -log((1 - gt_prob) / (n_labels - 1)) for every other present class
  kernels             k(i, j) = exp(-|f_i - f_j|^2 / 2), j == i included: Gaussian f = (x / 3, y / 3), weight 3;
                      bilateral f = (x / 80, y / 80, r / 13, g / 13, b / 13), weight 10
  normalisation       norm_i = 1 / sqrt(sum_j k(i, j) + 1e-20) per kernel
  iteration           Q0 = softmax(-U); Q <- softmax(-U + sum_kernels w norm_i sum_j k(i, j) norm_j Q_j), 5 times
  result              argmax_l Q_i(l), lowest class id on ties; a mask with one present class comes back unchanged
  ids outside [0, C)  (the reference has none: np.unique would make a class of each) are not counted as a class and carry no
                      evidence: U_i(l) is the "every other class" value for every present l; the pixel takes part in the messages like
                      any other; with fewer than two present classes the mask comes back unchanged, these ids included

Below the rule: the single pieces the device computes (messages with a scale on pixel j, the two normalisers, one update from given
messages), each with a per-element bound counted from the kernels' operations, and EDGE_CASES, the scenes of
tests/test_crf_edges_gpu.py with non-default parameters and launch-geometry edges.
"""
import functools
import zlib

import numpy as np

NEAR_TIE = 4e-3              # a pixel whose two best Q lie closer than this may take either class on the device
NEAR_TIE_CAP = 0.01          # at most this share of a case's pixels may be such near-ties
Q_ATOL = 2e-3                # |Q_device - Q_rule| on every entry
LP = 32                      # columns of a class-vector row on the device

# (N, H, W, C, present classes per image)
CASES = [
    (1, 19, 23, 3, [{0, 2}]),
    (2, 33, 31, 21, [{0, 3, 7, 15, 20}, {1, 20}]),          # 1023 pixels: one short of a multiple of the 128-pixel tile
    (1, 26, 40, 32, [set(range(32))]),                      # 1040 pixels: just past one
    (1, 1, 37, 4, [{1, 2, 3}]),
    (1, 24, 24, 2, [{0, 1}]),
    (1, 9, 9, 5, [{4}]),                                    # a single label
]
# one seed per case, chosen so that no image saturates: at least AMBIGUOUS_MIN of the pixels of every image with more than one
# class keep a Q entry in (0.02, 0.98) after 5 iterations (most seeds of the two-class scenes collapse to one class)
SEEDS = [10, 10, 16, 7, 6, 0]
AMBIGUOUS_MIN = 0.19
CASE_IDS = ['19x23c3', '2x33x31c21', '26x40c32', '1x37c4', '24x24c2', '9x9c5-single']


def _sq(f):
    return (f[:, None] - f[None, :]) ** 2


def _positions(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64)


def gauss_exponents(H, W, sxy=(3, 3)):
    """-> (n, n) float64, the natural-log exponent a(i, j) <= 0 of the Gaussian kernel: k = exp(a)"""
    x, y = _positions(H, W)
    sx, sy = (sxy if isinstance(sxy, (tuple, list)) else (sxy, sxy))
    return -0.5 * (_sq(x / sx) + _sq(y / sy))


def bilateral_exponents(img, sxy=80, srgb=13):
    """img (H, W, 3) uint8 -> (n, n) float64, the natural-log exponent a(i, j) <= 0 of the bilateral kernel"""
    H, W, _ = img.shape
    x, y = _positions(H, W)
    rgb = img.reshape(-1, 3).astype(np.float64)
    d = _sq(x / sxy) + _sq(y / sxy)
    for ch in range(3):
        d = d + _sq(rgb[:, ch] / srgb)
    return -0.5 * d


def kernel_matrices(img, sxy_gaussian=(3, 3), sxy_bilateral=80, srgb=13):
    """img (H, W, 3) uint8 -> (Kg, Kb), each (n, n) float64, k(i, j) over all pixel pairs in row-major order, diagonal = 1"""
    H, W, _ = img.shape
    return np.exp(gauss_exponents(H, W, sxy_gaussian)), np.exp(bilateral_exponents(img, sxy_bilateral, srgb))


def _scaled(V, scale):
    """V (n, L) with the factor of pixel j on row j; V itself without a scale"""
    V = np.asarray(V, np.float64)
    return V if scale is None else V * np.asarray(scale, np.float64).reshape(-1, 1)


def messages(img, V, scale=None, **kw):
    """the raw message sums: V (n, L) -> (Kg @ V, Kb @ V) in float64.  scale: one factor per pixel j, (n,), or a pair of them
    (Gaussian, bilateral): out_i = sum_j k(i, j) scale_j V_j"""
    kg, kb = kernel_matrices(img, **kw)
    sg, sb = scale if isinstance(scale, (tuple, list)) else (scale, scale)
    return kg @ _scaled(V, sg), kb @ _scaled(V, sb)


def gauss_norm(H, W, sxy=(3, 3)):
    """-> (n,) float64: 1 / sqrt(sum_j k(i, j) + 1e-20) of the Gaussian kernel"""
    return 1 / np.sqrt(np.exp(gauss_exponents(H, W, sxy)).sum(axis=1) + 1e-20)


def bilateral_norm(img, sxy=80, srgb=13):
    """-> (n,) float64: 1 / sqrt(sum_j k(i, j) + 1e-20) of the bilateral kernel"""
    return 1 / np.sqrt(np.exp(bilateral_exponents(img, sxy, srgb)).sum(axis=1) + 1e-20)


# ---- per-element bounds: U * (roundings) * (sum of |terms|), U = 2^-24, counted from the kernels' operations; nothing is fitted.
#
# A message element is sum_j k_ij s_j v_j with non-negative terms.  Per term: the product s_j v_j (1 rounding), the product with k
# and the running sum (the Gaussian's fmaf: 1, the MFMA: at most 2), so a chain of n terms is within (n + 2) U of its sum whatever
# the order; the separable Gaussian adds W then H terms instead of n, which is less.  k itself: the exponent is formed in fp32 from
# exact integer distances by two scalings (each factor rounded once on the host, each product once) and their sum, i.e. at most
# 4 roundings of quantities no larger than |a_ij| -- a relative error 4 |a_ij| U on k -- and the exponential adds one ulp (the
# MI355X guides give no figure for v_exp_f32; the ISA's 1 ulp and expf's are taken).  The 64 holds these few per-term roundings
# with a wide margin, as in tests/test_crf_gpu.py:
#     |d out_ic| <= U sum_j k_ij s_j v_jc (n + 64 + 4 |a_ij|)
# At the default parameters and low contrast |a| stays below a few units and this is the (n + 64) U of test_crf_gpu.  A k below the
# smallest normal float (|a| > 87) may be flushed to 0, and so may a product k s v: TINY = 2^-126 per term, absolutely.
# The normalisers 1 / sqrt(S + 1e-20): S >= 1 (the self term), so adding 1e-20 changes no bit; the relative bound of S halves
# through the square root, which and the division round once each (both correctly rounded): d norm <= norm (dS / 2S + 2 U).
U = 2.0 ** -24
TINY = 2.0 ** -126


def message_bound(a, V, scale=None):
    """a (n, n) exponents, V (n, L) >= 0 -> (n, L): the bound on |device - float64| of every element of exp(a) @ (scale V)"""
    n = a.shape[0]
    sv = _scaled(V, scale)
    assert sv.min() >= 0
    return U * ((np.exp(a) * (n + 64 + 4 * np.abs(a))) @ sv) + TINY * (n + sv.sum(axis=0))[None, :]


def norm_bound(a):
    """a (n, n) exponents -> (n,): the bound on |device - float64| of 1 / sqrt(row sum + 1e-20)"""
    s = np.exp(a).sum(axis=1)
    ds = message_bound(a, np.ones((a.shape[0], 1)))[:, 0]
    return (0.5 * ds / s + 2 * U) / np.sqrt(s + 1e-20)


# One update: logit_c = u_c + (wg ng_i) fg_ic + (wb nb_i) fb_ic over the present classes, Q = softmax.  Each message term is
# rounded at most 4 times (weight x normaliser, x message, two additions), the unary term 3 times (logf, two additions): 4 U of the
# sum of |terms|.  The argument of the logarithm adds an absolute part: gt_prob becomes a float (U / 2 relative, U / 2 on log gt,
# (U / 2) gt / (1 - gt) on log(1 - gt)), the subtraction and the division round once each -> U (1 + gt / (1 - gt)).
# x_c = logit_c - max is rounded once (U |x_c|; the maximum is one float for all classes of the pixel, so its own error cancels in
# the ratio); the fast exponential scales its argument by log2(e) and takes one v_exp_f32: (|x_c| + 4) U relative, the issue's
# figure.  With e_c (1 + r_c): |dQ_c| <= Q_c (r_c + sum_k Q_k r_k) to first order -- at most the 2 Q_c max r -- and the five
# additions of the butterfly, the division and the second-order terms are 8 U more.  An exponential below the smallest normal
# float may come out as 0: TINY.
def _present(m, C):
    inside = (m >= 0) & (m < C)
    present = np.zeros(C, bool)
    present[np.unique(m[inside])] = True
    return inside, present


def _update(mask, C, fg, ng, fb, nb, wg, wb, gt_prob):
    m = np.asarray(mask).reshape(-1).astype(np.int64)
    n = m.size
    inside, present = _present(m, C)
    nl = int(present.sum())
    q = np.zeros((n, C))
    if nl < 2:
        q[:, present] = 1
        return q, m.astype(np.int32), np.full(n, np.inf), np.zeros((n, C))
    terms = np.zeros((3, n, C))
    terms[0] = np.log((1 - gt_prob) / (nl - 1))
    terms[0][np.arange(n)[inside], m[inside]] = np.log(gt_prob)
    for t, (w, f, nrm) in enumerate(((wg, fg, ng), (wb, fb, nb)), 1):
        if f is not None:
            terms[t] = w * np.asarray(nrm, np.float64).reshape(-1, 1) * np.asarray(f, np.float64)[:, :C]
    logit = terms.sum(axis=0)
    x = logit[:, present] - logit[:, present].max(axis=1, keepdims=True)
    e = np.exp(x)
    qp = e / e.sum(axis=1, keepdims=True)
    q[:, present] = qp
    dlogit = U * (4 * np.abs(terms).sum(axis=0)[:, present] + 1 + gt_prob / (1 - gt_prob))
    r = dlogit + U * np.abs(x) + U * (np.abs(x) + 4)
    dq = np.zeros((n, C))
    dq[:, present] = qp * (r + (qp * r).sum(axis=1, keepdims=True) + 8 * U) + TINY
    return q, q.argmax(axis=1).astype(np.int32), top_two_gap(q), dq


def update(mask, C, fg, ng, fb, nb, wg, wb, gt_prob):
    """one step of the rule from given messages, over the present classes: mask (n,) class ids, fg / fb (n, >= C) message sums or
    None, ng / nb (n,) normalisers -> (Q (n, C), argmax (n,) int32 with the lowest id on ties, top-two gap (n,)).
    Ids outside [0, C) are not counted and carry no evidence (see dense_crf); with fewer than two present classes the mask comes
    back as it is, Q is 1 in the present column and the gap is inf."""
    return _update(mask, C, fg, ng, fb, nb, wg, wb, gt_prob)[:3]


def update_bound(mask, C, fg, ng, fb, nb, wg, wb, gt_prob):
    """-> (n, C): the bound on |device - float64| of every Q of update()"""
    return _update(mask, C, fg, ng, fb, nb, wg, wb, gt_prob)[3]


def _softmax_present(logit, present):
    """softmax over the present columns of (n, C) logits; exactly 0 elsewhere"""
    out = np.zeros_like(logit)
    z = logit[:, present]
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    out[:, present] = e / e.sum(axis=1, keepdims=True)
    return out


def dense_crf(img, mask, C, iterations=5, gt_prob=0.7, sxy_gaussian=(3, 3), compat_gaussian=3, sxy_bilateral=80, srgb=13,
              compat_bilateral=10, dtype=np.float64, self_term=True, symmetric=True, count_absent=False, count_outside=False,
              kernels=None):
    """img (H, W, 3) uint8, mask (H, W) class ids -> (refined mask (H, W) int32, Q (H, W, C) of `dtype`).
    A class id outside [0, C) is not counted as a class and carries no evidence: the pixel's unary term is that of "another class"
    for every present class; it takes part in the messages like any pixel and gets a class where the image has at least two.  An
    image with fewer than two present classes comes back unchanged, such ids included (Q = 1 in the present column, if there is one).
    self_term / symmetric / count_absent / count_outside switch on the wiring mistakes the end-to-end bound has to tell apart
    (tests only); kernels: kernel_matrices(img, ...) where the caller has them already."""
    H, W, _ = img.shape
    m = np.asarray(mask).reshape(-1).astype(np.int64)
    inside, present = _present(m, C)
    n_labels = C if count_absent else int(present.sum()) + int(count_outside and not inside.all())
    q = np.zeros((H * W, C), dtype)
    if present.sum() < 2:
        q[:, present] = 1
        return np.asarray(mask).astype(np.int32).copy(), q.reshape(H, W, C)
    neg_u = np.full((H * W, C), np.log((1 - gt_prob) / (n_labels - 1)), dtype)
    neg_u[np.arange(H * W)[inside], m[inside]] = np.log(gt_prob)
    ks = [k.astype(dtype) for k in (kernels or kernel_matrices(img, sxy_gaussian, sxy_bilateral, srgb))]
    if not self_term:
        for k in ks:
            np.fill_diagonal(k, 0)
    ws = (dtype(compat_gaussian), dtype(compat_bilateral))
    norms = [1 / np.sqrt(k.sum(axis=1) + dtype(1e-20)) for k in ks]
    q = _softmax_present(neg_u, present)
    for _ in range(iterations):
        logit = neg_u.copy()
        for k, w, nrm in zip(ks, ws, norms):
            if symmetric:
                logit = logit + w * nrm[:, None] * (k @ (nrm[:, None] * q))
            else:
                logit = logit + w * (nrm * nrm)[:, None] * (k @ q)
        q = _softmax_present(logit, present)
    return q.argmax(axis=1).astype(np.int32).reshape(H, W), q.reshape(H, W, C)


def top_two_gap(q):
    """(..., C) -> the difference of the two largest entries per pixel (inf for C == 1)"""
    if q.shape[-1] < 2:
        return np.full(q.shape[:-1], np.inf)
    s = np.sort(q, axis=-1)
    return s[..., -1] - s[..., -2]


# ---- ambiguous scenes: a saturated CRF (every Q within 1e-3 of 0 or 1) hides every mistake behind the softmax
def ambiguous_scene(rng, H, W, present):
    """a 3 x 3 block scene of the present classes whose colours lie within +-12 of one base colour, pixel noise of sigma 10, and
    35 % of the labels redrawn at random among the present classes -> (img (H, W, 3) uint8, mask (H, W) int32)"""
    present = np.array(sorted(present))
    blocks = present[rng.permutation(9) % len(present)].reshape(3, 3)
    truth = blocks[(np.arange(H) * 3 // H)[:, None], (np.arange(W) * 3 // W)[None, :]]
    base = rng.integers(80, 176, 3)
    colour = {int(c): base + rng.integers(-12, 13, 3) for c in present}
    img = np.stack([np.vectorize(lambda c, ch=ch: colour[int(c)][ch])(truth) for ch in range(3)], axis=-1).astype(np.float64)
    img = np.clip(np.rint(img + rng.normal(0, 10, img.shape)), 0, 255).astype(np.uint8)
    mask = truth.copy()
    redraw = rng.uniform(size=mask.shape) < 0.35
    mask[redraw] = rng.choice(present, int(redraw.sum()))
    # every present class occurs: plant the ones the draw left out, one pixel each along the flattened image
    flat = mask.reshape(-1)
    missing = [c for c in present if c not in flat]
    for k, c in enumerate(missing):
        flat[(k * 7919) % flat.size] = c
    assert set(np.unique(flat)) == set(int(c) for c in present)
    return img, mask.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case_inputs(i):
    """-> (images (N, H, W, 3) uint8, masks (N, H, W) int32) of case i; computed once, read-only"""
    N, H, W, C, present = CASES[i]
    rng = np.random.default_rng(SEEDS[i])
    imgs, masks = zip(*(ambiguous_scene(rng, H, W, present[b]) for b in range(N)))
    imgs, masks = np.stack(imgs), np.stack(masks)
    imgs.setflags(write=False)
    masks.setflags(write=False)
    return imgs, masks


@functools.lru_cache(maxsize=None)
def case_rule(i):
    """-> (masks (N, H, W) int32, Q (N, H, W, C) float64, top-two gap (N, H, W)) of the rule on case i; computed once, read-only"""
    N, H, W, C, _ = CASES[i]
    imgs, masks = case_inputs(i)
    out = [dense_crf(imgs[b], masks[b], C) for b in range(N)]
    m = np.stack([o[0] for o in out])
    q = np.stack([o[1] for o in out])
    gap = top_two_gap(q)
    for a in (m, q, gap):
        a.setflags(write=False)
    return m, q, gap


def case_v(i):
    """a non-negative random V (N, H*W, LP) float32 for the message tests: exact zeros in the absent and the padding columns"""
    N, H, W, C, present = CASES[i]
    rng = np.random.default_rng(2000 + i)
    v = rng.uniform(0, 1, (N, H * W, LP)).astype(np.float32)
    for b in range(N):
        absent = [c for c in range(LP) if c not in present[b]]
        v[b][:, absent] = 0
    return v


# ---- edge cases: non-default parameters and the launch geometry the six shared cases do not reach (tests/test_crf_edges_gpu.py)
# (N, H, W, C, present classes per image, keyword arguments of dense_crf); every row names the mechanism it is there for
EDGE_CASES = [
    # every parameter off its default, sx != sy, a row of 70 positions: two chunks of the Gaussian row pass, the second partial
    (1, 5, 70, 4, [{0, 1, 3}], dict(sxy_gaussian=(5, 2), sxy_bilateral=40, srgb=20, compat_gaussian=2, compat_bilateral=6,
                                    iterations=3, gt_prob=0.6)),
    # the same for the column pass (70 rows: three output tiles of 32), sx < sy, a single iteration
    (1, 70, 6, 3, [{0, 2}], dict(sxy_gaussian=(2, 6), iterations=1)),
    # a line of 260: the table loop past 256 and five chunks; two images with different class sets and normalisers
    (2, 3, 260, 6, [{1, 2, 5}, {0, 4}], {}),
    # n = 256: exactly one chunk of the bilateral walk and two full 128-row tiles
    (1, 16, 16, 2, [{0, 1}], {}),
    # n = 512: two full chunks; the last class id of 21; two iterations
    (1, 32, 16, 21, [{0, 5, 20}], dict(iterations=2)),
]
EDGE_SEEDS = [1, 0, 12, 5, 1]
EDGE_IDS = ['5x70c4-all-params', '70x6c3-1it', '2x3x260c6', '16x16c2', '32x16c21-2it']
OUTSIDE_BASE = 3                 # the edge case whose scene test_crf_edges_gpu also runs with class ids outside [0, C) planted
OUTSIDE_IDS = (-1, 2, 255)       # below 0, C itself, the ignore label of the data sets


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def edge_inputs(i):
    """-> (images (N, H, W, 3) uint8, masks (N, H, W) int32) of edge case i; computed once, read-only"""
    N, H, W, C, present, _ = EDGE_CASES[i]
    rng = np.random.default_rng(EDGE_SEEDS[i])
    imgs, masks = zip(*(ambiguous_scene(rng, H, W, present[b]) for b in range(N)))
    return _frozen(np.stack(imgs), np.stack(masks))


def _rule(imgs, masks, C, kw):
    out = [dense_crf(imgs[b], masks[b], C, **kw) for b in range(len(imgs))]
    q = np.stack([o[1] for o in out])
    return _frozen(np.stack([o[0] for o in out]), q, top_two_gap(q))


@functools.lru_cache(maxsize=None)
def edge_rule(i):
    """-> (masks, Q float64, top-two gap) of the rule on edge case i with its keyword arguments; computed once, read-only"""
    return _rule(*edge_inputs(i), EDGE_CASES[i][3], EDGE_CASES[i][5])


@functools.lru_cache(maxsize=None)
def outside_inputs():
    """edge case OUTSIDE_BASE with twelve pixels relabelled to the ids of OUTSIDE_IDS -> (images, masks), read-only"""
    imgs, masks = edge_inputs(OUTSIDE_BASE)
    masks = masks.copy()
    flat = masks.reshape(-1)
    at = np.random.default_rng(77).permutation(flat.size)[:12]
    flat[at] = np.resize(OUTSIDE_IDS, 12)
    assert set(np.unique(flat)) == EDGE_CASES[OUTSIDE_BASE][4][0] | set(OUTSIDE_IDS)
    return _frozen(imgs, masks)


@functools.lru_cache(maxsize=None)
def outside_rule():
    return _rule(*outside_inputs(), EDGE_CASES[OUTSIDE_BASE][3], EDGE_CASES[OUTSIDE_BASE][5])


# ---- the single kernels.  Gaussian: (H, W, sx, sy) -- lines of 1, 63, 64, 65, 129 and 257 positions on either axis (the chunk of
# 64 source positions, the tile of 32 outputs, the table's stride of 256), sx != sy; the long axis of the 257s has a wide sigma so
# that table[256] carries weight (exp(-256^2 / 2 / 150^2) = 0.23)
GAUSS_SHAPES = [(1, 1, 3, 2), (3, 63, 7, 2), (63, 3, 2, 7), (2, 64, 9, 1.5), (64, 2, 1.5, 9), (5, 65, 8, 2.5), (65, 5, 2.5, 8),
                (3, 129, 20, 2), (129, 3, 2, 20), (3, 257, 150, 1.5), (257, 3, 1.5, 150)]
# bilateral: (H, W) -- n = 1, 127, 128, 129 (the 128-row tile), 256, 257 (the 256-row chunk), 512
BILATERAL_SHAPES = [(1, 1), (1, 127), (8, 16), (3, 43), (16, 16), (1, 257), (16, 32)]
# image kind -> (sxy, srgb): two flat regions of 0 and 255 with small noise under a narrow colour sigma (exponents down to -1200:
# k underflows to exactly 0 across the regions), uniformly random bytes under a wide one (exponents spread over 0 .. -80)
BILATERAL_KINDS = {'two-region': (25, 9), 'random-bytes': (60, 35)}
PRESENT_COLUMNS = (0, 2, 3, 17, 31)        # the columns of V that hold numbers in the message tests; the others are exactly 0


def message_v(seed, N, n):
    """(N, n, LP) float32, uniform in (0, 1) in PRESENT_COLUMNS and exactly 0 elsewhere"""
    v = np.zeros((N, n, LP), np.float32)
    v[..., PRESENT_COLUMNS] = np.random.default_rng(seed).uniform(0, 1, (N, n, len(PRESENT_COLUMNS)))
    return v


def message_scale(seed, *shape):
    """float32 factors in (0.1, 1), the range of a normaliser"""
    return np.random.default_rng(seed).uniform(0.1, 1, shape).astype(np.float32)


def bilateral_image(kind, seed, N, H, W):
    """(N, H, W, 3) uint8"""
    rng = np.random.default_rng(seed)
    if kind == 'random-bytes':
        return rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    img = np.zeros((N, H * W, 3), np.float64)
    img[:, (H * W) // 2:] = 255                  # (n = 1: one region)
    return np.clip(np.rint(img + rng.normal(0, 3, img.shape)), 0, 255).astype(np.uint8).reshape(N, H, W, 3)


# update: name -> (N, n, C, ids per image (the present classes and, beyond them, ids outside [0, C)), gt_prob, wg, wb)
UPDATE_CASES = {
    'grid-stride': (2, 16384 + 9, 21, [(0, 3, 7, 15, 20), (1, 20)], 0.7, 3.0, 10.0),     # past the grid cap, a last partial sweep
    'odd-7': (1, 7, 4, [(1, 2, 3)], 0.7, 3.0, 10.0),                                      # one workgroup, its last half wave idle
    'gt-0.3': (1, 37, 5, [(1, 4)], 0.3, 2.0, 6.0),
    'outside': (2, 301, 6, [(0, 2, 5, -1, 6, 255), (3, 255)], 0.7, 3.0, 10.0),             # the second image: one present class
}


@functools.lru_cache(maxsize=None)
def update_inputs(name):
    """-> (mask (N, n) int32, fg (N, n, LP), ng (n,), fb (N, n, LP), nb (N, n)) float32, read-only: random non-negative messages
    in every column (absent and padding columns included: the kernel must mask them) and normalisers in (0.1, 1)"""
    N, n, C, ids, _, _, _ = UPDATE_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    mask = np.stack([np.asarray(ids[b], np.int32)[rng.integers(0, len(ids[b]), n)] for b in range(N)])
    for b in range(N):
        mask[b, :len(ids[b])] = ids[b]           # every id occurs
    fg, fb = (rng.uniform(0, 2, (N, n, LP)).astype(np.float32) for _ in range(2))
    ng = rng.uniform(0.1, 1, n).astype(np.float32)
    nb = rng.uniform(0.1, 1, (N, n)).astype(np.float32)
    return _frozen(mask, fg, ng, fb, nb)
