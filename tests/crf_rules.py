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
"""
import functools

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


def kernel_matrices(img, sxy_gaussian=(3, 3), sxy_bilateral=80, srgb=13):
    """img (H, W, 3) uint8 -> (Kg, Kb), each (n, n) float64, k(i, j) over all pixel pairs in row-major order, diagonal = 1"""
    H, W, _ = img.shape
    y, x = np.mgrid[0:H, 0:W]
    x = x.reshape(-1).astype(np.float64)
    y = y.reshape(-1).astype(np.float64)
    rgb = img.reshape(-1, 3).astype(np.float64)
    sx, sy = (sxy_gaussian if isinstance(sxy_gaussian, (tuple, list)) else (sxy_gaussian, sxy_gaussian))

    def sq(f):
        return (f[:, None] - f[None, :]) ** 2
    kg = np.exp(-0.5 * (sq(x / sx) + sq(y / sy)))
    d = sq(x / sxy_bilateral) + sq(y / sxy_bilateral)
    for ch in range(3):
        d = d + sq(rgb[:, ch] / srgb)
    return kg, np.exp(-0.5 * d)


def messages(img, V, **kw):
    """the raw message sums: V (n, L) -> (Kg @ V, Kb @ V) in float64"""
    kg, kb = kernel_matrices(img, **kw)
    V = np.asarray(V, np.float64)
    return kg @ V, kb @ V


def _softmax_present(logit, present):
    """softmax over the present columns of (n, C) logits; exactly 0 elsewhere"""
    out = np.zeros_like(logit)
    z = logit[:, present]
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    out[:, present] = e / e.sum(axis=1, keepdims=True)
    return out


def dense_crf(img, mask, C, iterations=5, gt_prob=0.7, sxy_gaussian=(3, 3), compat_gaussian=3, sxy_bilateral=80, srgb=13,
              compat_bilateral=10, dtype=np.float64, self_term=True, symmetric=True, count_absent=False, kernels=None):
    """img (H, W, 3) uint8, mask (H, W) class ids -> (refined mask (H, W) int32, Q (H, W, C) of `dtype`).
    self_term / symmetric / count_absent switch on the wiring mistakes the end-to-end bound has to tell apart (tests only);
    kernels: kernel_matrices(img, ...) where the caller has them already."""
    H, W, _ = img.shape
    m = np.asarray(mask).reshape(-1).astype(np.int64)
    present = np.zeros(C, bool)
    present[np.unique(m)] = True
    n_labels = C if count_absent else int(present.sum())
    q = np.zeros((H * W, C), dtype)
    if present.sum() == 1:
        q[:, present] = 1
        return np.asarray(mask).astype(np.int32).copy(), q.reshape(H, W, C)
    neg_u = np.full((H * W, C), np.log((1 - gt_prob) / (n_labels - 1)), dtype)
    neg_u[np.arange(H * W), m] = np.log(gt_prob)
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
