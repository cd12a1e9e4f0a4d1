"""The multi-scale / mirrored evaluation rule in float64 NumPy, on top of oracle.np_ops.resize_bilinear_fwd, and
the inputs the op-level tests share.

The rule: every pass's low-resolution logits are upsampled to the base resolution (half-pixel bilinear), turned into probabilities
(softmax over the classes), a mirrored pass's probabilities are reversed along x, and all T passes enter one sum with weight 1 / T
in the order scale by scale, plain before mirrored; the prediction is the argmax of the sum, lowest index on ties.

Inputs are built so that near-ties are rare in the rule itself: per image a 3 x 3 scene of class ids, every logit map standard normal
noise plus 4.0 on the scene class of its pixel (the scene reversed along x for the mirrored maps).  Independent random maps leave up to
0.8 % of the pixels with their two best sums within the comparison tolerance; these leave none in the cases below."""
import functools

import numpy as np

from oracle import np_ops

# twice the probability tolerance (rtol 1e-4, atol 1e-6) at p <= 1: closer sums than this may legitimately swap in fp32
NEAR_TIE = 2.1e-4
RTOL, ATOL = 1e-4, 1e-6          # test_head_softmax_ce's tolerance on probabilities; it holds for a weighted mean of such terms

# (N, H, W, C, logit map sizes, ldz or None = C rounded up to 4)
CASES = (
    (2, 33, 33, 21, ((9, 9), (5, 5), (17, 17)), None),
    (1, 20, 28, 4, ((5, 7), (10, 14)), 20),
    (1, 40, 33, 32, ((9, 9), (3, 4), (20, 17)), None),          # the register path's last class count
    (1, 40, 33, 33, ((9, 9), (3, 4), (20, 17)), None),          # the class walk's first
    (2, 17, 23, 3, ((5, 7), (17, 23)), None),                   # odd W: a centre column; h = H
    (1, 33, 33, 253, ((9, 9), (5, 5)), None),
    (1, 9, 9, 1, ((3, 3),), None),
    (1, 65, 129, 19, ((17, 33), (9, 17)), None),
)
CASE_IDS = ['%dx%dx%dx%d' % c[:4] for c in CASES]


def softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def pass_probs(z, H, W, mirrored=False):
    """(N,h,w,C) logits of one pass -> its (N,H,W,C) float64 contribution before weighting"""
    p = softmax(np_ops.resize_bilinear_fwd(np.asarray(z, np.float64), H, W))
    return p[:, :, ::-1, :] if mirrored else p


def rule(zs, zms, H, W):
    """zs: the plain logit maps scale by scale; zms: the mirrored ones (same length) or None -> the (N,H,W,C) float64 sum"""
    T = len(zs) * (2 if zms is not None else 1)
    w = 1.0 / T
    acc = 0.0
    for i, z in enumerate(zs):
        acc = acc + w * pass_probs(z, H, W)
        if zms is not None:
            acc = acc + w * pass_probs(zms[i], H, W, mirrored=True)
    return acc


def top_two_gap(acc):
    """per pixel, the distance between the two largest sums (inf with one class)"""
    if acc.shape[-1] == 1:
        return np.full(acc.shape[:-1], np.inf)
    s = np.sort(acc, axis=-1)
    return s[..., -1] - s[..., -2]


@functools.lru_cache(maxsize=None)
def case_inputs(i):
    """-> (zs, zms): float32 (N,h,w,C) logit maps of case i, plain and mirrored, read-only"""
    N, H, W, C, maps, _ = CASES[i]
    rng = np.random.default_rng(C + H)
    scene = rng.integers(0, C, (N, 3, 3))
    zs, zms = [], []
    # draw order: the scene, every plain map, then every mirrored map (with this order no pixel of any case has its two best sums
    # closer than NEAR_TIE; test_tta_cpu.py holds every case to a share of at most 1e-3)
    for out, sc in ((zs, scene), (zms, scene[:, :, ::-1])):
        for (h, w) in maps:
            sy, sx = (np.arange(h) * 3) // h, (np.arange(w) * 3) // w
            z = rng.standard_normal((N, h, w, C)) * 1.0
            cls = sc[:, sy][:, :, sx]                                     # (N,h,w): the scene class of each logit pixel
            np.put_along_axis(z, cls[..., None], np.take_along_axis(z, cls[..., None], -1) + 4.0, -1)
            z = z.astype(np.float32)
            z.setflags(write=False)
            out.append(z)
    return tuple(zs), tuple(zms)


@functools.lru_cache(maxsize=None)
def case_rule(i):
    """-> (acc float64 (N,H,W,C), argmax, top-two gap) of case i, all passes, read-only"""
    N, H, W, C, _, _ = CASES[i]
    zs, zms = case_inputs(i)
    acc = rule(zs, zms, H, W)
    acc.setflags(write=False)
    return acc, acc.argmax(-1), top_two_gap(acc)
