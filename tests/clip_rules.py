"""Gradient clipping of the Keras 2.11 legacy OptimizerV2 (clipvalue, clipnorm, global_clipnorm) restated in NumPy: the oracle of
tests/test_grad_clip_gpu.py.  Nothing here is shared with the product code.

What is clipped is the gradient of the whole loss, g' = g * grad_scale + 2 * l2 * w, as a float32 (the optimiser kernels form it
with one fused multiply-add on the float32 product 2 * l2 * w; `loss_gradient` restates exactly that, see there).  Variables are
given as a list of arrays, the freeze mask as a list of boolean arrays (True = trainable); frozen elements enter no norm and
keep their INPUT gradient g.  Order: clipvalue, then clipnorm (per variable) or global_clipnorm (one scale).  Norms, the
comparison and the quotient are float64; the scale is rounded once to float32:
    s = c / max(norm, c)   with a max that propagates NaN: exactly 1 at or below the threshold, 0 for an infinite per-variable
    norm, NaN for a NaN norm, and NaN for every variable when the GLOBAL norm is not finite (tf.clip_by_global_norm)."""
import numpy as np


def loss_gradient(g, w, l2, grad_scale):
    """float32 fmaf(g, grad_scale, (2 * l2) * w): the product 2 * l2 * w is rounded to float32 as the kernels round it (2 * l2 is
    exact), the multiply-add is evaluated in float64 and rounded to float32.  g * grad_scale is exact in float64 (24 x 24 bits).
    For grad_scale a power of two it is a float32 itself and the float64 sum of two float32 values rounds to float32 as the
    exact sum does (no double rounding: a float32 plus a term more than 29 bits below it cannot land on a float32 midpoint), so
    the result is bit-exact; the tests use 1 and 1/8."""
    g, w, l2 = (np.asarray(a, np.float32) for a in (g, w, l2))
    t = (np.float32(2.0) * l2) * w
    with np.errstate(invalid='ignore', over='ignore'):
        return (g.astype(np.float64) * np.float64(np.float32(grad_scale)) + t.astype(np.float64)).astype(np.float32)


def _scale(norm, c, global_rule=False):
    if global_rule and not np.isfinite(norm):
        return np.float32(np.nan)
    if np.isnan(norm):
        return np.float32(np.nan)
    if norm <= c:
        return np.float32(1.0)
    return np.float32(np.float64(c) / np.float64(norm))


def clip(gp, trainable, clipvalue=None, clipnorm=None, global_clipnorm=None):
    """gp: list of float32 arrays (g' per variable), trainable: list of boolean arrays.
    -> dict(norm=[per variable..., global] float64, scale=[per variable] float32, clipped=[float32 arrays: float32(g') after the
    clamp], product=[float64 arrays: clipped * scale, unrounded]); entries of frozen elements in clipped / product are NaN-free
    placeholders (0) and mean nothing."""
    assert clipnorm is None or global_clipnorm is None
    clipped, sumsq = [], []
    for v, on in zip(gp, trainable):
        v = np.asarray(v, np.float32).copy()
        if clipvalue is not None:
            c = np.float32(clipvalue)
            with np.errstate(invalid='ignore'):
                v = np.where(v < -c, -c, np.where(v > c, c, v)).astype(np.float32)
        v = np.where(on, v, np.float32(0))
        clipped.append(v)
        with np.errstate(invalid='ignore', over='ignore'):
            sumsq.append(np.sum(v.astype(np.float64) ** 2))
    with np.errstate(invalid='ignore', over='ignore'):
        norms = [np.sqrt(s) for s in sumsq]
        gnorm = np.sqrt(np.sum(np.array(sumsq, np.float64)))
    if global_clipnorm is not None:
        scales = [_scale(gnorm, global_clipnorm, True)] * len(gp)
    elif clipnorm is not None:
        scales = [_scale(n, clipnorm) for n in norms]
    else:
        scales = [np.float32(1.0)] * len(gp)
    with np.errstate(invalid='ignore', over='ignore'):
        product = [c.astype(np.float64) * np.float64(s) for c, s in zip(clipped, scales)]
    return dict(norm=np.array(norms + [gnorm], np.float64), scale=np.array(scales, np.float32), clipped=clipped, product=product)
