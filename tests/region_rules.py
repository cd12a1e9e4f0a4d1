"""The region losses (soft Dice, soft Jaccard, Tversky) restated in float64 NumPy from the rule in DESIGN section 7.  Shares nothing
with the product code: the tests compare the device's results against these functions.  The full-resolution logits come from
mining_rules.bilinear_logits, the float64 restatement of the bilinear head's resize."""
import numpy as np

from mining_rules import bilinear_logits, pixel_losses  # noqa: F401  (re-exported for the tests)


def valid_pixels(labels, C, ignore_index):
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    masked = (lab == ignore_index) if ignore_index else np.zeros(lab.shape, bool)
    return lab, ~masked & (lab >= 0) & (lab < C)


def softmax(logits):
    v = np.asarray(logits, np.float64)
    v = v.reshape(-1, v.shape[-1])
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def sums(logits, labels, ignore_index=255):
    """logits (..., C) at full resolution, labels (...) -> (I, P, Y) [C] each over the valid pixels, (prob [P, C], lab, valid)"""
    prob = softmax(logits)
    C = prob.shape[1]
    lab, valid = valid_pixels(labels, C, ignore_index)
    onehot = np.zeros_like(prob)
    onehot[np.nonzero(valid)[0], lab[valid]] = 1.0
    pv = prob * valid[:, None]
    return (pv * onehot).sum(axis=0), pv.sum(axis=0), onehot.sum(axis=0), (prob, lab, valid, onehot)


def coefficients(I, P, Y, alpha, beta, smooth, rho=1.0):
    """-> dict(loss = rho R, present = |S|, score = T [C] (NaN outside S), A [C], B [C])"""
    S = Y > 0
    n = int(S.sum())
    C = I.size
    T = np.full(C, np.nan)
    A, B = np.zeros(C), np.zeros(C)
    if n == 0:
        return dict(loss=0.0, present=0, score=T, A=A, B=B)
    rest = 1.0 - alpha - beta
    D = rest * I[S] + alpha * P[S] + beta * Y[S] + smooth
    num = I[S] + smooth
    T[S] = num / D
    A[S] = rho * (1.0 / D - rest * num / D ** 2) / n
    B[S] = rho * (alpha * num / D ** 2) / n
    return dict(loss=float(rho * (1.0 - T[S]).sum() / n), present=n, score=T, A=A, B=B)


def region(logits, labels, alpha, beta, smooth=1.0, rho=1.0, ignore_index=255):
    """-> dict(I, P, Y, loss, present, score, A, B, grad): grad = d (rho R) / d logits, the shape of logits, 0 at invalid pixels"""
    I, P, Y, (prob, lab, valid, onehot) = sums(logits, labels, ignore_index)
    out = coefficients(I, P, Y, alpha, beta, smooth, rho)
    g = (out['B'][None, :] - onehot * out['A'][None, :]) * valid[:, None]
    grad = prob * (g - (prob * g).sum(axis=1, keepdims=True))
    out.update(I=I, P=P, Y=Y, grad=grad.reshape(np.shape(logits)))
    return out


def value(logits, labels, alpha, beta, smooth=1.0, rho=1.0, ignore_index=255):
    I, P, Y, _ = sums(logits, labels, ignore_index)
    return coefficients(I, P, Y, alpha, beta, smooth, rho)['loss']


def base_gradient(logits, labels, loss=('ce',), ignore_index=255, pixel_weights=None):
    """d (mean over ALL pixels of the per-pixel loss) / d logits in float64 -> (loss, grad): ce with p_y clipped to [1e-7, 1 - 1e-7]
    and no gradient outside, weighted -w[y] log p_y, focal -alpha (1 - p_y)^gamma log p_y (include/dl3p.h)"""
    prob = softmax(logits)
    n, C = prob.shape
    lab, valid = valid_pixels(labels, C, ignore_index)
    y = np.where(valid, lab, 0)
    pt = prob[np.arange(n), y]
    onehot = np.zeros_like(prob)
    onehot[np.arange(n), y] = 1.0
    if loss[0] == 'weighted':
        wy = np.asarray(loss[1], np.float64)[y]
        l, f = -wy * np.log(pt), wy
    elif loss[0] == 'focal':
        gamma, a = float(loss[1]), float(loss[2])
        pc = np.clip(pt, 1e-15, 1 - 1e-15)
        l = -a * (1 - pc) ** gamma * np.log(pc)
        f = a * ((1 - pc) ** gamma - gamma * (1 - pc) ** (gamma - 1) * pc * np.log(pc))
        f = np.where(pt >= 1e-15, f, 0.0)              # no gradient below the clip
    else:
        l = -np.log(np.clip(pt, 1e-7, 1 - 1e-7))
        f = ((pt > 1e-7) & (pt < 1 - 1e-7)).astype(np.float64)
    w = np.ones(n) if pixel_weights is None else np.asarray(pixel_weights, np.float64).reshape(-1)
    l, f = l * w * valid, f * w * valid
    grad = f[:, None] * (prob - onehot) / n
    return float(l.sum() / n), grad.reshape(np.shape(logits))
