"""Hard-example mining restated in float64 NumPy from the rule in DESIGN section 7 and the per-pixel loss formulas in include/dl3p.h.
Shares nothing with the product code: the tests compare the device's results against these functions."""
import numpy as np


def kept_count(P, p, M, s):
    """k of the rule: float64 in the order written, int() truncates, clamped to [1, P]"""
    P64, p64 = np.float64(P), np.float64(p)
    if M == 0:
        kd = p64 * P64
    else:
        r = min(np.float64(1.0), np.float64(s) / np.float64(M))
        kd = (r * p64 + (np.float64(1.0) - r)) * P64
    return max(1, min(int(P), int(kd)))


def rule(losses, p, M, s):
    """losses [P] (any float dtype; compared as they are) -> (k, theta, keep [P] bool, m, m_plus, scale float32):
    theta the k-th largest loss, every loss >= theta kept (all ties), m of them, m_plus of them non-zero, scale = P / max(m_plus, 1)"""
    l = np.array(losses).reshape(-1)
    l = l + l.dtype.type(0)                      # -0.0 -> +0.0
    P = l.size
    k = kept_count(P, p, M, s)
    theta = np.partition(l, P - k)[P - k]
    keep = l >= theta
    m = int(keep.sum())
    m_plus = int((keep & (l != 0)).sum())
    scale = np.float32(np.float64(P) / np.float64(max(m_plus, 1)))
    return k, theta, keep, m, m_plus, scale


def mined_loss(losses, p, M, s):
    """the public loss: sum over the kept / max(m_plus, 1), float64"""
    l = np.asarray(losses, np.float64).reshape(-1)
    _, _, keep, _, m_plus, _ = rule(losses, p, M, s)
    return float(l[keep].sum() / max(m_plus, 1))


# ---------------------------------------------------------------------------------------------- per-pixel losses of the heads
def _axis(out, inn):
    """tf.image.resize half-pixel coordinates in float32, as dl3p_resize_bilinear_fwd states them: src = (o + 0.5) * in / out - 0.5;
    lo = max(floor(src), 0); hi = min(ceil(src), in - 1); t = src - floor(src)"""
    scale = np.float32(inn) / np.float32(out)
    src = (np.arange(out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    fl = np.floor(src)
    lo = np.maximum(fl.astype(np.int64), 0)
    hi = np.minimum(np.ceil(src).astype(np.int64), inn - 1)
    return lo, hi, (src - fl).astype(np.float64)


def bilinear_logits(z, H, W):
    """z (N,h,w,C) -> (N,H,W,C) float64"""
    z = np.asarray(z, np.float64)
    _, h, w, _ = z.shape
    ylo, yhi, ty = _axis(H, h)
    xlo, xhi, tx = _axis(W, w)
    tx, ty = tx[None, None, :, None], ty[None, :, None, None]
    top = z[:, ylo][:, :, xlo] + (z[:, ylo][:, :, xhi] - z[:, ylo][:, :, xlo]) * tx
    bot = z[:, yhi][:, :, xlo] + (z[:, yhi][:, :, xhi] - z[:, yhi][:, :, xlo]) * tx
    return top + (bot - top) * ty


def nearest_logits(z, r):
    return np.repeat(np.repeat(np.asarray(z, np.float64), r, axis=1), r, axis=2)


def pixel_losses(logits, labels, loss=('ce',), ignore_index=255, pixel_weights=None):
    """logits (N,H,W,C) at full resolution, labels (N,H,W) -> l (N*H*W) float64: the loss kind's value, times (label != ignore and
    0 <= label < C), times the pixel weight.  ce: -log(clip(p_y, 1e-7, 1 - 1e-7)); weighted: -w[y] log(p_y); focal:
    -alpha (1 - p_y)^gamma log(p_y) with p_y clipped to [1e-15, 1 - 1e-15]"""
    v = np.asarray(logits, np.float64)
    C = v.shape[-1]
    v = v.reshape(-1, C)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    masked = (lab == ignore_index) if ignore_index else np.zeros(lab.shape, bool)
    valid = ~masked & (lab >= 0) & (lab < C)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True)
    y = np.where(valid, lab, 0)
    pt = prob[np.arange(v.shape[0]), y]
    if loss[0] == 'weighted':
        l = -np.asarray(loss[1], np.float64)[y] * np.log(pt)
    elif loss[0] == 'focal':
        gamma, alpha = float(loss[1]), float(loss[2])
        pc = np.clip(pt, 1e-15, 1 - 1e-15)
        l = -alpha * (1 - pc) ** gamma * np.log(pc)
    else:
        l = -np.log(np.clip(pt, 1e-7, 1 - 1e-7))
    if pixel_weights is not None:
        l = l * np.asarray(pixel_weights, np.float64).reshape(-1)
    return np.where(valid, l, 0.0) + 0.0
