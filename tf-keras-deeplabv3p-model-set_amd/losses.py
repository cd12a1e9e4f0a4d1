"""The losses and metrics compile() takes (deeplabv3p/loss.py, deeplabv3p/metrics.py) as configuration holders for the head kernels, and
the host arithmetic on what the device counts: jaccard_from_counts, miou_from_confusion (eval.py:462-497)."""
import numpy as np


def _check_mining(top_k_percent_pixels, hard_example_mining_step):
    """the hard-example mining keywords every loss takes (DeepLab's train_utils.add_softmax_cross_entropy_loss_for_each_scale):
    0 < top_k_percent_pixels <= 1 (1.0: off), hard_example_mining_step an integer >= 0 (0: no ramp) -> (p, M)"""
    p, M = top_k_percent_pixels, hard_example_mining_step
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 < float(p) <= 1.0:
        raise ValueError('top_k_percent_pixels must lie in (0, 1], got %r' % (p,))
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or int(M) < 0:
        raise ValueError('hard_example_mining_step must be an integer >= 0, got %r' % (M,))
    return float(p), int(M)


class SparseCategoricalCrossEntropy(object):
    """deeplabv3p/loss.py:121-156: configuration holder -- the arithmetic is fused into the HIP head kernel"""

    def __init__(self, ignore_index=None, from_logits=False, *, top_k_percent_pixels=1.0, hard_example_mining_step=0):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits is not supported')
        self.top_k_percent_pixels, self.hard_example_mining_step = _check_mining(top_k_percent_pixels, hard_example_mining_step)
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.__name__ = 'sparse_categorical_crossentropy'


class WeightedSparseCategoricalCrossEntropy(object):
    """deeplabv3p/loss.py:159-191 (train.py:115, --weighted_type balanced): -w[y] * log(p_y)"""

    def __init__(self, weights, ignore_index=None, from_logits=False, *, top_k_percent_pixels=1.0, hard_example_mining_step=0):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits is not supported')
        self.top_k_percent_pixels, self.hard_example_mining_step = _check_mining(top_k_percent_pixels, hard_example_mining_step)
        self.weights = np.array(weights).astype('float32')
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.__name__ = 'weighted_sparse_categorical_crossentropy'


class SparseSoftmaxFocalLoss(object):
    """deeplabv3p/loss.py:63-118 (train.py:131, --loss focal): -alpha * (1 - p_y)^gamma * log(p_y)"""

    def __init__(self, gamma=2.0, alpha=0.25, ignore_index=None, from_logits=False, *, top_k_percent_pixels=1.0,
                 hard_example_mining_step=0):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits is not supported')
        self.top_k_percent_pixels, self.hard_example_mining_step = _check_mining(top_k_percent_pixels, hard_example_mining_step)
        self.gamma, self.alpha = gamma, alpha
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.__name__ = 'sparse_softmax_focal_loss'


def _finite_number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)):
        raise ValueError('%s must be a finite number, got %r' % (name, v))
    return float(v)


# what compile() answers where a region loss meets the nearest-upsampling head (Fast-SCNN)
REGION_NEAREST_TEXT = ('region losses (SparseTverskyLoss, SparseDiceLoss, SparseJaccardLoss) run behind the bilinear head only: the '
                      'nearest-upsampling head has no region kernels (a dl3p_nearest_region_sums and a dl3p_nearest_region_head_grad '
                      'next to dl3p_nearest_head_train are not built)')


class SparseTverskyLoss(object):
    """A region (overlap) loss on the model's softmax, alone or added to one of the per-pixel losses (DESIGN section 7,
    csrc/region_loss.hip).  Per class over the valid pixels of the batch: I = sum p [y == c], P = sum p, Y = |y == c|,
    T = (I + smooth) / ((1 - alpha - beta) I + alpha P + beta Y + smooth), i.e. (I + s) / (I + alpha FP + beta FN + s); the loss is
    the mean of 1 - T over the classes present in the labels (0 when none is).  alpha weighs false positives, beta false negatives.
    The compiled loss is base_weight * base + region_weight * that mean; base: None or a SparseCategoricalCrossEntropy,
    WeightedSparseCategoricalCrossEntropy or SparseSoftmaxFocalLoss with everything it carries (class weights, focal parameters,
    mining); sample weights act on the base term only."""

    def __init__(self, alpha=0.5, beta=0.5, smooth=1.0, ignore_index=None, from_logits=False, *, base=None, base_weight=1.0,
                 region_weight=1.0):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits=%r is not supported' % (from_logits,))
        self.alpha, self.beta = _finite_number('alpha', alpha), _finite_number('beta', beta)
        self.smooth = _finite_number('smooth', smooth)
        self.region_weight, self.base_weight = _finite_number('region_weight', region_weight), _finite_number('base_weight', base_weight)
        if self.alpha <= 0.0 or self.beta <= 0.0:
            raise ValueError('alpha and beta must be > 0, got alpha=%r beta=%r' % (alpha, beta))
        if self.smooth < 0.0:
            raise ValueError('smooth must be >= 0, got %r' % (smooth,))
        if self.region_weight <= 0.0:
            raise ValueError('region_weight must be > 0, got %r' % (region_weight,))
        if self.base_weight < 0.0:
            raise ValueError('base_weight must be >= 0, got %r' % (base_weight,))
        if base is not None and type(base) not in (SparseCategoricalCrossEntropy, WeightedSparseCategoricalCrossEntropy,
                                                   SparseSoftmaxFocalLoss):
            raise ValueError('base must be None or one of the per-pixel losses (SparseCategoricalCrossEntropy, '
                             'WeightedSparseCategoricalCrossEntropy, SparseSoftmaxFocalLoss), got %r' % (base,))
        if base is not None and base.ignore_index != ignore_index:
            raise ValueError('base.ignore_index=%r differs from ignore_index=%r: one label rule serves both terms'
                             % (base.ignore_index, ignore_index))
        self.base = base
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.__name__ = 'sparse_tversky_loss'


class SparseDiceLoss(SparseTverskyLoss):
    """soft Dice: Tversky with alpha = beta = 1/2, T = (2 I + 2 s) / (P + Y + 2 s)"""

    def __init__(self, smooth=1.0, ignore_index=None, from_logits=False, *, base=None, base_weight=1.0, region_weight=1.0):
        super().__init__(0.5, 0.5, smooth, ignore_index, from_logits, base=base, base_weight=base_weight,
                         region_weight=region_weight)
        self.__name__ = 'sparse_dice_loss'


class SparseJaccardLoss(SparseTverskyLoss):
    """soft Jaccard, the differentiable form of the IoU: Tversky with alpha = beta = 1, T = (I + s) / (P + Y - I + s)"""

    def __init__(self, smooth=1.0, ignore_index=None, from_logits=False, *, base=None, base_weight=1.0, region_weight=1.0):
        super().__init__(1.0, 1.0, smooth, ignore_index, from_logits, base=base, base_weight=base_weight,
                         region_weight=region_weight)
        self.__name__ = 'sparse_jaccard_loss'


def Jaccard(y_true=None, y_pred=None):
    """deeplabv3p/metrics.py:29-46, train.py:140 `metrics = {'pred_mask': Jaccard}`: a marker for compile(metrics=...);
    the counts come from dl3p_class_counts on the device and jaccard_from_counts evaluates them"""
    raise RuntimeError('Jaccard is evaluated on the device: pass it to compile(metrics=...)')


def jaccard_from_counts(counts):
    """counts (N,3,C) = per image [intersection, label pixels, predicted pixels] per class -> metrics.py:29-46"""
    c = np.asarray(counts, dtype=np.float64)
    inter, true, pred = c[:, 0], c[:, 1], c[:, 2]
    union = true + pred - inter
    legal = true > 0
    ious = []
    for i in range(c.shape[2]):
        if legal[:, i].any():
            ious.append(float(np.mean(inter[legal[:, i], i] / union[legal[:, i], i])))
    return float(np.mean(ious)) if ious else float('nan')


def _wants_jaccard(metrics):
    if not metrics:
        return False
    items = metrics.values() if isinstance(metrics, dict) else metrics
    flat = []
    for it in items:
        flat += list(it) if isinstance(it, (list, tuple)) else [it]
    return any(it is Jaccard or getattr(it, '__name__', it) == 'Jaccard' for it in flat)


def loss_spec(loss):
    """-> ('ce',) | ('weighted', weights) | ('focal', gamma, alpha): what the head kernel (and the oracle) need;
    a region loss: ('region', alpha, beta, smooth, region_weight, base_weight, the base's spec or None)"""
    if isinstance(loss, SparseTverskyLoss):
        return ('region', loss.alpha, loss.beta, loss.smooth, loss.region_weight, loss.base_weight,
                None if loss.base is None else loss_spec(loss.base))
    if isinstance(loss, WeightedSparseCategoricalCrossEntropy):
        return ('weighted', loss.weights)
    if isinstance(loss, SparseSoftmaxFocalLoss):
        return ('focal', float(loss.gamma), float(loss.alpha))
    return ('ce',)


def mining_spec(loss):
    """-> None (every pixel trains: top_k_percent_pixels == 1.0) | (p, M): the loss and its gradient come from the
    k = int((r p + 1 - r) P) highest-loss pixels of the batch, r = min(1, step / M) (csrc/mining.hip);
    a region loss mines what its base mines"""
    if isinstance(loss, SparseTverskyLoss):
        return None if loss.base is None else mining_spec(loss.base)
    p = float(getattr(loss, 'top_k_percent_pixels', 1.0))
    if p == 1.0:
        return None
    return (p, int(getattr(loss, 'hard_example_mining_step', 0)))


def miou_from_confusion(cm, class_names=None):
    """eval.py:462-497 on a (C,C) confusion matrix (rows = ground truth): PixelAcc, per-class ClassAcc / IoU / Dice /
    Freq, mClassAcc, mIoU (NaN -> 0 before the mean, like the reference), FWIoU"""
    cm = np.asarray(cm, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        inter = np.diag(cm)
        rows, cols, tot = cm.sum(axis=1), cm.sum(axis=0), cm.sum()
        pixel_acc = inter.sum() / tot
        class_acc = np.nan_to_num(inter / rows, nan=0.0)
        union = rows + cols - inter
        iou = np.nan_to_num(inter / union, nan=0.0)
        freq = np.nan_to_num(rows / tot, nan=0.0)
        dice = np.nan_to_num(2 * inter / (union + inter), nan=0.0)
    out = {'PixelAcc': float(pixel_acc), 'mClassAcc': float(class_acc.mean()), 'mIoU': float(iou.mean()),
           'FWIoU': float((freq[freq > 0] * iou[freq > 0]).sum()), 'IoU': iou, 'ClassAcc': class_acc, 'Dice': dice,
           'Freq': freq, 'confusion_matrix': cm}
    if class_names is not None:
        out['IoU_by_class'] = dict(sorted(zip(class_names, iou.tolist()), key=lambda kv: -kv[1]))
    return out
