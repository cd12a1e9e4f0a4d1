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
    """-> ('ce',) | ('weighted', weights) | ('focal', gamma, alpha): what the head kernel (and the oracle) need"""
    if isinstance(loss, WeightedSparseCategoricalCrossEntropy):
        return ('weighted', loss.weights)
    if isinstance(loss, SparseSoftmaxFocalLoss):
        return ('focal', float(loss.gamma), float(loss.alpha))
    return ('ce',)


def mining_spec(loss):
    """-> None (every pixel trains: top_k_percent_pixels == 1.0) | (p, M): the loss and its gradient come from the
    k = int((r p + 1 - r) P) highest-loss pixels of the batch, r = min(1, step / M) (csrc/mining.hip)"""
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
