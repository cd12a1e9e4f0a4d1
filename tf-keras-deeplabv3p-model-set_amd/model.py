"""create deeplabv3p models -- the drop-in counterpart of the reference's deeplabv3p/model.py:
`deeplab_model_map` (:23-48) and `get_deeplabv3p_model(model_type, num_classes, model_input_shape,
output_stride, freeze_level=0, weights_path=None, training=True, use_subpixel=False)` (:51-117), same
names, argument meaning and error behaviour.  What it returns is not a tf.keras.Model wrapping
TensorFlow ops but a `DeeplabModel` façade over the MI355X HIP executor, exposing what the reference's
callers use: compile / fit / fit_generator / train_on_batch / predict / summary / save / load_weights /
layers[i].trainable (train.py:155-247, eval.py:33-36, deeplab.py:71-113).
"""
import os
import sys
import time
from functools import partial

import numpy as np

from .graph import ACT_NONE
from .mobilenetv2 import Deeplabv3pMobileNetV2, Deeplabv3pLiteMobileNetV2

#
# A map of model type to construction function for DeepLabv3+ (reference model.py:23-48).  Entries that
# are out of this build's hot-path scope raise the same ValueError as an unknown key.
#
deeplab_model_map = {
    'mobilenetv2': partial(Deeplabv3pMobileNetV2, alpha=1.0),
    'mobilenetv2_lite': partial(Deeplabv3pLiteMobileNetV2, alpha=1.0),
}


def _register_optional():
    try:
        from .xception import Deeplabv3pXception
        deeplab_model_map['xception'] = Deeplabv3pXception
    except ImportError:
        pass
    try:
        from .mobilenetv3 import (Deeplabv3pMobileNetV3Large, Deeplabv3pLiteMobileNetV3Large,
                                  Deeplabv3pMobileNetV3Small, Deeplabv3pLiteMobileNetV3Small)
        deeplab_model_map['mobilenetv3large'] = partial(Deeplabv3pMobileNetV3Large, alpha=1.0)
        deeplab_model_map['mobilenetv3large_lite'] = partial(Deeplabv3pLiteMobileNetV3Large, alpha=1.0)
        deeplab_model_map['mobilenetv3small'] = partial(Deeplabv3pMobileNetV3Small, alpha=1.0)
        deeplab_model_map['mobilenetv3small_lite'] = partial(Deeplabv3pLiteMobileNetV3Small, alpha=1.0)
    except ImportError:
        pass
    try:
        from .resnet50 import Deeplabv3pResNet50
        deeplab_model_map['resnet50'] = Deeplabv3pResNet50
    except ImportError:
        pass
    try:
        from .peleenet import Deeplabv3pPeleeNet, Deeplabv3pLitePeleeNet
        deeplab_model_map['peleenet'] = Deeplabv3pPeleeNet
        deeplab_model_map['peleenet_lite'] = Deeplabv3pLitePeleeNet
    except ImportError:
        pass
    try:
        from .ghostnet import Deeplabv3pGhostNet, Deeplabv3pLiteGhostNet
        deeplab_model_map['ghostnet'] = Deeplabv3pGhostNet
        deeplab_model_map['ghostnet_lite'] = Deeplabv3pLiteGhostNet
    except ImportError:
        pass


_register_optional()


def _clip_args(clipnorm, clipvalue, global_clipnorm):
    """the clipping keywords of a Keras 2.11 legacy OptimizerV2 -> None | (clipvalue, clipnorm, global_clipnorm).  clipnorm and
    global_clipnorm together raise ValueError as Keras does; a value that is not a positive finite number raises ValueError too
    (our decision: Keras takes 0 and negative thresholds and then produces zero or sign-flipped gradients)."""
    if clipnorm is not None and global_clipnorm is not None:
        raise ValueError('Cannot accept both `clipnorm` and `global_clipnorm`, received clipnorm=%r, global_clipnorm=%r'
                         % (clipnorm, global_clipnorm))
    out = []
    for name, v in (('clipvalue', clipvalue), ('clipnorm', clipnorm), ('global_clipnorm', global_clipnorm)):
        if v is not None:
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError('%s must be a positive finite number, received %r' % (name, v))
            if not (v > 0.0 and np.isfinite(v)):
                raise ValueError('%s must be a positive finite number, received %r' % (name, v))
        out.append(v)
    return None if out == [None, None, None] else tuple(out)


class SGD:
    """Keras SGD(learning_rate, momentum=0.9, nesterov=False, clipnorm=None, clipvalue=None) (common/model_utils.py:123).
    clipvalue / clipnorm / global_clipnorm (all three optimisers): the gradient of the whole loss -- regulariser included, after
    the data-parallel all-reduce, trainable variables only -- is clamped to [-clipvalue, clipvalue], then scaled per variable to
    an L2 norm of at most clipnorm OR as a whole to a global norm of at most global_clipnorm, on the device
    (csrc/grad_clip.hip).  Both norms together, or a value that is not a positive finite number, raise ValueError."""

    def __init__(self, learning_rate=0.01, momentum=0.9, nesterov=False, clipnorm=None, clipvalue=None, global_clipnorm=None):
        if nesterov:
            raise ValueError('nesterov momentum is not on the hot path')
        self._clip = _clip_args(clipnorm, clipvalue, global_clipnorm)
        self.learning_rate, self.momentum = learning_rate, momentum
        self.iterations = 0          # Keras `optimizer.iterations`: a schedule starts at 0 with a NEW optimizer

    def clip_spec(self):
        """None | (clipvalue, clipnorm, global_clipnorm), None for a rule that is off"""
        return self._clip

    def lr_at(self, step):
        lr = self.learning_rate
        return float(lr(step)) if callable(lr) else float(lr)

    def spec(self):
        return ('sgd', float(self.momentum))


class Adam(SGD):
    """Keras Adam(learning_rate, epsilon=1e-7, amsgrad=False) (common/model_utils.py:119)"""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None):
        if amsgrad:
            raise ValueError('amsgrad is not built (the reference passes amsgrad=False)')
        self._clip = _clip_args(clipnorm, clipvalue, global_clipnorm)
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon
        self.momentum = 0.0
        self.iterations = 0

    def spec(self):
        return ('adam', float(self.beta_1), float(self.beta_2), float(self.epsilon))


class RMSprop(SGD):
    """Keras RMSprop(learning_rate, rho=0.9, momentum=0.0, centered=False) (common/model_utils.py:121)"""

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None):
        if momentum or centered:
            raise ValueError('RMSprop momentum / centered are not built (the reference uses momentum=0.0, centered=False)')
        self._clip = _clip_args(clipnorm, clipvalue, global_clipnorm)
        self.learning_rate, self.rho, self.epsilon = learning_rate, rho, epsilon
        self.momentum = 0.0
        self.iterations = 0

    def spec(self):
        return ('rmsprop', float(self.rho), float(self.epsilon))


class _AveragedOptimizer:
    """tensorflow-addons' optimizer wrappers (common/model_utils.py:133-172): the wrapped optimizer does its own update, the
    wrapper's rule then runs on the new weights in the same kernel (dl3p_*_avg).  learning_rate, lr_at, iterations and
    spec() are the wrapped optimizer's; avg_spec() is what the executor needs of the rule."""

    def __init__(self, optimizer, kwargs):
        if not isinstance(optimizer, SGD) or isinstance(optimizer, _AveragedOptimizer):
            raise ValueError('an averaged optimizer wraps SGD, Adam or RMSprop')
        if kwargs:
            raise ValueError('%s: %s not built (the reference passes none of them)'
                             % (type(self).__name__, ', '.join(sorted(kwargs))))
        self._optimizer = optimizer

    @property
    def learning_rate(self):
        return self._optimizer.learning_rate

    @learning_rate.setter
    def learning_rate(self, value):
        self._optimizer.learning_rate = value

    @property
    def iterations(self):
        return self._optimizer.iterations

    @iterations.setter
    def iterations(self, value):
        self._optimizer.iterations = value

    def lr_at(self, step):
        return self._optimizer.lr_at(step)

    def spec(self):
        return self._optimizer.spec()

    def clip_spec(self):
        return self._optimizer.clip_spec()


class MovingAverage(_AveragedOptimizer):
    """tfa.optimizers.MovingAverage(optimizer, average_decay=0.99): average <- average - (average - w) * (1 - decay) after
    every step (Keras moving_average_update, no zero-debias)"""

    def __init__(self, optimizer, average_decay=0.99, num_updates=None, start_step=0, dynamic_decay=False, **kwargs):
        if num_updates is not None or dynamic_decay or start_step:
            raise ValueError('MovingAverage num_updates / dynamic_decay / start_step are not built (the reference passes '
                             'average_decay only)')
        super().__init__(optimizer, kwargs)
        self.average_decay = average_decay

    def avg_spec(self):
        return ('ema', float(self.average_decay))


class SWA(_AveragedOptimizer):
    """tfa.optimizers.SWA(optimizer, start_averaging=0, average_period=10): a running mean of the weights at iterations
    start, start + period, start + 2 period, ... (iteration = step - 1)"""

    def __init__(self, optimizer, start_averaging=0, average_period=10, **kwargs):
        if average_period < 1:
            raise ValueError('average_period must be >= 1')
        if start_averaging < 0:
            raise ValueError('start_averaging must be >= 0')
        super().__init__(optimizer, kwargs)
        self.start_averaging, self.average_period = start_averaging, average_period

    def avg_spec(self):
        return ('swa', int(self.start_averaging), int(self.average_period))


class Lookahead(_AveragedOptimizer):
    """tfa.optimizers.Lookahead(optimizer, sync_period=6, slow_step_size=0.5): every sync_period steps
    slow <- slow + slow_step_size * (w - slow) and the weights are set to slow"""

    def __init__(self, optimizer, sync_period=6, slow_step_size=0.5, **kwargs):
        if sync_period < 1:
            raise ValueError('sync_period must be >= 1')
        super().__init__(optimizer, kwargs)
        self.sync_period, self.slow_step_size = sync_period, slow_step_size

    def avg_spec(self):
        return ('lookahead', int(self.sync_period), float(self.slow_step_size))


def get_averaged_optimizer(average_type, optimizer):
    """common/model_utils.py:133-172 with the reference's constants"""
    average_type = average_type.lower()
    if average_type == 'ema':
        return MovingAverage(optimizer, average_decay=0.99)
    if average_type == 'swa':
        return SWA(optimizer, start_averaging=0, average_period=10)
    if average_type == 'lookahead':
        return Lookahead(optimizer, sync_period=6, slow_step_size=0.5)
    raise ValueError('Unsupported average type')


def get_optimizer(optim_type, learning_rate, average_type=None, decay_type=None, decay_steps=100000, *, clipnorm=None,
                  clipvalue=None, global_clipnorm=None):
    """common/model_utils.py:112-172: 'sgd' (momentum 0.9), 'adam', 'rmsprop' with the four learning-rate schedules, wrapped
    by average_type 'ema' | 'swa' | 'lookahead'; clipnorm / clipvalue / global_clipnorm (the keywords :117-123 spell out as None)
    go to the optimiser"""
    clip = dict(clipnorm=clipnorm, clipvalue=clipvalue, global_clipnorm=global_clipnorm)
    optim_type = optim_type.lower()
    if optim_type not in ('sgd', 'adam', 'rmsprop'):
        raise ValueError('Unsupported optimizer type')
    if average_type:
        if not isinstance(average_type, str) or average_type.lower() not in ('ema', 'swa', 'lookahead'):
            raise ValueError('Unsupported average type')
        return get_averaged_optimizer(average_type, get_optimizer(optim_type, learning_rate, None, decay_type, decay_steps, **clip))
    lr = learning_rate
    if decay_type:
        d = decay_type.lower()
        if d == 'cosine':          # CosineDecay(alpha=0.2)
            lr = lambda s: learning_rate * (0.8 * 0.5 * (1 + np.cos(np.pi * min(s, decay_steps) / decay_steps)) + 0.2)
        elif d == 'exponential':   # ExponentialDecay(decay_rate=0.9)
            lr = lambda s: learning_rate * 0.9 ** (s / decay_steps)
        elif d == 'polynomial':    # PolynomialDecay(end=lr/100, power=1)
            lr = lambda s: (learning_rate - learning_rate / 100) * (1 - min(s, decay_steps) / decay_steps) + learning_rate / 100
        elif d == 'piecewise_constant':
            b = [500, int(decay_steps * 0.9), decay_steps]
            v = [0.001, learning_rate, learning_rate / 10., learning_rate / 100.]
            lr = lambda s: v[sum(1 for x in b if s > x)]
        else:
            raise ValueError('Unsupported lr decay type')
    if optim_type == 'adam':
        return Adam(lr, epsilon=1e-7, **clip)
    if optim_type == 'rmsprop':
        return RMSprop(lr, rho=0.9, **clip)
    return SGD(lr, momentum=0.9, **clip)


class SparseCategoricalCrossEntropy(object):
    """deeplabv3p/loss.py:121-156: configuration holder -- the arithmetic is fused into the HIP head kernel"""

    def __init__(self, ignore_index=None, from_logits=False):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits is not supported')
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.__name__ = 'sparse_categorical_crossentropy'


class WeightedSparseCategoricalCrossEntropy(object):
    """deeplabv3p/loss.py:159-191 (train.py:115, --weighted_type balanced): -w[y] * log(p_y)"""

    def __init__(self, weights, ignore_index=None, from_logits=False):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits is not supported')
        self.weights = np.array(weights).astype('float32')
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.__name__ = 'weighted_sparse_categorical_crossentropy'


class SparseSoftmaxFocalLoss(object):
    """deeplabv3p/loss.py:63-118 (train.py:131, --loss focal): -alpha * (1 - p_y)^gamma * log(p_y)"""

    def __init__(self, gamma=2.0, alpha=0.25, ignore_index=None, from_logits=False):
        if from_logits:
            raise ValueError('the model emits probabilities (Softmax pred_mask); from_logits is not supported')
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


class DistContext:
    """one process per GPU; collectives are RCCL (torch.distributed backend 'nccl') over xGMI.
    Gradient buckets are all-reduced on a side HIP stream so that they overlap the rest of backward."""

    def __init__(self, sync_bn=True, n_buckets=4):
        import torch.distributed as dist
        self.dist = dist
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.sync_bn = sync_bn
        self.n_buckets = n_buckets
        self._streams = {}
        self._bn_pg = None

    def all_reduce(self, t):
        """blocking (stream-ordered) sum all-reduce: SyncBatchNorm statistics of the forward pass"""
        self.dist.all_reduce(t, group=self._bn_group())

    def _bn_group(self):
        # SyncBatchNorm gets its own communicator (own RCCL stream): a statistics all-reduce never queues behind
        # a gradient bucket that is still on the wire.  DL3P_ONE_COMM=1 keeps everything on the default communicator
        # (one of the switches watchdog.FirstStepsGuard names when the first steps of a multi-rank job hang)
        if os.environ.get('DL3P_ONE_COMM', '0') not in ('', '0'):
            return None
        if self._bn_pg is None and self.dist.is_initialized() and self.dist.get_backend() == 'nccl':
            self._bn_pg = self.dist.new_group(backend='nccl')
        return self._bn_pg

    def broadcast(self, t, src=0):
        self.dist.broadcast(t, src)

    def _side(self, which):
        import torch
        if self._streams.get(which) is None:
            self._streams[which] = torch.cuda.Stream()
        return self._streams[which]

    def all_reduce_async(self, t):
        """sum all-reduce of a gradient bucket, ordered after everything already queued on the
        compute stream but running beside what is queued later"""
        import torch
        if not t.is_cuda:
            self.dist.all_reduce(t)
            return
        side = self._side('grad')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.dist.all_reduce(t)

    def wait_all(self):
        import torch
        if self._streams.get('grad') is not None:
            torch.cuda.current_stream().wait_stream(self._streams['grad'])

    def bn_all_reduce_begin(self, t):
        """SyncBatchNorm backward sums: start the all-reduce beside the compute stream (the deferred weight
        gradient of the previous layer runs meanwhile) ..."""
        import torch
        if not t.is_cuda:
            self.dist.all_reduce(t)
            return
        side = self._side('bn')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.dist.all_reduce(t, group=self._bn_group())

    def bn_all_reduce_end(self):
        """... and make the compute stream wait for it"""
        import torch
        if self._streams.get('bn') is not None:
            torch.cuda.current_stream().wait_stream(self._streams['bn'])


class StagedBatch:
    """a batch on its way to the device (BatchFeeder.put): device tensors with their host shapes, the staging slot they live in"""
    def __init__(self, slot, x, y, sample_weight):
        self.slot, self.x, self.y, self.sample_weight = slot, x, y, sample_weight


class BatchFeeder:
    """fit_generator's host -> device boundary (train.py:177-187 feeds numpy batches): TWO sets of pinned host buffers and device
    staging buffers and a copy stream, so that batch k + 1 crosses PCIe while the device runs step k.  put() copies the arrays into
    pinned memory (CPU) and starts the DMA on the copy stream; the consumer makes the compute stream wait for that DMA
    (consume), enqueues the step (whose first kernels read the staging buffers: uint8 -> float normalisation, label
    preparation) and releases the slot (release) -- the copy stream does not overwrite a slot before its last consumer ran."""
    def __init__(self, device='cuda'):
        import torch
        self.dev = device
        self.stream = torch.cuda.Stream()
        self.bufs = [{}, {}]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]
        self.free = [None, None]
        self.k = 0

    def _move(self, slot, name, a):
        import torch
        t = torch.as_tensor(a)
        shape = tuple(t.shape)
        if t.dtype not in (torch.uint8, torch.float32):
            t = t.to(torch.float32)
        t = t.reshape(-1)
        pair = self.bufs[slot].get(name)
        if pair is None or pair[0].numel() != t.numel() or pair[0].dtype != t.dtype:
            pair = self.bufs[slot][name] = (torch.empty(t.numel(), dtype=t.dtype, pin_memory=True),
                                            torch.empty(t.numel(), dtype=t.dtype, device=self.dev))
        host, dev = pair
        # one thread's memcpy (0.5 ms for 12.6 MB).  Tensor.copy_ spreads it over every core of the host and the OpenMP workers then
        # spin for their block time: on the 256-thread GPU box that starved the HIP runtime's own thread and a staged step took
        # 35 ms instead of 12 (scripts/micro/feed_dbg.py)
        np.copyto(host.numpy(), t.numpy())
        with torch.cuda.stream(self.stream):
            dev.copy_(host, non_blocking=True)
        return dev.view(shape)

    def put(self, x, y=None, sample_weight=None):
        slot = self.k & 1
        self.k += 1
        if getattr(x, 'is_cuda', False):
            # a batch made on the device (data.SegmentationGenerator, output='device'): nothing crosses PCIe, no pinned copy; the step
            # waits for the work that built it, which is whatever the current stream holds now
            import torch
            self.ready[slot].record(torch.cuda.current_stream())
            return StagedBatch(slot, x, y, sample_weight)
        self.ready[slot].synchronize()          # (the DMA that last read this slot's pinned buffers; long done)
        if self.free[slot] is not None:
            self.stream.wait_event(self.free[slot])
        sw = sample_weight
        out = StagedBatch(slot, self._move(slot, 'x', x), None if y is None else self._move(slot, 'y', y),
                          sw if (sw is None or isinstance(sw, str)) else self._move(slot, 'sw', sw))
        self.ready[slot].record(self.stream)
        return out

    def consume(self, staged):
        import torch
        torch.cuda.current_stream().wait_event(self.ready[staged.slot])

    def release(self, staged):
        import torch
        ev = self.free[staged.slot] = self.free[staged.slot] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream())


class LateScalar:
    """a device scalar read back one step late: an asynchronous copy into pinned memory behind the step that produced it, the value
    taken when the NEXT step has been enqueued (fit's loss: the device never waits for the host to look at a number)"""
    def __init__(self):
        import torch
        self.host = [torch.zeros(1, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        self.evt = [torch.cuda.Event(), torch.cuda.Event()]
        self.k = 0

    def post(self, dev_scalar):
        i = self.k & 1
        self.k += 1
        self.host[i].copy_(dev_scalar.reshape(-1)[:1], non_blocking=True)
        self.evt[i].record()
        return i

    def value(self, i):
        self.evt[i].synchronize()
        return float(self.host[i][0])


class DeeplabModel:
    def __init__(self, graph, head, model_type, num_classes, input_shape, training, backbone_len, seed=0, bf16=False):
        self.graph, self.head = graph, head
        self.bf16 = bool(bf16)          # mixed_precision policy at build time (train.py:37-46)
        self.name = 'deeplabv3p_' + model_type
        self.model_type, self.num_classes = model_type, num_classes
        self.input_shape_hw = tuple(input_shape)
        self.flatten_output = training      # Reshape((H*W, C)) when built for training (model.py:79-80)
        self.backbone_len = backbone_len
        # `model.layers` as Keras orders a functional model (by depth from the output, graph.keras_layer_order): what
        # layers[i].trainable (train.py:222-229, model.py:106-115), get_weights() and topological weight loading index.
        # The flat device buffers keep creation order (graph.all_params()).
        self.layers = graph.keras_layer_order(getattr(graph, 'output_layer', None))
        graph.init_weights()
        self.optimizer = None
        self.loss = None
        self.dist = None
        self.seed = seed
        self._store = None
        self._exec = {}
        self._steps = 0
        self.use_graphs = True
        self.stop_training = False

    # ---- Keras surface ------------------------------------------------------------------
    @property
    def input_shape(self):
        return (None,) + self.input_shape_hw + (3,)

    @property
    def output_shape(self):
        H, W = self.input_shape_hw
        return (None, H * W, self.num_classes) if self.flatten_output else (None, H, W, self.num_classes)

    def get_layer(self, name):
        return self.graph.layer_by_name[name]

    def count_params(self):
        return sum(p.size for p in self.graph.all_params())

    def summary(self, print_fn=print):
        print_fn('Model: "%s"' % self.name)
        print_fn('%-48s %-24s %12s' % ('Layer (type)', 'Output Shape', 'Param #'))
        print_fn('=' * 86)
        for l in self.layers:
            shape = (None,) + tuple(l.output_shape) if l.output_shape else ''
            print_fn('%-48s %-24s %12d' % ('%s (%s)' % (l.name, l.kind), str(shape), l.count_params()))
        tr = sum(p.size for p in self.graph.all_params() if p.trainable)
        tot = self.count_params()
        print_fn('=' * 86)
        print_fn('Total params: {:,}'.format(tot))
        print_fn('Trainable params: {:,}'.format(tr))
        print_fn('Non-trainable params: {:,}'.format(tot - tr))
        # which batch variance feeds the moving averages is a build-time choice that changes inference after training:
        # say so where a user looks, so weights trained here and reference-trained weights are not compared unawares
        mv = getattr(self, 'bn_moving_variance', 'biased')
        print_fn("BatchNormalization moving variance: %s batch variance (%s)" % (
            mv, 'Keras SyncBatchNormalization, what layers.py:63-70 selects for TF 2.2 .. 2.9' if mv == 'biased'
            else "fused BatchNormalization with Bessel's correction, what layers.py:63-70 selects under the pinned tensorflow==2.11.0"))

    def compile(self, optimizer=None, loss=None, metrics=None, sample_weight_mode=None, distributed=None,
                sync_bn=True, **kw):
        """model.compile(optimizer, loss, ...) (train.py:157,224): (re)binds optimiser and loss and drops the
        traced plans, so `layers[i].trainable` changes take effect like a Keras recompile"""
        # Keras keeps the slot variables and `iterations` on the optimizer OBJECT: compiling again with the same object
        # (train.py:224 after unfreezing) continues its schedule and momentum, a new object (train.py:190-224 builds one
        # for the second stage) starts its schedule at step 0 with fresh slots
        same_optimizer = optimizer is not None and optimizer is self.optimizer
        self.optimizer = optimizer or SGD(0.01)
        self.loss = loss or SparseCategoricalCrossEntropy(ignore_index=255)
        if sample_weight_mode not in (None, 'temporal'):
            raise ValueError("sample_weight_mode must be None or 'temporal' (train.py:116-120)")
        self.sample_weight_mode = sample_weight_mode
        self.metrics = metrics
        self._jaccard = _wants_jaccard(metrics)
        if distributed is None:
            import torch.distributed as dist
            distributed = dist.is_available() and dist.is_initialized() and (
                dist.get_world_size() > 1 or bool(os.environ.get('DL3P_FORCE_DIST')))
        if os.environ.get('DL3P_SYNC_BN', '1') in ('0',):
            sync_bn = False            # per-replica BatchNorm statistics (no forward collectives)
        # `distributed` may also be a DistContext (or a test double of one: tests/test_dist_gpu.py drives the executor's
        # world-size arithmetic on one GPU with a context whose sum over two identical ranks is a multiplication by 2)
        self.dist = distributed if isinstance(distributed, DistContext) else (DistContext(sync_bn) if distributed else None)
        self._exec = {}
        self._last_train_ex = None
        if self._store is not None:
            self._store.refresh_masks()
            if not same_optimizer:
                self._store.V.zero_()
                if self._store.V2 is not None:
                    self._store.V2.zero_()
                self._store.opt_step.zero_()       # (the dropout stream, store.step, keeps counting)
                # the slot of an averaged optimizer belongs to the object too: a new one takes it from the weights at its
                # first step (ParamStore.A_pending), a plain one has none
                if self._avg_spec() is None:
                    self._store.A, self._store.A_pending = None, False
                elif self._store.A is not None:
                    self._store.A_pending = True
        return self

    def _avg_spec(self):
        spec = getattr(self.optimizer, 'avg_spec', None)
        return spec() if spec is not None else None

    def _averaging_store(self, what):
        if self._avg_spec() is None:
            raise RuntimeError('%s: the compiled optimizer does not average weights' % what)
        store = self._ensure_store()
        if store.A is None:                # compiled, no executor yet: the slot is created like the first step would
            import torch
            store.A, store.A_pending = torch.zeros_like(store.P), True
        return store

    def get_average_weights(self):
        """the slot of the averaged optimizer in get_weights() order: the averages of MovingAverage / SWA, the slow weights of
        Lookahead.  Entries the optimizer does not update (frozen layers, BatchNorm moving statistics) have no slot in
        tensorflow-addons; here they hold the value the slot buffer was created with.  Before the first step of a new
        optimizer object that is the current weights."""
        store = self._averaging_store('get_average_weights')
        buf = store.P if store.A_pending else store.A
        return [store.get(p, buf) for p in self._keras_params()]

    def assign_average_vars(self):
        """tfa `optimizer.assign_average_vars(model.variables)` (MovingAverage, SWA): the weights become the averages, on
        the device, and every weight mirror is rebuilt.  Variables without a slot (frozen layers, BatchNorm moving
        statistics) keep their current value, and the slot buffer's copy of them is brought up to date with it, so that
        get_average_weights() describes the model that was just assigned."""
        store = self._averaging_store('assign_average_vars')
        if self._avg_spec()[0] == 'lookahead':
            raise RuntimeError('assign_average_vars: Lookahead keeps slow weights, not averages (tfa has no such method)')
        if store.A_pending:
            return                          # no step yet: the averages are the weights
        import torch
        merged = torch.where(store.lr_scale != 0, store.A, store.P)
        store.P.copy_(merged)
        store.A.copy_(merged)
        store.transpose()

    def _ensure_store(self):
        import torch
        if self._store is None:
            if not torch.cuda.is_available():
                raise RuntimeError('the DeepLabV3+ HIP path needs an MI355X device; there is no CPU fallback')
            from .executor import ParamStore
            self._store = ParamStore(self.graph, torch.device('cuda', torch.cuda.current_device()), bf16=self.bf16)
            if self.dist is not None:
                self.dist.broadcast(self._store.P, 0)   # identical replicas (MirroredStrategy semantics)
                self._store.transpose()
        return self._store

    def _clip_spec(self):
        spec = getattr(self.optimizer, 'clip_spec', None)
        return spec() if spec is not None else None

    @property
    def last_grad_norm(self):
        """the global L2 norm of the last training step's gradient as the norm rules saw it (the whole loss, trainable variables,
        after clipvalue, before any norm scaling); None without clipping or before the first step.  The number follows its step to
        the host asynchronously: reading it waits for that copy, the step itself never does."""
        ex = getattr(self, '_last_train_ex', None)
        return ex.last_grad_norm() if ex is not None else None

    def _executor(self, batch, training):
        avg = self._avg_spec() if training else None
        clip = self._clip_spec() if training else None
        key = (batch, training) if avg is None else (batch, training, avg)
        if clip is not None:
            key = key + (('clip',) + clip,)
        if key not in self._exec:
            from .executor import Executor
            store = self._ensure_store()
            ignore = self.loss.ignore_index if self.loss is not None else 255
            opt = self.optimizer.spec() if self.optimizer is not None else ('sgd', 0.9)
            rank = self.dist.rank if self.dist is not None else 0
            self._exec[key] = Executor(self.graph, self.head, store, batch, training, self.num_classes,
                                       ignore_index=ignore, dist=self.dist if training else None,
                                       seed=self.seed + 7919 * rank, loss=loss_spec(self.loss), optimizer=opt,
                                       sample_weighted=getattr(self, 'sample_weight_mode', None) == 'temporal',
                                       class_counts=getattr(self, '_jaccard', False), averaging=avg, clip=clip)
        return self._exec[key]

    def train_on_batch(self, x, y, sample_weight=None, return_tensor=False):
        """one optimiser step on (x (B,H,W,3) float32 in [-1,1] or uint8, y (B,H*W,1) class ids[, sample_weight (B,H*W)
        with compile(sample_weight_mode='temporal'); 'adaptive' = the generator's balanced class weights, computed on
        the device from uint8 labels]); returns the data loss"""
        if self.optimizer is None:
            raise RuntimeError('You must compile your model before training')
        staged = x if isinstance(x, StagedBatch) else None
        if staged is not None:              # (prefetch_batch: the arrays are already on their way; the compute stream waits for the DMA)
            x, y, sample_weight = staged.x, staged.y, staged.sample_weight
            self._feeder().consume(staged)
        # more than one rank: the executor trace (every collective once), the graph capture and the first replays are where
        # a multi-process job can hang -- bounded by watchdog.FirstStepsGuard (prints the switches to try, exits non-zero)
        guarded = self.dist is not None and self.dist.world_size > 1 and self._steps < 3
        from .watchdog import FirstStepsGuard
        # (an unguarded step arms nothing: world 1 / timeout 0; `with` cancels the timer on every exit path -- an exception
        # the caller catches must not leave it armed to os._exit(3) the process minutes later)
        with FirstStepsGuard(self.dist.rank if guarded else 0, self.dist.world_size if guarded else 1,
                             'train step %d' % self._steps):
            ex = self._executor(int(x.shape[0]), True)
            ex.set_inputs(x, y, sample_weight)
            if staged is not None:
                self._feeder().release(staged)
            ex.lr.fill_(self.optimizer.lr_at(self.optimizer.iterations))
            if self.use_graphs and not ex.graphed and self._steps_on(ex) >= 1:
                ex.capture()
            ex.train_step()
            self._last_train_ex = ex
            if guarded:
                import torch
                torch.cuda.synchronize()
        ex._steps = self._steps_on(ex) + 1
        self._steps += 1
        self.optimizer.iterations += 1
        if return_tensor:
            return ex.loss
        loss = float(ex.loss.item())
        self.last_metrics = {'Jaccard': jaccard_from_counts(ex.metric_counts.cpu().numpy())} if ex.metric_counts is not None else {}
        return loss

    @staticmethod
    def _steps_on(ex):
        return getattr(ex, '_steps', 0)

    def _feeder(self):
        if getattr(self, '_feed', None) is None:
            self._feed = BatchFeeder()
        return self._feed

    def prefetch_batch(self, x, y, sample_weight=None):
        """start moving a host batch to the device (pinned staging, copy stream; double-buffered: at most one batch ahead of the one
        in flight) -> a StagedBatch that train_on_batch takes in place of the arrays.  fit / fit_generator does this for every
        batch: the copy of batch k + 1 runs beside step k"""
        return self._feeder().put(x, y, sample_weight)

    def predict(self, x, verbose=0, batch_size=None):
        """probabilities (B,H*W,C) for a training-shaped model, (B,H,W,C) otherwise (eval.py:33-36)"""
        if isinstance(x, (list, tuple)):
            x = x[0]
        if not _on_device_u8(x):                # (CUDA uint8 tensors go to set_inputs as they are)
            x = np.asarray(x)
            if x.dtype != np.uint8:             # uint8 pixels are normalised on the device (Executor.set_inputs)
                x = x.astype(np.float32, copy=False)
        B = x.shape[0]
        ex = self._executor(B, False)
        ex.set_inputs(x)
        ex.forward()
        H, W = self.input_shape_hw
        p = ex.probs.view(B, H, W, self.num_classes).cpu().numpy()
        return p.reshape(B, H * W, self.num_classes) if self.flatten_output else p

    def predict_mask(self, x):
        """class ids (B,H,W) int32 = np.argmax(predict(x), -1) (eval.py:33-36, deeplab.py:97-99) taken on the device: the
        mask is 1/84 of the bytes of the 21-class probability tensor"""
        import torch
        if isinstance(x, (list, tuple)):
            x = x[0]
        if not _on_device_u8(x):                # (CUDA uint8 tensors go to set_inputs as they are)
            x = np.asarray(x)
            if x.dtype != np.uint8:
                x = x.astype(np.float32, copy=False)
        B = x.shape[0]
        ex = self._executor(B, False)
        ex.set_inputs(x)
        H, W = self.input_shape_hw
        pred = torch.empty(B * H * W, dtype=torch.int32, device='cuda')
        ex.eval_step(None, pred)
        return pred.view(B, H, W).cpu().numpy()

    def fit(self, x=None, steps_per_epoch=None, epochs=1, initial_epoch=0, verbose=1, callbacks=None,
            validation_data=None, validation_steps=None, weighted_type=None, **kw):
        """Keras-like loop over a Sequence/generator yielding (images, labels) (train.py:177-187).
        weighted_type='adaptive' (train.py --weighted_type, deeplabv3p/data.py:134-145): a generator that yields uint8
        labels and no weights gets the balanced per-image class weights computed on the device"""
        gen = x
        n = steps_per_epoch or len(gen)
        history = {'loss': []}
        for cb in callbacks or []:
            getattr(cb, 'set_model', lambda m: None)(self)
        for epoch in range(initial_epoch, epochs):
            t0, losses, metric_sums = time.time(), [], {}
            it = iter(gen) if not hasattr(gen, '__getitem__') else None
            fetch = (lambda i: gen[i]) if it is None else (lambda i: next(it))

            def stage(batch):
                # generators yield (x, y) or, in adaptive weighting mode, (x, y, sample_weight) (deeplabv3p/data.py:149-154)
                sw = batch[2] if len(batch) > 2 else None
                if isinstance(sw, dict):
                    sw = next(iter(sw.values()))          # {'pred_mask': weights}
                if sw is None and weighted_type == 'adaptive' and getattr(batch[1], 'dtype', None) == np.uint8:
                    sw = 'adaptive'
                return self.prefetch_batch(batch[0], batch[1], sw), int(np.shape(batch[0])[0])
            late = getattr(self, '_late_loss', None) or LateScalar()
            self._late_loss = late
            pending = None                                 # the loss of the step before, still on its way to the host
            staged, bsz = stage(fetch(0)) if n > 0 else (None, 0)
            for i in range(n):
                # the step is only enqueued here; while the device runs it the generator prepares the next batch (decode, augment,
                # resize on the host) and that batch crosses PCIe on the copy stream; the loss is looked at one step late
                loss_t = self.train_on_batch(staged, None, return_tensor=True)
                ex = self._executor(bsz, True)
                slot = late.post(loss_t)
                counts = ex.metric_counts.cpu().numpy() if ex.metric_counts is not None else None
                if i + 1 < n:
                    staged, bsz = stage(fetch(i + 1))
                if pending is not None:
                    losses.append(late.value(pending))
                pending = slot
                if counts is not None:
                    metric_sums.setdefault('Jaccard', []).append(jaccard_from_counts(counts))
                if losses and not np.isfinite(losses[-1]):      # TerminateOnNaN (train.py:64), one step late
                    self.stop_training = True
                    break
            if pending is not None:
                losses.append(late.value(pending))
                if not np.isfinite(losses[-1]):
                    self.stop_training = True
            logs = {'loss': float(np.mean(losses))}
            for mk, mv in metric_sums.items():             # Keras averages a metric over the epoch's batches
                logs[mk] = float(np.nanmean(mv))
            if validation_data is not None:
                logs['val_loss'] = self.evaluate(validation_data, validation_steps)
                for mk, mv in getattr(self, 'last_val_metrics', {}).items():
                    logs['val_' + mk] = mv
            history['loss'].append(logs['loss'])
            if verbose:
                print('Epoch %d/%d - %.1fs - loss: %.4f%s' % (
                    epoch + 1, epochs, time.time() - t0, logs['loss'],
                    (' - val_loss: %.4f' % logs['val_loss']) if 'val_loss' in logs else ''))
            if hasattr(gen, 'on_epoch_end'):
                gen.on_epoch_end()
            for cb in callbacks or []:
                getattr(cb, 'on_epoch_end', lambda e, l=None: None)(epoch, logs)
            if self.stop_training:
                break
        return history

    fit_generator = fit

    # ---- weights ------------------------------------------------------------------------
    def _sync_to_host(self):
        if self._store is not None:
            self._store.download()

    def _keras_params(self):
        return [p for l in self.layers for p in l.params]

    def get_weights(self):
        self._sync_to_host()
        return [p.value for p in self._keras_params()]

    def set_weights(self, weights):
        ps = self._keras_params()
        assert len(weights) == len(ps), (len(weights), len(ps))
        for p, w in zip(ps, weights):
            w = np.asarray(w, dtype=np.float32)
            assert w.shape == p.shape, (p.name, w.shape, p.shape)
            p.value = w.copy()
        if self._store is not None:
            self._store.upload()

    def get_weights_by_name(self):
        self._sync_to_host()
        return {p.name: p.value for p in self.graph.all_params()}

    def set_weights_by_name(self, d, strict=True):
        for p in self.graph.all_params():
            if p.name in d:
                w = np.asarray(d[p.name], dtype=np.float32)
                assert w.shape == p.shape, (p.name, w.shape, p.shape)
                p.value = w.copy()
            elif strict:
                raise KeyError(p.name)
        if self._store is not None:
            self._store.upload()

    def _keras_layers(self):
        """[(layer name, [(Keras weight name, array), ...]), ...] in topological order, weightless layers included"""
        self._sync_to_host()
        return [(l.name, [(p.name + ':0', p.value) for p in l.params]) for l in self.layers]

    def save(self, path):
        """whole-model checkpoint (train.py:247, deeplab.py:113).  `*.h5`: the Keras HDF5 layout (weights under
        `model_weights`, see h5io.py; `model_config` records the factory arguments -- it is not a Keras-deserialisable
        layer config, `keras.Model.load_weights` reads the file, `load_model` does not).  Anything else: `.npz` keyed
        by Keras weight name."""
        if path.endswith('.h5') or path.endswith('.hdf5'):
            import json
            from . import h5io
            cfg = json.dumps({'class_name': 'DeeplabV3p', 'config': {
                'name': self.name, 'factory': {'model_type': self.model_type, 'num_classes': self.num_classes,
                                               'model_input_shape': list(self.input_shape_hw),
                                               'output_stride': getattr(self.graph, 'output_stride', None),
                                               'training': bool(self.flatten_output),
                                               # (the moving statistics in this file were accumulated under this rule)
                                               'bn_moving_variance': getattr(self, 'bn_moving_variance', 'biased')}}})
            h5io.write_keras_h5(path, self._keras_layers(), whole_model=True, model_config=cfg)
            return
        np.savez(path if path.endswith('.npz') else path + '.npz', **self.get_weights_by_name())

    def save_weights(self, path):
        """`model.save_weights`: the same tree at the file root"""
        if path.endswith('.h5') or path.endswith('.hdf5'):
            from . import h5io
            h5io.write_keras_h5(path, self._keras_layers(), whole_model=False)
            return
        self.save(path)

    def _load_keras_h5(self, path, by_name, skip_mismatch):
        """Keras `load_weights_from_hdf5_group` (topological: the i-th layer WITH weights of the file feeds the i-th
        layer with weights of the model, names ignored) / `..._by_name` (layers matched by name, weights by position)"""
        from . import h5io
        file_layers, _ = h5io.read_keras_h5(path)
        mine = [l for l in self.layers if l.params]

        def assign(layer, ws, lname):
            if len(ws) != len(layer.params):
                if skip_mismatch:
                    return
                raise ValueError('Layer %r expects %d weight(s), but the saved layer %r holds %d'
                                 % (layer.name, len(layer.params), lname, len(ws)))
            for p, (wn, w) in zip(layer.params, ws):
                if tuple(w.shape) != p.shape:
                    if skip_mismatch:
                        continue
                    raise ValueError('Shape mismatch for %s: model %s, file %s %s' % (p.name, p.shape, wn, w.shape))
                p.value = np.ascontiguousarray(w, dtype=np.float32)

        if by_name:
            index = {n: ws for n, ws in file_layers if ws}
            for l in mine:
                if l.name in index:
                    assign(l, index[l.name], l.name)
        else:
            theirs = [(n, ws) for n, ws in file_layers if ws]
            if len(theirs) != len(mine):
                raise ValueError('You are trying to load a weight file containing %d layers into a model with %d layers.'
                                 % (len(theirs), len(mine)))
            for l, (n, ws) in zip(mine, theirs):
                assign(l, ws, n)
        if self._store is not None:
            self._store.upload()

    def load_weights(self, path, by_name=False, skip_mismatch=False):
        """model.py:102-104 `model.load_weights(weights_path, by_name=False)`; Keras `.h5` files or `.npz`"""
        if not os.path.exists(path) and os.path.exists(path + '.npz'):
            path = path + '.npz'
        with open(path, 'rb') as fh:
            magic = fh.read(8)
        if magic == b'\x89HDF\r\n\x1a\n':
            return self._load_keras_h5(path, by_name, skip_mismatch)
        data = np.load(path)
        if by_name:
            self.set_weights_by_name({k: data[k] for k in data.files}, strict=False)
        else:
            self.set_weights([data[p.name] for p in self._keras_params()])


def _on_device_u8(a):
    """a CUDA uint8 tensor: what data.SegmentationGenerator(output='device') yields"""
    import torch
    return isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.uint8


def _evaluate(self, gen, steps=None):
    """Keras `evaluate` / the validation pass of `fit`: mean of the compiled loss with inference-mode BN and no dropout,
    evaluated on the device (the probability tensor is neither written nor downloaded); fills last_val_metrics"""
    import torch
    n = steps or len(gen)
    tot, cnt, jac = 0.0, 0, []
    for i in range(n):
        first = gen[i]
        if _on_device_u8(first[0]):             # a device generator: one fetch, the CUDA uint8 tensors as they are
            x, y = first[0], first[1]
            B = x.shape[0]
            ex = self._executor(B, False)
            ex.set_inputs(x, y)
        else:                                   # (host arrays: images of one fetch, labels of a second, as ever)
            x, y = np.asarray(first[0]), np.asarray(gen[i][1])
            B = x.shape[0]
            ex = self._executor(B, False)
            ex.set_inputs(x if x.dtype == np.uint8 else x.astype(np.float32, copy=False),
                          y if y.dtype == np.uint8 else y.astype(np.float32, copy=False))
        counts = None
        if getattr(self, '_jaccard', False):
            counts = torch.zeros((B, 3, self.num_classes), dtype=torch.int32, device='cuda')
        loss = float(ex.eval_loss_step(counts).item())
        tot += loss * B
        cnt += B
        if counts is not None:
            jac.append(jaccard_from_counts(counts.cpu().numpy()))
    self.last_val_metrics = {'Jaccard': float(np.nanmean(jac))} if jac else {}
    return tot / max(cnt, 1)


DeeplabModel.evaluate = _evaluate


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


def _evaluate_miou(self, gen, steps=None, class_names=None, verbose=0):
    """eval.py:376-512 `eval_mIOU` for a generator of (images, labels) batches: inference forward, argmax and the
    confusion matrix stay on the device (Executor.eval_step); only the C x C counters come back.  -> miou_from_confusion"""
    import torch
    n = steps or len(gen)
    C = self.num_classes
    cm = torch.zeros(C * C, dtype=torch.int64, device='cuda')
    for i in range(n):
        batch = gen[i]
        if _on_device_u8(batch[0]):
            ex = self._executor(batch[0].shape[0], False)
            ex.set_inputs(batch[0], batch[1])
        else:
            x, y = np.asarray(batch[0]), np.asarray(batch[1])
            ex = self._executor(x.shape[0], False)
            ex.set_inputs(x if x.dtype == np.uint8 else x.astype(np.float32, copy=False),
                          y if y.dtype == np.uint8 else y.astype(np.float32, copy=False))
        ex.eval_step(cm)
    res = miou_from_confusion(cm.view(C, C).cpu().numpy(), class_names)
    if verbose:
        print('mIoU=%.3f' % (res['mIoU'] * 100))
        print('FWIoU=%.3f' % (res['FWIoU'] * 100))
        print('PixelAcc=%.3f' % (res['PixelAcc'] * 100))
        print('mClassAcc=%.3f' % (res['mClassAcc'] * 100))
    return res


DeeplabModel.evaluate_miou = _evaluate_miou


# ---- multi-scale / mirrored evaluation ----------------------------------------------------------------------------------
# DeepLab's evaluation protocol (the published mIoU figures): the image at several scales, each also mirrored, the class
# probabilities of all passes averaged at the base resolution before the argmax.  The reference repository evaluates one scale,
# unmirrored; the semantics below are this project's.  Per scale one dl3p_tta_accumulate launch adds the plain
# and the mirrored pass into one running sum; the last launch writes no sum and leaves the mask / the confusion counters.
def tta_size(n, s):
    """DeepLab's crop-size rule for a side of n pixels at scale s: int((n - 1) * s + 1.0) in float64 (513 -> 257, 385, 641, 769, 897
    for 0.5 .. 1.75; s = 1 gives n)"""
    return int((int(n) - 1) * float(s) + 1.0)


def _default_tta(scales, flip):
    try:
        return not flip and tuple(float(s) for s in scales) == (1.0,)
    except TypeError:
        return False


def _tta_check(self, scales):
    """ValueError for what the multi-scale evaluation does not serve -> the scales as a tuple of floats"""
    if getattr(self, '_factory', None) is None:
        raise ValueError("multi-scale / mirrored evaluation is built for get_deeplabv3p_model models only, not for '%s' from "
                         "get_unet_model / get_fast_scnn_model" % (self.model_type,))
    scales = tuple(float(s) for s in scales)
    if not scales:
        raise ValueError('scales must name at least one scale (got an empty sequence)')
    for s in scales:
        if not s > 0:
            raise ValueError('scales must be positive (got %r)' % (s,))
    return scales


def _tta_siblings(self, scales):
    """one inference model per scale, in the order given: this model for a scale that keeps its input shape, otherwise a sibling from
    the same factory with this model's arguments at (tta_size(H, s), tta_size(W, s)).  Siblings are cached per shape and built only
    when absent; every call refreshes their weights from this model's parameter store"""
    import contextlib
    import io
    from . import mixed_precision
    scales = _tta_check(self, scales)
    H, W = self.input_shape_hw
    cache = self.__dict__.setdefault('_tta_cache', {})
    out = []
    for s in scales:
        shape = (tta_size(H, s), tta_size(W, s))
        if shape == (H, W):
            out.append(self)
            continue
        if shape not in cache:
            if min(shape) < 1:
                raise ValueError('scale %r gives the input shape %r' % (s, shape))
            f = self._factory
            policy = mixed_precision._GLOBAL
            mixed_precision._GLOBAL = 'mixed_bfloat16' if self.bf16 else 'float32'      # the policy this model was built under
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    cache[shape] = get_deeplabv3p_model(f['model_type'], self.num_classes, shape, f['output_stride'], freeze_level=0,
                                                        weights_path=None, training=False, seed=self.seed,
                                                        bn_moving_variance=f['bn_moving_variance'])
            except ValueError as e:
                raise ValueError("scale %r: model type '%s' cannot be built at input shape %r: %s" % (s, self.model_type, shape, e))
            finally:
                mixed_precision._GLOBAL = policy
        out.append(cache[shape])
    store = self._ensure_store()
    for sib in {id(m): m for m in out if m is not self}.values():
        st = sib._ensure_store()
        same = st.total == store.total and len(st.params) == len(store.params) and all(
            a.dev_shape == b.dev_shape and st.offset[a] == store.offset[b] for a, b in zip(st.params, store.params))
        assert same, 'a sibling at another input shape has the same parameters in the same layout'
        if same:
            st.P.copy_(store.P)             # device to device
            st.transpose()
        else:
            sib.set_weights(self.get_weights())
    return out


def _tta_frames(self, frames_u8, check_only=False):
    """uint8 frames (B,H,W,3) at the model's input shape, host or device -> a dense CUDA uint8 tensor"""
    import torch
    dt = getattr(frames_u8, 'dtype', None)
    if dt not in (np.uint8, torch.uint8):
        raise ValueError('multi-scale / mirrored evaluation takes uint8 frames (they are resized as bytes, like Pillow does); '
                         'got dtype %r' % (dt,))
    H, W = self.input_shape_hw
    if tuple(frames_u8.shape[1:]) != (H, W, 3):
        raise ValueError('the model takes (B, %d, %d, 3) frames, got %r' % (H, W, tuple(frames_u8.shape)))
    if check_only:
        return None
    if not isinstance(frames_u8, torch.Tensor):
        frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8))
    return frames_u8.cuda(non_blocking=True).contiguous()


def _tta_run(self, frames_u8, scales, flip, labels=None, confusion=None, want_mask=False, want_sum=False):
    """the passes of one batch -> (sum (B,H,W,Cpad) or None, mask (B,H,W) int32 or None); labels / confusion: the base executor's
    label plane and a (C,C) int64 counter tensor that the last launch adds to"""
    import torch
    from . import augment, ops
    from ._lib import lib
    scales = _tta_check(self, scales)
    _tta_frames(self, frames_u8, check_only=True)       # (every refusal comes before the first device call)
    models = _tta_siblings(self, scales)
    frames = _tta_frames(self, frames_u8)
    B = int(frames.shape[0])
    H, W = self.input_shape_hw
    C = self.num_classes
    weight = 1.0 / (len(scales) * (2 if flip else 1))
    ones = torch.ones(B, dtype=torch.int32, device=frames.device) if flip else None      # flags: bit 0 = mirror along x
    acc = pred = None
    for i, m in enumerate(models):
        hs, ws = m.input_shape_hw
        x = frames if m is self else augment.pil_resize(frames, (hs, ws))
        ex = m._executor(B, False)
        ex.set_inputs(x)
        z, zm = ex.eval_logits(), None
        if flip:
            z = z.clone()                       # (the mirrored pass reuses the executor's buffer)
            xm = torch.empty_like(x)
            lib().aug_flip_crop_u8(x.data_ptr(), xm.data_ptr(), None, None, ones.data_ptr(), None, B, hs, ws, hs, ws,
                                   torch.cuda.current_stream().cuda_stream)
            ex.set_inputs(xm)
            zm = ex.eval_logits()
        last = i == len(models) - 1
        acc, p, _ = ops.tta_accumulate(z, zm, C, H, W, weight, acc=acc, write=(not last) or want_sum,
                                       labels=labels if last else None, confusion=confusion if last else None,
                                       want_mask=want_mask and last)
        pred = p if last else pred
    return acc, pred


def _predict_tta(self, frames_u8, scales=(1.0,), flip=False):
    """mean class probabilities over the passes of DeepLab's multi-scale / mirrored protocol: frames_u8 (B,H,W,3) uint8 at the model's
    input shape, on the host or the device -> (B,H,W,C) float32, (B,H*W,C) for a training-shaped model"""
    acc, _ = _tta_run(self, frames_u8, scales, flip, want_sum=True)
    H, W = self.input_shape_hw
    p = acc[..., :self.num_classes].cpu().numpy()
    return p.reshape(p.shape[0], H * W, self.num_classes) if self.flatten_output else p


def _evaluate_miou_tta(self, gen, steps=None, class_names=None, verbose=0, *, scales=(1.0,), flip=False):
    """_evaluate_miou, and with other `scales` / `flip` than the defaults DeepLab's multi-scale / mirrored protocol (not the reference
    repository's: eval.py evaluates one scale): per batch every pass's logits are added as probabilities into one running sum on the
    device and the last launch counts against the labels; only the C x C counters come back.  The generator then yields uint8 images"""
    if _default_tta(scales, flip):
        return _evaluate_miou(self, gen, steps, class_names, verbose)
    import torch
    scales = _tta_check(self, scales)
    n = steps or len(gen)
    C = self.num_classes
    cm = None
    for i in range(n):
        batch = gen[i]
        x, y = batch[0], batch[1]
        if not _on_device_u8(x):
            x = np.asarray(x)
        _tta_frames(self, x, check_only=True)
        if cm is None:
            cm = torch.zeros((C, C), dtype=torch.int64, device='cuda')
        frames = _tta_frames(self, x)
        if not _on_device_u8(y):
            y = np.asarray(y)
            y = y if y.dtype == np.uint8 else y.astype(np.float32, copy=False)
        base = self._executor(int(frames.shape[0]), False)
        base.set_inputs(frames, y)          # the labels of this batch, where the last launch reads them
        _tta_run(self, frames, scales, flip, labels=base.labels, confusion=cm)
    res = miou_from_confusion(cm.cpu().numpy() if cm is not None else np.zeros((C, C), np.int64), class_names)
    if verbose:
        print('mIoU=%.3f' % (res['mIoU'] * 100))
        print('FWIoU=%.3f' % (res['FWIoU'] * 100))
        print('PixelAcc=%.3f' % (res['PixelAcc'] * 100))
        print('mClassAcc=%.3f' % (res['mClassAcc'] * 100))
    return res


DeeplabModel._tta_siblings = _tta_siblings
DeeplabModel.predict_tta = _predict_tta
DeeplabModel.evaluate_miou = _evaluate_miou_tta


# model types whose graphs contain ops without a bf16 kernel on the TRAINING path are rejected when the model is built, not at
# the first train step.  Empty since round 3: the data gradient of a dense k x k conv (dl3p_col2im_bf16 behind the
# GEMM) and max pooling (dl3p_maxpool2d_*_bf16) closed the gap for Xception and ResNet50 -- train.py:37-46 applies the policy to
# every model type.  The U-Net types (get_unet_model) are refused under the policy whether built for training or not: the 2x2
# stride-2 transposed conv (csrc/deconv.hip) has no bf16 twin yet.
_NO_BF16_TRAINING = {'unet_standard': 'dl3p_deconv2x2_* has no bf16 kernels', 'unet_lite': 'dl3p_deconv2x2_* has no bf16 kernels',
                     'fast_scnn': 'the nearest-upsampling and window-pooling kernels have no bf16 twins'}


def get_deeplabv3p_model(model_type, num_classes, model_input_shape, output_stride, freeze_level=0,
                         weights_path=None, training=True, use_subpixel=False, seed=0, bn_moving_variance='biased'):
    """deeplabv3p/model.py:51-117, same positional / keyword arguments.  Two extras, keyword-only in spirit:
    `seed` (weight initialisation) and `bn_moving_variance`, which of the two Keras classes CustomBatchNormalization
    (layers.py:63-70) can resolve to is restated for the MOVING variance: 'biased' = SyncBatchNormalization, Keras' non-fused
    path (TF 2.2 .. 2.9, and what north_star asks for: SyncBN over the global batch); 'unbiased' = plain fused
    BatchNormalization with Bessel's correction, which is what the string compare at layers.py:64 selects under the pinned
    tensorflow==2.11.0.  Training-mode outputs, losses and gradients do not depend on it; inference after
    training does (factor count / (count - 1) in the variance each step contributes)."""
    if bn_moving_variance not in ('biased', 'unbiased'):
        raise ValueError("bn_moving_variance must be 'biased' or 'unbiased' (got %r)" % (bn_moving_variance,))
    from . import graph as graph_mod, mixed_precision
    bf16 = mixed_precision.is_bf16()        # the global policy at build time, like Keras layers pick theirs up
    graph_mod.CHANNEL_ALIGN = 8 if bf16 else 4
    try:
        model = _build_model(model_type, num_classes, model_input_shape, output_stride, freeze_level, weights_path, training,
                             use_subpixel, seed, bf16)
        model.graph.bn_moving_variance = model.bn_moving_variance = bn_moving_variance
        # what _tta_siblings hands the factory again for the same model at another input shape
        model._factory = {'model_type': model_type, 'output_stride': output_stride, 'bn_moving_variance': bn_moving_variance}
        return model
    finally:
        graph_mod.CHANNEL_ALIGN = 4


def _build_model(model_type, num_classes, model_input_shape, output_stride, freeze_level, weights_path, training,
                 use_subpixel, seed, bf16):
    # check if model type is valid
    if model_type not in deeplab_model_map.keys():
        raise ValueError('This model type is not supported now')
    if use_subpixel:
        raise ValueError('Subpixel head is experimental in the reference (README TODO) and not on the hot path')
    if not 1 <= int(num_classes) <= 253:
        # PNG label maps hold fewer than 254 classes (train.py:34); up to 32 classes a pixel's class vector stays in
        # registers in the head kernels, beyond that they walk the classes (dl3p_upsample_softmax_loss)
        raise ValueError('num_classes must be in [1, 253] (got %r)' % (num_classes,))

    model_function = deeplab_model_map[model_type]
    H, W = model_input_shape
    if bf16 and training and model_type in _NO_BF16_TRAINING:
        # the policy of train.py:37-46 applies to every model type there; here the mixed-precision kernels cover the
        # MobileNet families (BASELINE configs[4]).  Say so when the model is built, not at the first train step.
        raise ValueError("mixed_bfloat16 training is not built for model type '%s' (%s); build it under the float32 policy"
                         % (model_type, _NO_BF16_TRAINING[model_type]))
    # the reference builds a 21-class stub head and cuts it off again at layers[-5] (model.py:59-65);
    # the builders here stop at that tensor.  weights=None: offline, random init.
    g, x, backbone_len = model_function(input_shape=(H, W, 3), weights=None, num_classes=21, OS=output_stride,
                                        seed=seed)
    print('backbone layers number: {}'.format(backbone_len))
    base_len = len(g.layers)           # every layer but the new head (= len(base_model.layers), model.py:108)

    # new head (model.py:75-86): conv_upsample 1x1 (+bias) -> pred_resize -> [Reshape] -> Softmax('pred_mask').
    # The class dimension is padded to a multiple of 4 on the device (pad weights/bias stay exactly 0).
    cpad = (num_classes + g.align - 1) // g.align * g.align
    x = g.conv2d(x, num_classes, 1, 'conv_upsample', use_bias=True, pad_to=cpad)
    out = g.passthrough(x, 'Lambda', (H, W, num_classes), name='pred_resize')
    if training:
        out = g.passthrough(out, 'Reshape', (H * W, num_classes))
    out = g.passthrough(out, 'Softmax', (H * W, num_classes) if training else (H, W, num_classes), name='pred_mask')
    g.output_layer = out.klayer
    if x.tensor.C != cpad or not x.is_plain:
        raise AssertionError('head tensor layout')

    model = DeeplabModel(g, x, model_type, num_classes, (H, W), training, backbone_len, seed=seed, bf16=bf16)

    if weights_path:
        model.load_weights(weights_path, by_name=False)
        print('Load weights {}.'.format(weights_path))

    if freeze_level in [1, 2]:
        # Freeze the backbone part or freeze all but final feature map & input layers.
        num = (backbone_len, base_len)[freeze_level - 1]
        for i in range(num):
            model.layers[i].trainable = False
        print('Freeze the first {} layers of total {} layers.'.format(num, len(model.layers)))
    elif freeze_level == 0:
        # Unfreeze all layers.
        for i in range(len(model.layers)):
            model.layers[i].trainable = True
        print('Unfreeze all of the layers.')
    return model


def get_unet_model(model_type, num_classes, model_input_shape, freeze_level=0, weights_path=None, training=True, seed=0):
    """unet/model.py:21-61, same positional arguments (+ `seed`, weight initialisation): 'unet_standard' | 'unet_lite' with the
    reference's head -- the final Conv2D(num_classes, 1) logits are already at full resolution -- [Reshape] -> Softmax('pred_mask').
    freeze_level is accepted and ignored like there (its code is commented out, :50-59): every layer is trainable.  The
    returned model is a DeeplabModel: compile / fit / predict / evaluate_miou / save / load_weights as for the DeepLab types."""
    from . import mixed_precision, unet as unet_mod
    if model_type not in unet_mod.unet_model_map.keys():
        raise ValueError('This model type is not supported now')
    if model_type == 'unet_simple':
        raise ValueError('unet_simple is not built: it needs ' + ', '.join(unet_mod.UNET_SIMPLE_MISSING))
    if not 1 <= int(num_classes) <= 253:
        raise ValueError('num_classes must be in [1, 253] (got %r)' % (num_classes,))
    H, W = model_input_shape
    if H % 16 or W % 16:
        # four 2x2 poolings and four 2x upsamplings: Keras fails at the first `concatenate` otherwise
        raise ValueError('U-Net input height and width must be multiples of 16 (got %r)' % ((H, W),))
    if mixed_precision.is_bf16() and model_type in _NO_BF16_TRAINING:
        raise ValueError("model type '%s' is not built for the mixed_bfloat16 policy (%s); build it under the float32 policy"
                         % (model_type, _NO_BF16_TRAINING[model_type]))
    g, x = unet_mod.unet_model_map[model_type](num_classes, input_shape=(H, W, 3), weights=None, seed=seed)
    base_len = len(g.layers)
    # the classifier: a plain Conv2D(num_classes, 1, padding='same') -- glorot_uniform, zero bias, no regulariser -- reading the
    # 2 logical channels of the padded bottleneck; its class dimension is padded to a multiple of 4 like conv_upsample's
    cpad = (num_classes + g.align - 1) // g.align * g.align
    x = g.conv2d(x, num_classes, 1, None, use_bias=True, pad_to=cpad, l2=0.0)
    out = x
    if training:
        out = g.passthrough(out, 'Reshape', (H * W, num_classes))
    out = g.passthrough(out, 'Softmax', (H * W, num_classes) if training else (H, W, num_classes), name='pred_mask')
    g.output_layer = out.klayer
    if x.tensor.C != cpad or not x.is_plain or (x.tensor.H, x.tensor.W) != (H, W):
        raise AssertionError('head tensor layout')
    model = DeeplabModel(g, x, model_type, num_classes, (H, W), training, base_len, seed=seed, bf16=False)
    model.name = model_type
    if weights_path:
        model.load_weights(weights_path, by_name=False)
        print('Load weights {}.'.format(weights_path))
    return model


def get_fast_scnn_model(model_type, num_classes, model_input_shape, weights_path=None, training=True, seed=0,
                        bn_moving_variance='biased'):
    """fast_scnn/model.py:19-45, same positional arguments (+ `seed` and `bn_moving_variance`, as get_deeplabv3p_model has them):
    'fast_scnn' with the reference's own head -- Dropout(0.3) -> UpSampling2D((8, 8)) -> [Reshape] -> Softmax('pred_mask') -- served
    by the nearest head kernels from the logits at H/8.  The returned model is a DeeplabModel like every other family's."""
    from . import mixed_precision, fast_scnn as fs_mod
    if model_type not in fs_mod.fast_scnn_model_map.keys():
        raise ValueError('This model type is not supported now')
    if not 1 <= int(num_classes) <= 253:
        raise ValueError('num_classes must be in [1, 253] (got %r)' % (num_classes,))
    if bn_moving_variance not in ('biased', 'unbiased'):
        raise ValueError("bn_moving_variance must be 'biased' or 'unbiased' (got %r)" % (bn_moving_variance,))
    H, W = model_input_shape
    if H % 32 or W % 32 or H < 256 or W < 256:
        # five stride-2 stages, then pool_size = ((H / 32) // 8, (W / 32) // 8) in the pyramid pooling block: 0 below 256, and Keras
        # cannot build AveragePooling2D(pool_size=0)
        raise ValueError('Fast-SCNN input height and width must be multiples of 32 and at least 256: the pyramid pooling block '
                         'pools with pool_size = (H/32)//8, which Keras cannot build for smaller inputs (got %r)' % ((H, W),))
    if mixed_precision.is_bf16() and model_type in _NO_BF16_TRAINING:
        raise ValueError("model type '%s' is not built for the mixed_bfloat16 policy (%s); build it under the float32 policy"
                         % (model_type, _NO_BF16_TRAINING[model_type]))
    g, x = fs_mod.fast_scnn_model_map[model_type](num_classes, input_shape=(H, W, 3), weights=None, training=training, seed=seed)
    base_len = len(g.layers)
    out = g.passthrough(x, 'UpSampling2D', (H, W, num_classes), name='up_sampling2d_1')
    if training:
        out = g.passthrough(out, 'Reshape', (H * W, num_classes), name='reshape')
    out = g.passthrough(out, 'Softmax', (H * W, num_classes) if training else (H, W, num_classes), name='pred_mask')
    g.output_layer = out.klayer
    cpad = (num_classes + g.align - 1) // g.align * g.align
    if x.tensor.C != cpad or not x.is_plain or (x.tensor.H * 8, x.tensor.W * 8) != (H, W):
        raise AssertionError('head tensor layout')
    model = DeeplabModel(g, x, model_type, num_classes, (H, W), training, base_len, seed=seed, bf16=False)
    model.name = 'Fast_SCNN'
    model.graph.bn_moving_variance = model.bn_moving_variance = bn_moving_variance
    if weights_path:
        model.load_weights(weights_path, by_name=False)
        print('Load weights {}.'.format(weights_path))
    return model


class EvalCallBack:
    """common/callbacks.py:33-53: every `eval_epoch_interval` epochs run the mIOU evaluation and, with
    save_eval_checkpoint, keep the best model under the reference's file name pattern.  The reference re-reads the
    dataset from disk inside eval_mIOU; here the evaluation batches come from `eval_generator` (images, labels) and the
    argmax + confusion matrix stay on the device (DeeplabModel.evaluate_miou)."""

    def __init__(self, eval_generator, class_names=None, log_dir='.', eval_epoch_interval=10, save_eval_checkpoint=False,
                 steps=None):
        self.eval_generator, self.class_names, self.log_dir = eval_generator, class_names, log_dir
        self.eval_epoch_interval, self.save_eval_checkpoint, self.steps = eval_epoch_interval, save_eval_checkpoint, steps
        self.best_mIOU = 0.0
        self.history = []
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.eval_epoch_interval:
            return
        logs = logs or {}
        mIOU = float(self.model.evaluate_miou(self.eval_generator, class_names=self.class_names, steps=self.steps)['mIoU'])
        self.history.append((epoch + 1, mIOU))
        if self.save_eval_checkpoint and mIOU > self.best_mIOU:
            self.best_mIOU = mIOU
            nan = float('nan')
            name = 'ep{epoch:03d}-loss{loss:.3f}-Jaccard{Jaccard:.3f}-val_loss{val_loss:.3f}-val_Jaccard{val_Jaccard:.3f}-mIOU{mIOU:.3f}.h5'
            self.model.save(os.path.join(self.log_dir, name.format(
                epoch=epoch + 1, loss=logs.get('loss', nan), Jaccard=logs.get('Jaccard', nan),
                val_loss=logs.get('val_loss', nan), val_Jaccard=logs.get('val_Jaccard', nan), mIOU=mIOU)))


class AverageModelCheckpoint:
    """tfa.callbacks.AverageModelCheckpoint (train.py:198-211) for `fit`, in tfa's order: every `period` epochs the averages
    are assigned to the weights FIRST (update_weights=False keeps a device copy of the weights to put back afterwards),
    then Keras' ModelCheckpoint logic runs on them -- the best-only test on `monitor`, `model.save` / `save_weights` under
    `filepath` formatted with epoch + 1 and the logs.  With update_weights=True the weights are therefore replaced by
    the averages at every such epoch end, whether or not a file is written.  Optimizer slots are not part of the file."""

    def __init__(self, filepath, update_weights, monitor='val_loss', mode='min', verbose=0, save_weights_only=False,
                 save_best_only=False, period=1):
        if mode not in ('auto', 'min', 'max'):
            raise ValueError("mode must be 'auto', 'min' or 'max'")
        self.filepath, self.update_weights, self.monitor, self.verbose = filepath, update_weights, monitor, verbose
        self.save_weights_only, self.save_best_only, self.period = save_weights_only, save_best_only, period
        if mode == 'auto':
            mode = 'max' if ('acc' in monitor or monitor.startswith('fmeasure')) else 'min'
        self.better = (lambda a, b: a > b) if mode == 'max' else (lambda a, b: a < b)
        self.best = -np.inf if mode == 'max' else np.inf
        self.epochs_since_last_save = 0
        self.saved = []
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        self.epochs_since_last_save += 1
        if self.epochs_since_last_save < self.period:
            return
        self.epochs_since_last_save = 0
        store = self.model._averaging_store('AverageModelCheckpoint')
        keep = None if self.update_weights else store.P.clone()
        self.model.assign_average_vars()
        try:
            self._save_model(epoch, logs or {})
        finally:
            if keep is not None:
                store.P.copy_(keep)
                store.transpose()

    def _save_model(self, epoch, logs):
        path = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            current = logs.get(self.monitor)
            if current is None:
                print('Can save best model only with %s available, skipping.' % self.monitor)
                return
            if not self.better(current, self.best):
                if self.verbose:
                    print('Epoch %05d: %s did not improve from %0.5f' % (epoch + 1, self.monitor, self.best))
                return
            if self.verbose:
                print('Epoch %05d: %s improved from %0.5f to %0.5f, saving model to %s'
                      % (epoch + 1, self.monitor, self.best, current, path))
            self.best = current
        elif self.verbose:
            print('Epoch %05d: saving model to %s' % (epoch + 1, path))
        (self.model.save_weights if self.save_weights_only else self.model.save)(path)
        self.saved.append(path)
