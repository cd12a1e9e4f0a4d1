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
from .optimizers import (_clip_args, SGD, Adam, RMSprop, _AveragedOptimizer, MovingAverage, SWA, Lookahead,  # noqa: F401
                         get_averaged_optimizer, get_optimizer)
from .losses import (SparseCategoricalCrossEntropy, WeightedSparseCategoricalCrossEntropy, SparseSoftmaxFocalLoss, Jaccard,  # noqa: F401
                     SparseTverskyLoss, SparseDiceLoss, SparseJaccardLoss, REGION_NEAREST_TEXT, jaccard_from_counts, _wants_jaccard, loss_spec, mining_spec, miou_from_confusion)
from .feed import DistContext, StagedBatch, BatchFeeder, LateScalar  # noqa: F401
from .callbacks import EvalCallBack, AverageModelCheckpoint  # noqa: F401

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


def _on_device_u8(a):
    """a CUDA uint8 tensor: what data.SegmentationGenerator(output='device') yields"""
    import torch
    return isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.uint8


def batch_input(a):
    """a batch of images or labels as Executor.set_inputs takes it, the one rule of predict, evaluate and the inference front end: a
    CUDA uint8 tensor as it is; anything else as a NumPy array, uint8 kept (pixels are normalised and labels prepared on the
    device), every other dtype as float32 -- the array itself where it already is float32"""
    if _on_device_u8(a):
        return a
    a = np.asarray(a)
    return a if a.dtype == np.uint8 else a.astype(np.float32, copy=False)


def tta_size(n, s):
    """DeepLab's crop-size rule for a side of n pixels at scale s: int((n - 1) * s + 1.0) in float64 (513 -> 257, 385, 641, 769, 897
    for 0.5 .. 1.75; s = 1 gives n)"""
    return int((int(n) - 1) * float(s) + 1.0)


def single_pass(scales, flip):
    """the defaults of the multi-scale keywords: one unmirrored pass at the model's own size, which every family serves"""
    try:
        return not flip and tuple(float(s) for s in scales) == (1.0,)
    except TypeError:
        return False


def _print_miou(res):
    print('mIoU=%.3f' % (res['mIoU'] * 100))
    print('FWIoU=%.3f' % (res['FWIoU'] * 100))
    print('PixelAcc=%.3f' % (res['PixelAcc'] * 100))
    print('mClassAcc=%.3f' % (res['mClassAcc'] * 100))


class DeeplabModel:
    def __init__(self, graph, head, model_type, num_classes, input_shape, training, backbone_len, seed=0, bf16=False, family='deeplabv3p',
                 name=None, output_stride=None, bn_moving_variance='biased'):
        self.graph, self.head = graph, head
        self.bf16 = bool(bf16)          # mixed_precision policy at build time (train.py:37-46)
        self.name = name or 'deeplabv3p_' + model_type
        # how the model was built, beyond its own attributes: what save() records and _tta_siblings hands the factory again
        self.factory = {'family': family, 'model_type': model_type, 'output_stride': output_stride,
                        'bn_moving_variance': bn_moving_variance}
        # which batch variance feeds the moving averages; the executor reads it from the graph
        graph.bn_moving_variance = self.bn_moving_variance = bn_moving_variance
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
        # what compile() binds ...
        self.metrics, self._jaccard, self.sample_weight_mode = None, False, None
        # ... and what training, evaluation and the multi-scale passes leave behind
        self._feed, self._late_loss, self._last_train_ex = None, None, None
        self.last_metrics, self.last_val_metrics = {}, {}
        self._tta_cache = {}            # input shape -> sibling model (_tta_siblings)

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
        mv = self.bn_moving_variance
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
        if isinstance(loss, SparseTverskyLoss) and getattr(self.graph, 'head_upsample', 'bilinear') == 'nearest':
            raise ValueError(REGION_NEAREST_TEXT)
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
        ex = self._last_train_ex
        return ex.last_grad_norm() if ex is not None else None

    @property
    def last_mining(self):
        """what hard-example mining selected in the last training step: {'k': size of the kept set the rule asked for, 'threshold':
        the k-th largest per-pixel loss, 'kept': pixels at or above it (ties included), 'nonzero': of those, the ones whose loss is
        not 0 (the loss' normaliser)}; None without mining (top_k_percent_pixels == 1.0) or before the first step.  Like
        last_grad_norm the record follows its step to the host asynchronously: reading it waits for that copy only."""
        ex = self._last_train_ex
        return ex.last_mining() if ex is not None else None

    @property
    def last_region(self):
        """the region term of the last training step: {'loss': region_weight * R, 'present': the number of classes present in the
        batch's labels, 'score': the soft overlap T_c per class, NaN for a class that is not present}; None while no region loss
        (SparseTverskyLoss, SparseDiceLoss, SparseJaccardLoss) is compiled or before the first step.  Follows its step to the host
        asynchronously, like last_mining."""
        ex = self._last_train_ex
        return ex.last_region() if ex is not None else None

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
            spec, region = loss_spec(self.loss), None
            if spec[0] == 'region':      # the executor takes the base's spec as its per-pixel loss, and the region parameters beside it
                region, spec = spec[1:6] + (spec[6] is not None,), (spec[6] or ('ce',))
            self._exec[key] = Executor(self.graph, self.head, store, batch, training, self.num_classes,
                                       ignore_index=ignore, dist=self.dist if training else None,
                                       seed=self.seed + 7919 * rank, loss=spec, optimizer=opt,
                                       sample_weighted=self.sample_weight_mode == 'temporal',
                                       class_counts=self._jaccard, averaging=avg, clip=clip, mining=mining_spec(self.loss),
                                       region=region)
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
            if self.use_graphs and not ex.graphed and ex.steps_run >= 1:       # (the second step of each executor)
                ex.capture()
            ex.train_step()
            self._last_train_ex = ex
            if guarded:
                import torch
                torch.cuda.synchronize()
        ex.steps_run += 1
        self._steps += 1
        self.optimizer.iterations += 1
        if return_tensor:
            return ex.loss
        loss = float(ex.loss.item())
        self.last_metrics = {'Jaccard': jaccard_from_counts(ex.metric_counts.cpu().numpy())} if ex.metric_counts is not None else {}
        return loss

    def _feeder(self):
        if self._feed is None:
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
        x = batch_input(x)
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
        if isinstance(x, (list, tuple)):
            x = x[0]
        return self.class_ids(x).cpu().numpy()

    def class_ids(self, x, scales=(1.0,), flip=False):
        """predict_mask left on the device: x (B,H,W,3) at the model's input shape -> (B,H,W) int32 CUDA tensor.  Other `scales` /
        `flip` than the defaults: the mask of the multi-scale / mirrored passes (predict_tta's argmax); x is uint8 frames then"""
        import torch
        if not single_pass(scales, flip):       # the mask of the last dl3p_tta_accumulate launch
            return self._tta_run(x, scales, flip, want_mask=True)[1]
        x = batch_input(x)
        B = int(x.shape[0])
        ex = self._executor(B, False)
        ex.set_inputs(x)
        H, W = self.input_shape_hw
        pred = torch.empty(B * H * W, dtype=torch.int32, device='cuda')
        ex.eval_step(None, pred)
        return pred.view(B, H, W)

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
            late = self._late_loss = self._late_loss or LateScalar()
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
                for mk, mv in self.last_val_metrics.items():
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
                'name': self.name, 'factory': {'model_type': self.factory['model_type'], 'num_classes': self.num_classes,
                                               'model_input_shape': list(self.input_shape_hw),
                                               # (always null: no graph ever carried the stride this entry was read from, and the
                                               # file's bytes stay what they were; self.factory holds it)
                                               'output_stride': None,
                                               'training': bool(self.flatten_output),
                                               # (the moving statistics in this file were accumulated under this rule)
                                               'bn_moving_variance': self.factory['bn_moving_variance']}}})
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

    # ---- evaluation ---------------------------------------------------------------------
    def _eval_batches(self, gen, steps, images=batch_input):
        """walks `steps` batches of a Sequence of (images, labels), each fetched ONCE -> (the inference executor of the batch's size with
        images and labels set, the images as `images` made them) per batch"""
        for i in range(steps or len(gen)):
            batch = gen[i]
            x = images(batch[0])
            ex = self._executor(int(x.shape[0]), False)
            ex.set_inputs(x, batch_input(batch[1]))
            yield ex, x

    def evaluate(self, gen, steps=None):
        """Keras `evaluate` / the validation pass of `fit`: mean of the compiled loss with inference-mode BN and no dropout,
        evaluated on the device (the probability tensor is neither written nor downloaded); fills last_val_metrics"""
        import torch
        tot, cnt, jac = 0.0, 0, []
        for ex, x in self._eval_batches(gen, steps):
            B = int(x.shape[0])
            counts = None
            if self._jaccard:
                counts = torch.zeros((B, 3, self.num_classes), dtype=torch.int32, device='cuda')
            loss = float(ex.eval_loss_step(counts).item())
            tot += loss * B
            cnt += B
            if counts is not None:
                jac.append(jaccard_from_counts(counts.cpu().numpy()))
        self.last_val_metrics = {'Jaccard': float(np.nanmean(jac))} if jac else {}
        return tot / max(cnt, 1)

    def evaluate_miou(self, gen, steps=None, class_names=None, verbose=0, *, scales=(1.0,), flip=False, dense_crf=False):
        """eval.py:376-512 `eval_mIOU` for a generator of (images, labels) batches: inference forward, argmax and the
        confusion matrix stay on the device (Executor.eval_step); only the C x C counters come back.  -> miou_from_confusion.
        With other `scales` / `flip` than the defaults DeepLab's multi-scale / mirrored protocol (not the reference repository's: eval.py
        evaluates one scale): per batch every pass's logits are added as probabilities into one running sum on the device and the last
        launch counts against the labels.  The generator then yields uint8 images.
        dense_crf (True, or a dict of ops.dense_crf's keyword arguments; eval.py --do_crf with exact filters): each batch's class ids,
        of the single pass or of the multi-scale passes, are refined by the dense CRF on the device with the batch's own images, which
        the generator yields as uint8, and the refined masks are counted against the labels"""
        import torch
        from . import ops
        C = self.num_classes
        crf = ops.crf_params(dense_crf, C)
        if crf is not None:
            single = single_pass(scales, flip)
            if not single:
                scales = self.tta_scales(scales)
            H, W = self.input_shape_hw
            cm = None
            for base, frames in self._eval_batches(gen, steps, images=self._tta_frames):
                if cm is None:
                    cm = torch.zeros((C, C), dtype=torch.int64, device='cuda')
                if single:
                    pred = torch.empty((int(frames.shape[0]), H, W), dtype=torch.int32, device='cuda')
                    base.eval_step(None, pred)
                else:
                    pred = self._tta_run(frames, scales, flip, want_mask=True)[1]
                ops.mask_confusion(ops.dense_crf(frames, pred, C, **crf), base.labels, C, cm)
        elif single_pass(scales, flip):
            cm = torch.zeros(C * C, dtype=torch.int64, device='cuda')
            for ex, _ in self._eval_batches(gen, steps):
                ex.eval_step(cm)
            cm = cm.view(C, C)
        else:
            scales = self.tta_scales(scales)
            cm = None                           # (made behind the first batch's checks: every refusal comes before the first device call)
            for base, frames in self._eval_batches(gen, steps, images=self._tta_frames):
                if cm is None:
                    cm = torch.zeros((C, C), dtype=torch.int64, device='cuda')
                # the labels of this batch are where the last launch reads them
                self._tta_run(frames, scales, flip, labels=base.labels, confusion=cm)
        res = miou_from_confusion(cm.cpu().numpy() if cm is not None else np.zeros((C, C), np.int64), class_names)
        if verbose:
            _print_miou(res)
        return res

    # ---- multi-scale / mirrored evaluation ----------------------------------------------
    # DeepLab's evaluation protocol (the published mIoU figures): the image at several scales, each also mirrored, the class
    # probabilities of all passes averaged at the base resolution before the argmax.  The reference repository evaluates one scale,
    # unmirrored; the semantics below are this project's.  Per scale one dl3p_tta_accumulate launch adds the
    # plain and the mirrored pass into one running sum; the last launch writes no sum and leaves the mask / the confusion counters.
    def tta_scales(self, scales):
        """ValueError for what the multi-scale evaluation does not serve -> the scales as a tuple of floats"""
        if self.factory['family'] != 'deeplabv3p':
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
        """one inference model per scale, in the order given: this model for a scale that keeps its input shape, otherwise a sibling
        from the same factory with this model's arguments at (tta_size(H, s), tta_size(W, s)).  Siblings are cached per shape and built
        only when absent; every call refreshes their weights from this model's parameter store"""
        import contextlib
        import io
        from . import mixed_precision
        scales = self.tta_scales(scales)
        H, W = self.input_shape_hw
        cache = self._tta_cache
        out = []
        for s in scales:
            shape = (tta_size(H, s), tta_size(W, s))
            if shape == (H, W):
                out.append(self)
                continue
            if shape not in cache:
                if min(shape) < 1:
                    raise ValueError('scale %r gives the input shape %r' % (s, shape))
                f = self.factory
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
            st.P.copy_(store.P)             # device to device
            st.transpose()
        return out

    def _tta_frames(self, frames_u8, check_only=False):
        """uint8 frames (B,H,W,3) at the model's input shape, host or device -> a dense CUDA uint8 tensor"""
        import torch
        if not isinstance(frames_u8, torch.Tensor):
            frames_u8 = np.asarray(frames_u8)
        dt = frames_u8.dtype
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
        scales = self.tta_scales(scales)
        self._tta_frames(frames_u8, check_only=True)        # (every refusal comes before the first device call)
        models = self._tta_siblings(scales)
        frames = self._tta_frames(frames_u8)
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

    def predict_tta(self, frames_u8, scales=(1.0,), flip=False):
        """mean class probabilities over the passes of DeepLab's multi-scale / mirrored protocol: frames_u8 (B,H,W,3) uint8 at the
        model's input shape, on the host or the device -> (B,H,W,C) float32, (B,H*W,C) for a training-shaped model"""
        acc, _ = self._tta_run(frames_u8, scales, flip, want_sum=True)
        H, W = self.input_shape_hw
        p = acc[..., :self.num_classes].cpu().numpy()
        return p.reshape(p.shape[0], H * W, self.num_classes) if self.flatten_output else p


# model types whose graphs contain ops without a bf16 kernel on the TRAINING path are rejected when the model is built, not at
# the first train step.  Empty since round 3: the data gradient of a dense k x k conv (dl3p_col2im_bf16 behind the
# GEMM) and max pooling (dl3p_maxpool2d_*_bf16) closed the gap for Xception and ResNet50 -- train.py:37-46 applies the policy to
# every model type.  The U-Net types (get_unet_model) are refused under the policy whether built for training or not: the 2x2
# stride-2 transposed conv (csrc/deconv.hip) has no bf16 twin yet.
_NO_BF16_TRAINING = {'unet_standard': 'dl3p_deconv2x2_* has no bf16 kernels', 'unet_lite': 'dl3p_deconv2x2_* has no bf16 kernels',
                     'fast_scnn': 'the nearest-upsampling and window-pooling kernels have no bf16 twins'}


# ---- what the three factories share: the argument checks (each factory calls them in its own order, which decides which of two
# broken arguments is reported) and everything behind "the graph and its logits tensor exist"
def _check_num_classes(num_classes):
    if not 1 <= int(num_classes) <= 253:
        # PNG label maps hold fewer than 254 classes (train.py:34); up to 32 classes a pixel's class vector stays in
        # registers in the head kernels, beyond that they walk the classes (dl3p_upsample_softmax_loss)
        raise ValueError('num_classes must be in [1, 253] (got %r)' % (num_classes,))


def _check_bn_moving_variance(bn_moving_variance):
    if bn_moving_variance not in ('biased', 'unbiased'):
        raise ValueError("bn_moving_variance must be 'biased' or 'unbiased' (got %r)" % (bn_moving_variance,))


def _check_policy(model_type, bf16, training=None):
    """the mixed-precision refusal.  training True / False: a family whose inference runs in bf16, refused only when built for
    training; None: a family without bf16 kernels, refused either way"""
    if not bf16 or model_type not in _NO_BF16_TRAINING:
        return
    if training is None:
        raise ValueError("model type '%s' is not built for the mixed_bfloat16 policy (%s); build it under the float32 policy"
                         % (model_type, _NO_BF16_TRAINING[model_type]))
    if training:
        # the policy of train.py:37-46 applies to every model type there; here the mixed-precision kernels cover the
        # MobileNet families (BASELINE configs[4]).  Say so when the model is built, not at the first train step.
        raise ValueError("mixed_bfloat16 training is not built for model type '%s' (%s); build it under the float32 policy"
                         % (model_type, _NO_BF16_TRAINING[model_type]))


def _finish_model(g, logits, family, model_type, num_classes, shape, training, backbone_len, seed, bf16, name=None, output_stride=None,
                  bn_moving_variance='biased', weights_path=None, resize=None, reshape_name=None, logits_stride=None):
    """the tail of every factory: `resize` = (layer kind, name) of the family's weightless step from the logits to full resolution,
    -> [Reshape] -> Softmax('pred_mask'), the check that the logits are what the head kernels take (class dimension padded to the
    graph's alignment, a plain tensor, at 1 / logits_stride of the input where the family fixes that), the model and its weights"""
    H, W = shape
    out = logits
    if resize is not None:
        out = g.passthrough(out, resize[0], (H, W, num_classes), name=resize[1])
    if training:
        out = g.passthrough(out, 'Reshape', (H * W, num_classes), name=reshape_name)
    out = g.passthrough(out, 'Softmax', (H * W, num_classes) if training else (H, W, num_classes), name='pred_mask')
    g.output_layer = out.klayer
    t = logits.tensor
    cpad = (num_classes + g.align - 1) // g.align * g.align
    if t.C != cpad or not logits.is_plain or (logits_stride and (t.H * logits_stride, t.W * logits_stride) != (H, W)):
        raise AssertionError('head tensor layout')
    model = DeeplabModel(g, logits, model_type, num_classes, (H, W), training, backbone_len, seed=seed, bf16=bf16, family=family,
                         name=name, output_stride=output_stride, bn_moving_variance=bn_moving_variance)
    if weights_path:
        model.load_weights(weights_path, by_name=False)
        print('Load weights {}.'.format(weights_path))
    return model


def get_deeplabv3p_model(model_type, num_classes, model_input_shape, output_stride, freeze_level=0,
                         weights_path=None, training=True, use_subpixel=False, seed=0, bn_moving_variance='biased'):
    """deeplabv3p/model.py:51-117, same positional / keyword arguments.  Two extras, keyword-only in spirit:
    `seed` (weight initialisation) and `bn_moving_variance`, which of the two Keras classes CustomBatchNormalization
    (layers.py:63-70) can resolve to is restated for the MOVING variance: 'biased' = SyncBatchNormalization, Keras' non-fused
    path (TF 2.2 .. 2.9, and what north_star asks for: SyncBN over the global batch); 'unbiased' = plain fused
    BatchNormalization with Bessel's correction, which is what the string compare at layers.py:64 selects under the pinned
    tensorflow==2.11.0.  Training-mode outputs, losses and gradients do not depend on it; inference after
    training does (factor count / (count - 1) in the variance each step contributes)."""
    _check_bn_moving_variance(bn_moving_variance)
    from . import graph as graph_mod, mixed_precision
    bf16 = mixed_precision.is_bf16()        # the global policy at build time, like Keras layers pick theirs up
    graph_mod.CHANNEL_ALIGN = 8 if bf16 else 4
    try:
        return _build_model(model_type, num_classes, model_input_shape, output_stride, freeze_level, weights_path, training,
                            use_subpixel, seed, bf16, bn_moving_variance)
    finally:
        graph_mod.CHANNEL_ALIGN = 4


def _build_model(model_type, num_classes, model_input_shape, output_stride, freeze_level, weights_path, training,
                 use_subpixel, seed, bf16, bn_moving_variance):
    # check if model type is valid
    if model_type not in deeplab_model_map.keys():
        raise ValueError('This model type is not supported now')
    if use_subpixel:
        raise ValueError('Subpixel head is experimental in the reference (README TODO) and not on the hot path')
    _check_num_classes(num_classes)

    model_function = deeplab_model_map[model_type]
    H, W = model_input_shape
    _check_policy(model_type, bf16, training=bool(training))
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
    model = _finish_model(g, x, 'deeplabv3p', model_type, num_classes, (H, W), training, backbone_len, seed, bf16,
                          output_stride=output_stride, bn_moving_variance=bn_moving_variance, weights_path=weights_path,
                          resize=('Lambda', 'pred_resize'))

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
    _check_num_classes(num_classes)
    H, W = model_input_shape
    if H % 16 or W % 16:
        # four 2x2 poolings and four 2x upsamplings: Keras fails at the first `concatenate` otherwise
        raise ValueError('U-Net input height and width must be multiples of 16 (got %r)' % ((H, W),))
    _check_policy(model_type, mixed_precision.is_bf16())
    g, x = unet_mod.unet_model_map[model_type](num_classes, input_shape=(H, W, 3), weights=None, seed=seed)
    base_len = len(g.layers)
    # the classifier: a plain Conv2D(num_classes, 1, padding='same') -- glorot_uniform, zero bias, no regulariser -- reading the
    # 2 logical channels of the padded bottleneck; its class dimension is padded to a multiple of 4 like conv_upsample's
    cpad = (num_classes + g.align - 1) // g.align * g.align
    x = g.conv2d(x, num_classes, 1, None, use_bias=True, pad_to=cpad, l2=0.0)
    return _finish_model(g, x, 'unet', model_type, num_classes, (H, W), training, base_len, seed, False, name=model_type,
                         weights_path=weights_path, logits_stride=1)


def get_fast_scnn_model(model_type, num_classes, model_input_shape, weights_path=None, training=True, seed=0,
                        bn_moving_variance='biased'):
    """fast_scnn/model.py:19-45, same positional arguments (+ `seed` and `bn_moving_variance`, as get_deeplabv3p_model has them):
    'fast_scnn' with the reference's own head -- Dropout(0.3) -> UpSampling2D((8, 8)) -> [Reshape] -> Softmax('pred_mask') -- served
    by the nearest head kernels from the logits at H/8.  The returned model is a DeeplabModel like every other family's."""
    from . import mixed_precision, fast_scnn as fs_mod
    if model_type not in fs_mod.fast_scnn_model_map.keys():
        raise ValueError('This model type is not supported now')
    _check_num_classes(num_classes)
    _check_bn_moving_variance(bn_moving_variance)
    H, W = model_input_shape
    if H % 32 or W % 32 or H < 256 or W < 256:
        # five stride-2 stages, then pool_size = ((H / 32) // 8, (W / 32) // 8) in the pyramid pooling block: 0 below 256, and Keras
        # cannot build AveragePooling2D(pool_size=0)
        raise ValueError('Fast-SCNN input height and width must be multiples of 32 and at least 256: the pyramid pooling block '
                         'pools with pool_size = (H/32)//8, which Keras cannot build for smaller inputs (got %r)' % ((H, W),))
    _check_policy(model_type, mixed_precision.is_bf16())
    g, x = fs_mod.fast_scnn_model_map[model_type](num_classes, input_shape=(H, W, 3), weights=None, training=training, seed=seed)
    return _finish_model(g, x, 'fast_scnn', model_type, num_classes, (H, W), training, len(g.layers), seed, False, name='Fast_SCNN',
                         bn_moving_variance=bn_moving_variance, weights_path=weights_path, resize=('UpSampling2D', 'up_sampling2d_1'),
                         reshape_name='reshape', logits_stride=8)
