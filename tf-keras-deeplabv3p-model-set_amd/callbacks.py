"""The callbacks fit takes: the reference's EvalCallBack (common/callbacks.py) and tfa's AverageModelCheckpoint."""
import os

import numpy as np


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
