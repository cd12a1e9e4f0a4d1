"""The optimisers compile() takes: Keras' SGD / Adam / RMSprop with their clipping keywords, tensorflow-addons' averaging wrappers
and the reference's get_optimizer (common/model_utils.py:112-172).  Configuration holders: the arithmetic runs on the device."""
import numpy as np


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
