"""Fast-SCNN restated LITERALLY in float64, twice, written out from reading reference fast_scnn/models/fast_scnn.py:18-153 and
deeplabv3p/models/layers.py:

  FastSCNNOracle   on oracle.np_net.Net (NumPy tape): the reference of tests/test_fast_scnn_gpu.py.  The tape ops the oracle lacks are
                   added here: nearest upsampling (np.repeat), non-overlapping window average pooling, a separable conv with stride /
                   dilation and a regularised bias, a depthwise conv with a bias.
  FastSCNNTorch    the same network on torch-CPU autograd, written separately (its own walk, padding, naming): the twin that
                   tests/test_fast_scnn_cpu.py holds the NumPy restatement against (loss, every gradient, BatchNorm statistics).

Both are literal: a real UpSampling2D((4, 4)) in front of the dilation-4 separable conv at H/8, the class logits replicated 8 x 8 with a
softmax and a loss term per full-resolution pixel, a real concatenation for the pyramid pooling block, the depthwise bias added to z.
Nothing of the product's folding is in here.

Layer names are Keras' auto-names (one counter per layer class, in construction order), parameters are keyed '<layer>/<weight>' like
DeeplabModel.get_weights_by_name().  l2 (2e-5): DeeplabConv2D kernel and bias; the bias ONLY of DeeplabSeparableConv2D and
DeeplabDepthwiseConv2D (Keras hands kernel_regularizer to neither a depthwise nor a pointwise kernel).  Both classes share one interface:
params, table, l2_of, trainable, count_params, act_derivs / flip_count / flip_total, predict, loss_and_grads (-> cross-entropy; grads
hold d(ce + l2 penalty)), sgd_step.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import np_ops as O
from oracle.np_net import Net, Var

TOL = 1e-3
L2 = 2e-5
EPS, MOMENTUM = 1e-3, 0.99
BINS = (2, 4, 6, 8)
_BASE = {'conv': 'conv2d', 'bn': 'batch_normalization', 'sep': 'separable_conv2d', 'dw': 'depthwise_conv2d'}


def same_pad(x, k, s, d):
    """TF 'same' padding of an NCHW tensor for a k x k window, stride s, dilation d (the odd unit goes to the end)"""
    pads = []
    for size in (x.shape[3], x.shape[2]):
        out = -(-size // s)
        total = max((out - 1) * s + (k - 1) * d + 1 - size, 0)
        pads += [total // 2, total - total // 2]
    return F.pad(x, pads)


class FastSCNNTorch:
    """layer_table(): [(name, kind, {weight: shape})] in construction order; params: {name/weight: float64 array}"""

    def __init__(self, num_classes, input_shape, seed=0):
        self.C, (self.H, self.W) = num_classes, input_shape
        self.table = []
        # {BatchNorm name: 0 / 1 array (N, h, w, C)}: the branch the ReLU behind that BatchNorm took in the float32 run under test.  An
        # element within rounding distance of 0 can sit on the other side in float64 (an O(1) error in that element's gradient);
        # with the pattern handed in, the comparison measures the kernels.  flip_count of flip_total elements differed
        self.act_derivs, self.flip_count, self.flip_total = None, 0, 0
        self._walk(None)
        rng = np.random.default_rng(seed)
        self.params = {}
        for name, kind, ws in self.table:
            for key, shape in ws.items():
                if key in ('kernel', 'depthwise_kernel', 'pointwise_kernel'):
                    fan_in = int(np.prod(shape[:-1])) if key != 'depthwise_kernel' else 9 * shape[2]
                    fan_out = int(np.prod(shape[:2])) * shape[-1]
                    lim = np.sqrt(6.0 / (fan_in + fan_out))
                    v = rng.uniform(-lim, lim, shape)
                elif key in ('gamma', 'moving_variance'):
                    v = rng.uniform(0.5, 1.5, shape)
                else:                                   # biases, beta, moving means: away from 0, so that no gradient is noise
                    v = rng.uniform(-0.3, 0.3, shape)
                self.params['%s/%s' % (name, key)] = v.astype(np.float64)

    def l2_of(self, pname):
        layer, key = pname.rsplit('/', 1)
        kind = {n: k for n, k, _ in self.table}[layer]
        if kind == 'conv':
            return L2
        return L2 if (kind in ('sep', 'dw') and key == 'bias') else 0.0

    def trainable(self, pname):
        return not pname.endswith(('moving_mean', 'moving_variance'))

    # ------------------------------------------------------------------------------------------------ the network, once
    def _walk(self, run):
        """the reference's calls in order.  run is None: record the layer table; otherwise run(kind, name, x, **kw) executes"""
        cnt = {}

        def nm(kind):
            i = cnt.get(kind, 0)
            cnt[kind] = i + 1
            return _BASE[kind] if i == 0 else '%s_%d' % (_BASE[kind], i)

        def layer(kind, x, cin, cout=None, name=None, **kw):
            name = name or nm(kind)
            if run is not None:
                return run(kind, name, x, **kw)
            ws = {'conv': lambda: {'kernel': (kw['k'], kw['k'], cin, cout), 'bias': (cout,)},
                  'sep': lambda: {'depthwise_kernel': (3, 3, cin, 1), 'pointwise_kernel': (1, 1, cin, cout), 'bias': (cout,)},
                  'dw': lambda: {'depthwise_kernel': (3, 3, cin, 1), 'bias': (cin,)},
                  'bn': lambda: {'gamma': (cin,), 'beta': (cin,), 'moving_mean': (cin,), 'moving_variance': (cin,)}}[kind]()
            self.table.append((name, kind, ws))
            return None

        def op(f, *a):
            if run is None:
                return None
            return self._relu(a[0]) if f is F.relu else f(*a)

        def conv_block(x, kind, cin, cout, k, s, relu=True):
            x = layer(kind, x, cin, cout, k=k, s=s)
            x = layer('bn', x, cout)
            return op(F.relu, x) if relu else x

        def bottleneck(x, cin, cout, s, residual):
            inputs = x
            x = conv_block(x, 'conv', cin, 6 * cin, 1, 1)
            x = layer('dw', x, 6 * cin, s=s)
            x = layer('bn', x, 6 * cin)
            x = op(F.relu, x)
            x = conv_block(x, 'conv', 6 * cin, cout, 1, 1, relu=False)
            return op(torch.add, x, inputs) if residual else x

        x = conv_block(self._x if run else None, 'conv', 3, 32, 3, 2)
        x = conv_block(x, 'sep', 32, 48, 3, 2)
        lds = conv_block(x, 'sep', 48, 64, 3, 2)
        x, cin = lds, 64
        for cout, s in ((64, 2), (96, 2), (128, 1)):
            x = bottleneck(x, cin, cout, s, False)
            x = bottleneck(x, cout, cout, 1, True)
            x = bottleneck(x, cout, cout, 1, True)
            cin = cout
        h, w = self.H // 32, self.W // 32
        cat = [x]
        for b in BINS:
            y = op(lambda t: F.avg_pool2d(t, (h // b, w // b), stride=(h // b, w // b)), x)
            y = layer('conv', y, 128, 128, k=3, s=2)
            cat.append(op(lambda t: F.interpolate(t, size=(h, w), mode='bilinear', align_corners=False), y))
        gfe = op(lambda *t: torch.cat(t, 1), *cat)
        ff1 = conv_block(lds, 'conv', 64, 128, 1, 1, relu=False)
        ff2 = op(lambda t: t.repeat_interleave(4, 2).repeat_interleave(4, 3), gfe)
        ff2 = layer('sep', ff2, 640, 128, s=1, d=4)
        ff2 = layer('bn', ff2, 128)
        ff2 = op(F.relu, ff2)
        ff2 = layer('conv', ff2, 128, 128, k=1, s=1)
        x = op(torch.add, ff1, ff2)
        x = layer('bn', x, 128)
        x = op(F.relu, x)
        for name in ('DSConv1_classifier', 'DSConv2_classifier'):
            x = layer('sep', x, 128, 128, name=name, s=1)
            x = layer('bn', x, 128)
            x = op(F.relu, x)
        return conv_block(x, 'conv', 128, self.C, 1, 1, relu=False)

    def _relu(self, x):
        d = (self.act_derivs or {}).get(self._last_bn)
        if d is None:
            return F.relu(x)
        d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).permute(0, 3, 1, 2)
        if d.shape[2] * 4 == x.shape[2]:                 # the product ran this layer in front of the UpSampling2D((4, 4))
            d = d.repeat_interleave(4, 2).repeat_interleave(4, 3)
        self.flip_count += int(((x.detach() > 0).double() != d).sum())
        self.flip_total += d.numel()
        return x * d

    def count_params(self):
        return sum(int(np.prod(s)) for _, _, ws in self.table for s in ws.values())

    # ------------------------------------------------------------------------------------------------ execution
    def _forward(self, P, x, training, mask):
        """P: {name: float64 tensor}; -> logits (N, C, H/8, W/8) behind the Dropout, {bn name: (batch mean, biased var, count)}"""
        stats = {}

        def run(kind, name, t, k=3, s=1, d=1):
            g = lambda key: P['%s/%s' % (name, key)]
            if kind == 'conv':
                return F.conv2d(same_pad(t, k, s, 1), g('kernel').permute(3, 2, 0, 1), g('bias'), stride=s)
            if kind in ('sep', 'dw'):
                c = t.shape[1]
                t = F.conv2d(same_pad(t, 3, s, d), g('depthwise_kernel').permute(2, 3, 0, 1), None, stride=s, dilation=d, groups=c)
                if kind == 'dw':
                    return t + g('bias').view(1, -1, 1, 1)
                return F.conv2d(t, g('pointwise_kernel').permute(3, 2, 0, 1), g('bias'))
            self._last_bn = name
            if training:
                mean = t.mean((0, 2, 3))
                var = ((t - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
                stats[name] = (mean.detach().numpy(), var.detach().numpy(), t.numel() // t.shape[1])
            else:
                mean, var = g('moving_mean'), g('moving_variance')
            return (t - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS) * g('gamma').view(1, -1, 1, 1) \
                + g('beta').view(1, -1, 1, 1)
        self._x = x
        z = self._walk(run)
        if training and mask is not None:
            z = z * torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float64)).permute(0, 3, 1, 2) / (1.0 - 0.3)
        return z, stats

    def _tensors(self, grad):
        return {k: torch.tensor(v, dtype=torch.float64, requires_grad=grad and self.trainable(k)) for k, v in self.params.items()}

    def predict(self, x):
        """-> probabilities (N, H, W, C): inference-mode BatchNorm, no dropout, the logits replicated 8 x 8"""
        with torch.no_grad():
            z, _ = self._forward(self._tensors(False), torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), False, None)
            z = z.repeat_interleave(8, 2).repeat_interleave(8, 3)
            return torch.softmax(z, 1).permute(0, 2, 3, 1).numpy()

    def loss_and_grads(self, x, y, mask, ignore_index=255):
        """one training forward + backward.  mask: the Dropout keep mask (N, H/8, W/8, C) of 0 / 1.  -> cross-entropy (mean over all
        N H W entries, clipped to [1e-7, 1 - 1e-7], ignored labels contribute 0); self.grads = d(ce + l2 penalty) / d(weight),
        self.stats = the batch statistics of every BatchNorm"""
        P = self._tensors(True)
        z, self.stats = self._forward(P, torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), True, mask)
        z = z.repeat_interleave(8, 2).repeat_interleave(8, 3)
        N = z.shape[0]
        p = torch.softmax(z, 1).permute(0, 2, 3, 1).reshape(-1, self.C)
        lab = torch.from_numpy(y.reshape(-1).astype(np.int64))
        valid = (lab != ignore_index) & (lab >= 0) & (lab < self.C)
        pt = p.gather(1, torch.where(valid, lab, torch.zeros_like(lab)).view(-1, 1)).view(-1)
        ce = (-(pt.clamp(1e-7, 1 - 1e-7)).log() * valid).sum() / lab.numel()
        # the clip stops the gradient outside (1e-7, 1 - 1e-7), as tf.clip_by_value does
        reg = sum(self.l2_of(k) * (t ** 2).sum() for k, t in P.items() if self.trainable(k) and self.l2_of(k))
        (ce + reg).backward()
        self.grads = {k: t.grad.numpy() for k, t in P.items() if t.requires_grad}
        return float(ce.detach())

    def sgd_step(self, lr, momentum, moving_variance='biased'):
        """Keras SGD(momentum), first step (v = -lr g), and the moving statistics of every BatchNorm"""
        for k, g in self.grads.items():
            self.params[k] = self.params[k] - lr * g
        for name, (mean, var, count) in self.stats.items():
            if moving_variance == 'unbiased':
                var = var * count / (count - 1.0)
            self.params[name + '/moving_mean'] = self.params[name + '/moving_mean'] * MOMENTUM + mean * (1 - MOMENTUM)
            self.params[name + '/moving_variance'] = self.params[name + '/moving_variance'] * MOMENTUM + var * (1 - MOMENTUM)


def data(N, H, W, C, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
    y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
    y[rng.uniform(size=y.shape) < 0.05] = 255
    return x, y


# ---- the restatement on oracle.np_net.Net ---------------------------------------------------------------------------------------
class FastSCNNNet(Net):
    """oracle.np_net.Net + the tape ops Fast-SCNN needs that it lacks, and Keras' auto-names"""

    def __init__(self, dtype=np.float64, seed=0):
        super().__init__(dtype, seed)
        self.counters = {}
        self.kinds = {}              # layer name -> 'conv' | 'sep' | 'dw' | 'bn', in construction order

    def auto(self, base, kind=None):
        i = self.counters.get(base, 0)
        self.counters[base] = i + 1
        name = base if i == 0 else '%s_%d' % (base, i)
        if kind:
            self.kinds[name] = kind
        return name

    def _uniform(self, lo, hi):
        return lambda s: self.rng.uniform(lo, hi, s)

    def conv(self, x, filters, k, stride=1):
        """DeeplabConv2D: kernel and bias, l2 on both (Net.conv2d)"""
        name = self.auto('conv2d', 'conv')
        y = self.conv2d(x, filters, k, name, stride=stride, use_bias=True)
        return y

    def separable(self, x, filters, stride=1, rate=1, name=None):
        """DeeplabSeparableConv2D: ONE layer -- 3x3 depthwise (stride, dilation; no bias) then 1x1 + bias; l2 on the bias only"""
        if name is None:
            name = self.auto('separable_conv2d', 'sep')
        else:
            self.kinds[name] = 'sep'
        cin = x.v.shape[-1]
        wd4 = self.param(name + '/depthwise_kernel', (3, 3, cin, 1), lambda s: O.glorot_uniform(self.rng, s, 9 * cin, 9), l2=0.0)
        wp = self.param(name + '/pointwise_kernel', (1, 1, cin, filters), lambda s: O.glorot_uniform(self.rng, s, cin, filters), l2=0.0)
        b = self.param(name + '/bias', (filters,), np.zeros, l2=O.L2_FACTOR)
        wd = wd4[..., 0]
        mid = O.dwconv2d_fwd(x.v, wd, stride, rate, 'same')
        y = Var(O.conv2d_fwd(mid, wp, 1, 1, 'same', b))

        def bwd():
            if y.g is None:
                return
            gmid, gwp, gb = O.conv2d_bwd(mid, wp, y.g, 1, 1, 'same', True)
            gx, gwd = O.dwconv2d_bwd(x.v, wd, gmid, stride, rate, 'same')
            self.acc_grad(name + '/depthwise_kernel', gwd[..., None])
            self.acc_grad(name + '/pointwise_kernel', gwp)
            self.acc_grad(name + '/bias', gb)
            x.acc(gx)
        self.tape.append(bwd)
        return y

    def depthwise(self, x, stride):
        """DeeplabDepthwiseConv2D with Keras' default bias, ADDED to z; l2 on the bias only"""
        name = self.auto('depthwise_conv2d', 'dw')
        z = self.dwconv2d(x, 3, name, stride=stride)
        b = self.param(name + '/bias', (x.v.shape[-1],), np.zeros, l2=O.L2_FACTOR)
        y = Var(z.v + b)

        def bwd():
            if y.g is not None:
                self.acc_grad(name + '/bias', y.g.sum((0, 1, 2)))
                z.acc(y.g)
        self.tape.append(bwd)
        return y

    def batchnorm(self, x):
        return self.bn(x, self.auto('batch_normalization', 'bn'))

    def relu_(self, x):
        """ReLU behind a BatchNorm; an injected branch pattern recorded in front of a folded UpSampling2D((4, 4)) is replicated"""
        d = self.act_derivs.get(x.tag) if isinstance(x.tag, str) else None
        if d is not None and d.shape[1] * 4 == x.v.shape[1]:
            self.act_derivs[x.tag] = np.repeat(np.repeat(d, 4, 1), 4, 2)
        return self.relu(x)

    def upsample(self, x, r):
        """UpSampling2D((r, r)), nearest: np.repeat; backward sums every r x r block"""
        N, H, W, C = x.v.shape
        y = Var(np.repeat(np.repeat(x.v, r, 1), r, 2))

        def bwd():
            if y.g is not None:
                x.acc(y.g.reshape(N, H, r, W, r, C).sum((2, 4)))
        self.tape.append(bwd)
        return y

    def avgpool(self, x, kh, kw):
        """AveragePooling2D((kh, kw), strides=(kh, kw)), 'valid': floor-sized; uncovered rows and columns get no gradient"""
        N, H, W, C = x.v.shape
        Ho, Wo = H // kh, W // kw
        y = Var(x.v[:, :Ho * kh, :Wo * kw].reshape(N, Ho, kh, Wo, kw, C).mean((2, 4)))

        def bwd():
            if y.g is not None:
                g = np.zeros_like(x.v)
                g[:, :Ho * kh, :Wo * kw] = np.repeat(np.repeat(y.g, kh, 1), kw, 2) / (kh * kw)
                x.acc(g)
        self.tape.append(bwd)
        return y


def fast_scnn_body(net, x, num_classes):
    """fast_scnn.py:86-141, line by line -> the logits at H/8 in front of the Dropout"""
    def conv_block(t, conv_type, filters, k, stride, relu=True):                                   # :18-33
        t = net.separable(t, filters, stride) if conv_type == 'ds' else net.conv(t, filters, k, stride)
        t = net.batchnorm(t)
        return net.relu_(t) if relu else t

    def res_bottleneck(inputs, filters, t, s, r=False):                                            # :36-52
        y = conv_block(inputs, 'conv', inputs.v.shape[-1] * t, 1, 1)
        y = net.depthwise(y, s)
        y = net.relu_(net.batchnorm(y))
        y = conv_block(y, 'conv', filters, 1, 1, relu=False)
        return net.add(y, inputs) if r else y

    def bottleneck_block(t, filters, expansion, strides, n):                                       # :55-64
        t = res_bottleneck(t, filters, expansion, strides)
        for _ in range(1, n):
            t = res_bottleneck(t, filters, expansion, 1, True)
        return t

    lds = conv_block(x, 'conv', 32, 3, 2)                                                          # :102-104
    lds = conv_block(lds, 'ds', 48, 3, 2)
    lds = conv_block(lds, 'ds', 64, 3, 2)
    gfe = bottleneck_block(lds, 64, 6, 2, 3)                                                       # :109-111
    gfe = bottleneck_block(gfe, 96, 6, 2, 3)
    gfe = bottleneck_block(gfe, 128, 6, 1, 3)
    h, w = gfe.v.shape[1:3]                                                                        # :67-83
    cat = [gfe]
    for b in (2, 4, 6, 8):
        t = net.avgpool(gfe, h // b, w // b)
        t = net.conv(t, 128, 3, 2)
        cat.append(net.resize(t, h, w))
    gfe = net.concat(cat)
    ff1 = conv_block(lds, 'conv', 128, 1, 1, relu=False)                                           # :115-128
    ff2 = net.upsample(gfe, 4)
    ff2 = net.separable(ff2, 128, 1, rate=4)
    ff2 = net.relu_(net.batchnorm(ff2))
    ff2 = net.conv(ff2, 128, 1, 1)
    ff = net.relu_(net.batchnorm(net.add(ff1, ff2)))
    c = net.relu_(net.batchnorm(net.separable(ff, 128, name='DSConv1_classifier')))                # :131-139
    c = net.relu_(net.batchnorm(net.separable(c, 128, name='DSConv2_classifier')))
    return conv_block(c, 'conv', num_classes, 1, 1, relu=False)


class FastSCNNOracle:
    """the NumPy restatement behind the interface of FastSCNNTorch.  Weights: the twin's initialisation (same seed, same numbers),
    so that the two start equal; every test overwrites them anyway"""

    def __init__(self, num_classes, input_shape, seed=0):
        self.C, (self.H, self.W) = num_classes, input_shape
        self.net = FastSCNNNet(np.float64, seed)
        self.act_derivs = None
        self.moving_variance = 'biased'          # which batch variance feeds the moving average (Net.bn_moving_variance)
        self._run(np.zeros((1, self.H, self.W, 3)), False, None)            # creates the parameters, in Keras order
        net = self.net
        self.table = []
        for name in net.order:
            layer, key = name.rsplit('/', 1)
            if not self.table or self.table[-1][0] != layer:
                self.table.append((layer, net.kinds[layer], {}))
            self.table[-1][2][key] = net.params[name].shape
        self.params = dict(FastSCNNTorch(num_classes, input_shape, seed).params)
        assert sorted(self.params) == sorted(net.params)

    flip_count = property(lambda self: self.net.flip_count)
    flip_total = property(lambda self: self.net.flip_total)

    def l2_of(self, pname):
        return self.net.l2[pname]

    def trainable(self, pname):
        return self.net.trainable[pname]

    def count_params(self):
        return sum(int(np.prod(v.shape)) for v in self.net.params.values())

    def _run(self, x, training, mask):
        net = self.net
        net.counters, net.bn_moving_variance = {}, self.moving_variance
        net.begin(training)
        net.act_derivs = {k: np.asarray(v, np.float64) for k, v in (self.act_derivs or {}).items()} if training else {}
        net.dropout_masks = {} if mask is None else {'dropout': np.asarray(mask, np.float64)}
        z = fast_scnn_body(net, Var(np.asarray(x, np.float64)), self.C)
        z = net.dropout(z, net.auto('dropout'), 0.3)                                               # :141
        return net.upsample(z, 8)                                                                  # :143

    def _load(self):
        for k, v in self.params.items():
            self.net.params[k] = np.asarray(v, np.float64)

    def predict(self, x):
        self._load()
        z = self._run(x, False, None).v
        e = np.exp(z - z.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)

    def loss_and_grads(self, x, y, mask, ignore_index=255):
        self._load()
        net = self.net
        logits = self._run(x, True, mask)
        N, H, W, C = logits.v.shape
        ce, _, dlogits = O.loss_fwd_bwd(logits.v, np.asarray(y, np.float64).reshape(N, H, W), None, ignore_index)
        logits.g = dlogits
        net.backward()
        self.grads = {k: net.grads[k] + 2.0 * net.l2[k] * net.params[k] for k in net.params if net.trainable[k]}
        return float(ce)

    def sgd_step(self, lr, momentum, moving_variance='biased'):
        """Keras SGD(momentum), first step, and the moving statistics the last training forward left (its moving_variance setting)"""
        assert self.moving_variance == moving_variance
        for k, g in self.grads.items():
            self.params[k] = self.params[k] - lr * g
        for k, v in self.net.moving_updates.items():
            self.params[k] = v
