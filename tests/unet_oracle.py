"""Float64 restatement of the U-Net family (reference unet/models/unet.py UNetStandard / UNetLite, unet/model.py) for the tests,
on the oracle's tape (oracle/np_net.py Net) the way tests/ghostnet_oracle.py is.  Two tape ops the oracle does not have are added
HERE: `conv2d_transpose` (Conv2DTranspose(filters, 2, strides=(2, 2)): forward, data, weight and bias gradient) and the
`separable_conv2d` helper (one Keras layer: depthwise_kernel, pointwise_kernel, bias).  `UNetOracle` is the NumPy restatement,
`torch_oracle` the same graph on torch-CPU autograd (`UNetTorchNet`) to triangulate it against.

Written out from the reference file, with real concatenations; not derived from the product's unet.py.  Layer names are what a
fresh Keras session gives (conv2d, conv2d_1, ..., conv2d_transpose, separable_conv2d, ...): each class counts its own instances
in creation order.  Plain Keras layers carry no regulariser: every parameter has l2 = 0."""
import numpy as np

from oracle import np_ops as O
from oracle.np_net import Net, OracleModel, Var
from peleenet_oracle import TOL, data, rel

UNET_TYPES = ('unet_standard', 'unet_lite')


# ---- the transposed conv as plain NumPy (k == stride == 2, no padding: every output pixel has exactly one tap) -------------
def conv2d_transpose_fwd(x, w, b=None):
    """x (N,H,W,Cin), w the Keras kernel as stored (2,2,Cout,Cin) -> (N,2H,2W,Cout): y[n,2h+p,2w+q,o] = sum_i x[n,h,w,i] w[p,q,o,i]"""
    N, H, W, _ = x.shape
    y = np.einsum('nhwi,pqoi->nhpwqo', x, w).reshape(N, 2 * H, 2 * W, w.shape[2])
    return y if b is None else y + b


def conv2d_transpose_bwd(x, w, gy):
    """-> (gx, gw, gb)"""
    N, H, W, _ = x.shape
    g6 = gy.reshape(N, H, 2, W, 2, gy.shape[-1])
    return (np.einsum('nhpwqo,pqoi->nhwi', g6, w), np.einsum('nhwi,nhpwqo->pqoi', x, g6), gy.sum((0, 1, 2)))


class UNetNet(Net):
    """Net + the layers of the U-Net files.  Keras auto-names: one counter per layer class"""

    def begin(self, training=True):
        super().begin(training)
        self._count = {}

    def auto_name(self, base):
        n = self._count.get(base, 0)
        self._count[base] = n + 1
        return base if n == 0 else '%s_%d' % (base, n)

    def plain_conv2d(self, x, filters, k, he_normal=True, relu=True):
        """Conv2D(filters, k, activation='relu', padding='same', kernel_initializer='he_normal'): bias, no regulariser"""
        name = self.auto_name('conv2d')
        cin = x.v.shape[-1]
        init = ((lambda s: O.he_normal(self.rng, s, k * k * cin)) if he_normal else
                (lambda s: O.glorot_uniform(self.rng, s, k * k * cin, k * k * filters)))
        w = self.param(name + '/kernel', (k, k, cin, filters), init, l2=0.0)
        b = self.param(name + '/bias', (filters,), np.zeros, l2=0.0)
        y = Var(O.conv2d_fwd(x.v, w, 1, 1, 'same', b))

        def bwd():
            if y.g is None:
                return
            gx, gw, gb = O.conv2d_bwd(x.v, w, y.g, 1, 1, 'same', True)
            self.acc_grad(name + '/kernel', gw)
            self.acc_grad(name + '/bias', gb)
            x.acc(gx)
        self.tape.append(bwd)
        y.tag = name            # Net.act: the injected ReLU pattern is looked up by this name
        return self.relu(y) if relu else y

    def conv2d_transpose(self, x, filters, relu=True):
        """Conv2DTranspose(filters, 2, strides=(2, 2), activation='relu', kernel_initializer='he_normal'); the kernel is stored
        (2, 2, filters, Cin) and Keras takes the fans from that shape: fan_in = 4 filters"""
        name = self.auto_name('conv2d_transpose')
        cin = x.v.shape[-1]
        w = self.param(name + '/kernel', (2, 2, filters, cin), lambda s: O.he_normal(self.rng, s, 4 * filters), l2=0.0)
        b = self.param(name + '/bias', (filters,), np.zeros, l2=0.0)
        y = Var(conv2d_transpose_fwd(x.v, w, b))

        def bwd():
            if y.g is None:
                return
            gx, gw, gb = conv2d_transpose_bwd(x.v, w, y.g)
            self.acc_grad(name + '/kernel', gw)
            self.acc_grad(name + '/bias', gb)
            x.acc(gx)
        self.tape.append(bwd)
        y.tag = name
        return self.relu(y) if relu else y

    def separable_conv2d(self, x, filters, relu=True):
        """SeparableConv2D(filters, 3, activation='relu', padding='same'): depthwise 3x3 (no bias, no activation) then 1x1 + bias;
        both kernels glorot_uniform (kernel_initializer does not reach them; unpinned reading)"""
        name = self.auto_name('separable_conv2d')
        cin = x.v.shape[-1]
        wd4 = self.param(name + '/depthwise_kernel', (3, 3, cin, 1), lambda s: O.glorot_uniform(self.rng, s, 9 * cin, 9), l2=0.0)
        wp = self.param(name + '/pointwise_kernel', (1, 1, cin, filters), lambda s: O.glorot_uniform(self.rng, s, cin, filters), l2=0.0)
        b = self.param(name + '/bias', (filters,), np.zeros, l2=0.0)
        wd = wd4[..., 0]
        mid = O.dwconv2d_fwd(x.v, wd, 1, 1, 'same')
        y = Var(O.conv2d_fwd(mid, wp, 1, 1, 'same', b))

        def bwd():
            if y.g is None:
                return
            gmid, gwp, gb = O.conv2d_bwd(mid, wp, y.g, 1, 1, 'same', True)
            gx, gwd = O.dwconv2d_bwd(x.v, wd, gmid, 1, 1, 'same')
            self.acc_grad(name + '/depthwise_kernel', gwd[..., None])
            self.acc_grad(name + '/pointwise_kernel', gwp)
            self.acc_grad(name + '/bias', gb)
            x.acc(gx)
        self.tape.append(bwd)
        y.tag = name
        return self.relu(y) if relu else y

    def maxpool(self, x):
        self.auto_name('max_pooling2d')
        return self.maxpool2d(x, 2, 2, (0, 0, 0, 0))

    def drop(self, x):
        return self.dropout(x, self.auto_name('dropout'), 0.5)


def unet_body(net, x, lite):
    """unet.py:28-69 (UNetStandard) / :97-138 (UNetLite), line by line"""
    conv = net.separable_conv2d if lite else (lambda t, f: net.plain_conv2d(t, f, 3))
    conv1 = conv(conv(x, 64), 64)
    pool1 = net.maxpool(conv1)
    conv2 = conv(conv(pool1, 128), 128)
    pool2 = net.maxpool(conv2)
    conv3 = conv(conv(pool2, 256), 256)
    pool3 = net.maxpool(conv3)
    conv4 = conv(conv(pool3, 512), 512)
    drop4 = net.drop(conv4)
    pool4 = net.maxpool(drop4)
    conv5 = conv(conv(pool4, 1024), 1024)
    drop5 = net.drop(conv5)
    up6 = net.conv2d_transpose(drop5, 512)
    conv6 = conv(conv(net.concat([drop4, up6]), 512), 512)
    up7 = net.conv2d_transpose(conv6, 256)
    conv7 = conv(conv(net.concat([conv3, up7]), 256), 256)
    up8 = net.conv2d_transpose(conv7, 128)
    conv8 = conv(conv(net.concat([conv2, up8]), 128), 128)
    up9 = net.conv2d_transpose(conv8, 64)
    conv9 = conv(conv(net.concat([conv1, up9]), 64), 64)
    return conv(conv9, 2)


class UNetOracle(OracleModel):
    """get_unet_model (unet/model.py:21-61) restated: body, Conv2D(num_classes, 1) logits at full resolution, Softmax"""
    net_class = UNetNet

    def __init__(self, model_type, num_classes, input_shape, dtype=np.float64, seed=0):
        if model_type not in UNET_TYPES:
            raise ValueError('This model type is not supported now')
        self.model_type, self.num_classes = model_type, num_classes
        self.H, self.W = input_shape
        self.net = self.net_class(dtype, seed)
        self.velocity = {}
        self.freeze_level = 0
        self._forward_graph(np.zeros((1, 16, 16, 3), dtype=np.float64), 16, 16, training=False)

    def _forward_graph(self, x, H, W, training):
        net = self.net
        net.begin(training)
        y = unet_body(net, Var(net.q(x)), self.model_type == 'unet_lite')
        net.tap('head_in', y)
        logits = net.plain_conv2d(y, self.num_classes, 1, he_normal=False, relu=False)      # Conv2D(num_classes, 1, padding="same")
        net.tap('logits', logits)
        return logits


# ---- the same graph on torch-CPU autograd ---------------------------------------------------------------------------------
def torch_oracle(*args, **kw):
    import torch
    import torch.nn.functional as F
    from oracle.torch_net import TorchModel, TorchNet, _nchw, _nhwc

    class UNetTorchNet(TorchNet, UNetNet):
        def plain_conv2d(self, x, filters, k, he_normal=True, relu=True):
            name = self.auto_name('conv2d')
            cin = x.v.shape[-1]
            init = ((lambda s: O.he_normal(self.rng, s, k * k * cin)) if he_normal else
                    (lambda s: O.glorot_uniform(self.rng, s, k * k * cin, k * k * filters)))
            w = self.tparam(name + '/kernel', (k, k, cin, filters), init)
            b = self.tparam(name + '/bias', (filters,), np.zeros)
            y = Var(_nhwc(F.conv2d(_nchw(x.v), w.permute(3, 2, 0, 1), b, padding=k // 2)))
            return self.relu(y) if relu else y

        def conv2d_transpose(self, x, filters, relu=True):
            name = self.auto_name('conv2d_transpose')
            cin = x.v.shape[-1]
            w = self.tparam(name + '/kernel', (2, 2, filters, cin), lambda s: O.he_normal(self.rng, s, 4 * filters))
            b = self.tparam(name + '/bias', (filters,), np.zeros)
            # torch's transposed-conv weight is (Cin, Cout, kh, kw) and, like Keras', is not flipped
            y = Var(_nhwc(F.conv_transpose2d(_nchw(x.v), w.permute(3, 2, 0, 1), b, stride=2)))
            return self.relu(y) if relu else y

        def separable_conv2d(self, x, filters, relu=True):
            name = self.auto_name('separable_conv2d')
            cin = x.v.shape[-1]
            wd = self.tparam(name + '/depthwise_kernel', (3, 3, cin, 1), lambda s: O.glorot_uniform(self.rng, s, 9 * cin, 9))
            wp = self.tparam(name + '/pointwise_kernel', (1, 1, cin, filters), lambda s: O.glorot_uniform(self.rng, s, cin, filters))
            b = self.tparam(name + '/bias', (filters,), np.zeros)
            mid = F.conv2d(_nchw(x.v), wd.permute(2, 3, 0, 1), None, padding=1, groups=cin)
            y = Var(_nhwc(F.conv2d(mid, wp.permute(3, 2, 0, 1), b)))
            return self.relu(y) if relu else y

    class UNetTorchOracle(UNetOracle, TorchModel):
        net_class = UNetTorchNet
    return UNetTorchOracle(*args, **kw)


def relu_derivs(m, ex):
    """ReLU'(z) of every conv + bias + ReLU layer as the device holds z (the U-Net types have no other activation), by Keras layer
    name: handed to the float64 restatement (Net.act_derivs) so that elements within rounding distance of the kink take the branch
    the device took"""
    out = {}
    for op in m.graph.ops:
        if op.kind in ('conv_dense', 'conv_deconv', 'conv_pw') and op.out is not m.head.tensor:      # (the classifier has no ReLU)
            C = op.layer.output_shape[-1]
            out[op.layer.name] = (ex.view(op.out)[..., :C].cpu().numpy() > 0).astype(np.float64)
    return out


def randomise(o):
    """non-trivial biases (Keras starts them at zero), as tests/test_ghostnet_gpu.py::_randomise does: without them the 2-channel
    ReLU bottleneck in front of the classifier can be dead"""
    rng, rng_dw = np.random.default_rng(42), np.random.default_rng(43)
    for k, v in o.net.params.items():
        if k.endswith('/depthwise_kernel'):
            # Keras' default glorot_uniform on a (3, 3, Cin, 1) kernel has fan_in = 9 Cin: each of unet_lite's 19 separable layers
            # shrinks its signal about sixfold and the encoder's gradients arrive at 1e-11, under the 1e-6 floor of rel() -- the
            # comparison would be its absolute branch.  The test case redraws them variance-preserving (N(0, 2 / 9), the He scale
            # of a 9-tap filter in front of a ReLU), so that every gradient is compared relatively.
            v[...] = rng_dw.standard_normal(v.shape) * np.sqrt(2.0 / 9.0)
        elif k.endswith('/bias'):
            v[...] = rng.standard_normal(v.shape) * 0.1
        else:
            continue
        if hasattr(o.net, 't'):             # the torch twin holds its own copies
            import torch
            with torch.no_grad():
                o.net.t[k].copy_(torch.as_tensor(v))


GPU_CASE = dict(N=2, H=32, W=32, C=21, seed=3)


def gpu_case(model_type, factory=None, H=None, W=None):
    """the case of tests/test_unet_gpu.py's train step: (restatement with randomised biases, x, y, host-drawn dropout masks)"""
    c = dict(GPU_CASE)
    H, W = H or c['H'], W or c['W']
    o = (factory or UNetOracle)(model_type, c['C'], (H, W))
    randomise(o)
    x, y = data(c['N'], H, W, c['C'], seed=c['seed'])
    rng = np.random.default_rng(7)
    masks = {'dropout': (rng.uniform(size=(c['N'], H // 8, W // 8, 512)) >= 0.5).astype(np.float64),
             'dropout_1': (rng.uniform(size=(c['N'], H // 16, W // 16, 1024)) >= 0.5).astype(np.float64)}
    return o, x, y, masks


__all__ = ['randomise', 'gpu_case', 'GPU_CASE', 'UNetOracle', 'UNetNet', 'torch_oracle', 'conv2d_transpose_fwd', 'conv2d_transpose_bwd', 'unet_body', 'UNET_TYPES',
           'O', 'TOL', 'data', 'rel', 'relu_derivs']
