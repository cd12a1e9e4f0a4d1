"""Float64 restatement of DeepLabV3+ PeleeNet (reference deeplabv3p/models/deeplabv3p_peleenet.py) for the tests: the body is
built from the oracle's primitive layers (oracle/np_net.py conv2d / bn / relu / concat / maxpool2d) plus a local average pool
of its own, on the same tape; the heads are the oracle's ASPP / ASPP-Lite / decoder blocks.  `PeleeOracle` is the NumPy
restatement, `PeleeTorchOracle` the same graph on torch-CPU autograd (oracle/torch_net.py) -- an independent implementation
of every primitive and of reverse-mode differentiation to triangulate the NumPy one against.

Written out from the reference's code, not from the product's graph builder (peleenet.py): the concatenations here are real
copies, the dense blocks real Concatenate layers."""
import numpy as np

from oracle import np_ops as O
from oracle.np_net import OracleModel, Var

PELEE_TYPES = ('peleenet', 'peleenet_lite')


# ---- local average pooling (AveragePooling2D(k, strides, 'valid'), deeplabv3p_peleenet.py:249-253) ------------------------
def avgpool2d_fwd(x, k, stride):
    """x (N,H,W,C) -> floor-sized mean of the k x k windows, taps summed in (ky, kx) order"""
    N, H, W, C = x.shape
    Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
    y = np.zeros((N, Ho, Wo, C), dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            y += x[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
    return y / (k * k)


def avgpool2d_bwd(gy, x_shape, k, stride):
    N, H, W, C = x_shape
    Ho, Wo = gy.shape[1:3]
    gx = np.zeros(x_shape, dtype=gy.dtype)
    for ky in range(k):
        for kx in range(k):
            gx[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :] += gy
    return gx / (k * k)


def _avgpool(net, x, k, stride):
    if hasattr(net, 't'):                     # TorchNet: torch tensors under autograd
        import torch.nn.functional as F
        return Var(F.avg_pool2d(x.v.permute(0, 3, 1, 2), k, stride).permute(0, 2, 3, 1))
    y = Var(net.q(avgpool2d_fwd(x.v, k, stride)))
    shape = x.v.shape

    def bwd():
        if y.g is not None:
            x.acc(avgpool2d_bwd(y.g, shape, k, stride))
    net.tape.append(bwd)
    return y


# ---- the PeleeNet body (deeplabv3p_peleenet.py:63-298) ---------------------------------------------------------------------
def _basic(net, x, c, k, stride, padding, name):
    x = net.conv2d(x, c, k, name + '_conv', stride=stride, padding=padding)
    x = net.bn(x, name + '_norm')
    return net.relu(x)


def _dense(net, x, growth_rate, bottleneck_width, name):
    growth_rate = int(growth_rate / 2)
    inter_channel = int(growth_rate * bottleneck_width / 4) * 4
    num_input_features = x.v.shape[-1]
    if inter_channel > num_input_features / 2:
        inter_channel = int(num_input_features / 8) * 4
    b1 = _basic(net, x, inter_channel, 1, 1, 'valid', name + '_branch1a')
    b1 = _basic(net, b1, growth_rate, 3, 1, 'same', name + '_branch1b')
    b2 = _basic(net, x, inter_channel, 1, 1, 'valid', name + '_branch2a')
    b2 = _basic(net, b2, growth_rate, 3, 1, 'same', name + '_branch2b')
    b2 = _basic(net, b2, growth_rate, 3, 1, 'same', name + '_branch2c')
    return net.concat([x, b1, b2])


def peleenet_body(net, x, OS, growth_rate=32, block_config=(3, 4, 8, 6), num_init_features=32, bottleneck_width=(1, 2, 4, 4)):
    name = 'bbn_features_stemblock'
    out = _basic(net, x, num_init_features, 3, 2, 'same', name + '_stem1')
    b2 = _basic(net, out, num_init_features // 2, 1, 1, 'valid', name + '_stem2a')
    b2 = _basic(net, b2, num_init_features, 3, 2, 'same', name + '_stem2b')
    b1 = net.maxpool2d(out, 2, 2, (0, 0, 0, 0))
    f = _basic(net, net.concat([b1, b2]), num_init_features, 1, 1, 'valid', name + '_stem3')
    num_features = num_init_features
    skip = None
    for i, n in enumerate(block_config):
        for j in range(n):
            f = _dense(net, f, growth_rate, bottleneck_width[i], 'bbn_features_denseblock%d_denselayer%d' % (i + 1, j + 1))
        num_features += n * growth_rate
        f = _basic(net, f, num_features, 1, 1, 'valid', 'bbn_features_transition%d' % (i + 1))
        if i == 0:
            skip = f
        if (OS == 8 and i < 1) or (OS == 16 and i < 2) or (OS == 32 and i != len(block_config) - 1):
            f = _avgpool(net, f, 2, 2)
    return f, skip


class PeleeOracle(OracleModel):
    """OracleModel (oracle/np_net.py) for the two PeleeNet types: same head, parameters, freeze levels and train step"""

    def __init__(self, model_type, num_classes, input_shape, output_stride, dtype=np.float64, seed=0, freeze_level=0,
                 bn_moving_variance='biased'):
        if model_type not in PELEE_TYPES:
            raise ValueError('This model type is not supported now')
        self.model_type = model_type
        self.num_classes = num_classes
        self.H, self.W = input_shape
        self.OS = output_stride
        self.net = self.net_class(dtype, seed)
        self.net.bn_moving_variance = bn_moving_variance
        self.velocity = {}
        self.freeze_level = freeze_level
        # parameters materialise in one dry forward on a small probe (64 x 64: the smallest size the OS 32 table takes)
        self._forward_graph(np.zeros((1, 64, 64, 3), dtype=np.float64), 64, 64, training=False)
        self.backbone_param_names = list(self._backbone_names)
        if freeze_level in (1, 2):
            for n in self.net.order:
                layer = n.rsplit('/', 1)[0]
                frozen = layer != 'conv_upsample' if freeze_level == 2 else layer in self._backbone_layers
                self.net.layer_trainable[layer] = not frozen

    def _forward_graph(self, x, H, W, training):
        net = self.net
        net.begin(training)
        xin = Var(net.q(x))
        n_before = len(net.order)
        f, skip = peleenet_body(net, xin, self.OS)
        if not hasattr(self, '_backbone_names'):
            self._backbone_names = net.order[n_before:]
            self._backbone_layers = {n.rsplit('/', 1)[0] for n in self._backbone_names}
        net.tap('backbone_out', f)
        if self.model_type.endswith('_lite'):
            y = net.aspp_lite_block(f)
        else:
            y = net.aspp_block(f, self.OS)
            net.tap('aspp_out', y)
            y = net.decoder_block(y, skip)
        net.tap('head_in', y)
        y = net.conv2d(y, self.num_classes, 1, 'conv_upsample', use_bias=True, keep_f32=True)
        net.tap('conv_upsample', y)
        logits = net.resize(y, H, W, keep_f32=True)
        net.tap('pred_resize', logits)
        return logits


def torch_oracle(*args, **kw):
    """the same graph on torch-CPU autograd (import deferred: torch is only needed by the triangulation)"""
    from oracle.torch_net import TorchModel

    class PeleeTorchOracle(PeleeOracle, TorchModel):
        pass
    return PeleeTorchOracle(*args, **kw)


# ---- shared by the GPU tests of the PeleeNet types ----------------------------------------------------------------------
TOL = 1e-3      # fp32 against float64 (the parity bound of the other model types)


def data(N, H, W, C, seed=0):
    """inputs in [-1, 1) and labels with 5 % ignored (255) pixels"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
    y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
    y[rng.uniform(size=y.shape) < 0.05] = 255
    return x, y


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-6, np.abs(b).max()))


def relu_derivs(m, ex, ops):
    """ReLU'(u) of every BatchNorm + ReLU as the HIP kernels evaluate u (PeleeNet has no other activation): handed to the
    float64 restatement so that elements within rounding distance of the kink take the branch the device took"""
    out = {}
    for bn in m.graph.bns:
        if bn.act == 0:
            continue
        assert bn.act == ops.ACT_RELU, bn.name
        sc = ex.gscale[bn.group.id][bn.offset:bn.offset + bn.C]
        sh = ex.gshift[bn.group.id][bn.offset:bn.offset + bn.C]
        out[bn.name] = (ops.affine_act(ex.view(bn.z), sc, sh, bn.act).cpu().numpy() > 0).astype(np.float64)
    return out


__all__ = ['PeleeOracle', 'torch_oracle', 'peleenet_body', 'avgpool2d_fwd', 'avgpool2d_bwd', 'O', 'TOL', 'data', 'rel',
           'relu_derivs']
