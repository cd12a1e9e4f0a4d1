"""Float64 restatement of DeepLabV3+ GhostNet (reference deeplabv3p/models/deeplabv3p_ghostnet.py) for the tests: the body is
built from the oracle's primitive layers (oracle/np_net.py conv2d / dwconv2d / bn / act / concat / add / global_avgpool /
mul_bcast) on the same tape; the heads are the oracle's ASPP / ASPP-Lite / decoder blocks.  `GhostOracle` is the NumPy
restatement, `torch_oracle` the same graph on torch-CPU autograd (oracle/torch_net.py) -- an independent implementation of every
primitive and of reverse-mode differentiation to triangulate the NumPy one against.

Written out from the reference's code, not from the product's graph builder (ghostnet.py): the ghost modules here are real
Concatenate layers of two separately computed halves."""
import math

import numpy as np

from oracle import np_ops as O
from oracle.np_net import OracleModel, Var
from peleenet_oracle import TOL, data, rel, relu_derivs

GHOST_TYPES = ('ghostnet', 'ghostnet_lite')


def make_divisible(v, divisor, min_value=None):
    """_make_divisible (:67-74)"""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


# (k, t, c, SE, s, r) per stage (:204-285); s == -1: stride 1, downsample structure kept.  The three tables share everything but
# the strides / rates of stages 5 .. 8, written here as a function of the output stride.
def cfgs(OS):
    s5, r6 = {8: (-1, 2), 16: (2, 1), 32: (2, 1)}[OS]
    s7, r7, r8 = {8: (-1, 2, 4), 16: (-1, 1, 2), 32: (2, 1, 1)}[OS]
    return [
        [[3, 16, 16, 0, 1, 1]],
        [[3, 48, 24, 0, 2, 1]],
        [[3, 72, 24, 0, 1, 1]],
        [[5, 72, 40, 0.25, 2, 1]],
        [[5, 120, 40, 0.25, 1, 1]],
        [[3, 240, 80, 0, s5, 1]],
        [[3, 200, 80, 0, 1, r6], [3, 184, 80, 0, 1, r6], [3, 184, 80, 0, 1, r6], [3, 480, 112, 0.25, 1, r6],
         [3, 672, 112, 0.25, 1, r6]],
        [[5, 672, 160, 0.25, s7, r7]],
        [[5, 960, 160, 0, 1, r8], [5, 960, 160, 0.25, 1, r8], [5, 960, 160, 0, 1, r8], [5, 960, 160, 0.25, 1, r8]],
    ]


def _ghost_module(net, x, out_chs, act, name):
    """GhostModule (:135-153): primary 1x1 conv -> BN [-> ReLU], cheap 3x3 depthwise conv of it -> BN [-> ReLU], Concatenate"""
    init = int(math.ceil(out_chs / 2))
    x1 = net.conv2d(x, init, 1, name + '_primary_conv_0', padding='valid')
    x1 = net.bn(x1, name + '_primary_conv_1')
    if act:
        x1 = net.relu(x1)
    x2 = net.dwconv2d(x1, 3, name + '_cheap_operation_0', 1, 1, 'same')
    x2 = net.bn(x2, name + '_cheap_operation_1')
    if act:
        x2 = net.relu(x2)
    y = net.concat([x1, x2])
    assert y.v.shape[-1] == out_chs
    return y


def _se(net, x, name):
    """SqueezeExcite (:104-120)"""
    C = x.v.shape[-1]
    s = net.global_avgpool(x)
    s = net.conv2d(s, make_divisible(C * 0.25, 4), 1, name + '_conv_reduce', use_bias=True)
    s = net.relu(s)
    s = net.conv2d(s, C, 1, name + '_conv_expand', use_bias=True)
    s = net.act(s, O.ACT_HSIGMOID)
    return net.mul_bcast(x, s)


def _bottleneck(net, x_in, mid, out, k, stride, rate, keep, se_ratio, name):
    """GhostBottleneck (:156-201)"""
    x = _ghost_module(net, x_in, mid, True, name + '_ghost1')
    if stride > 1 or keep:
        x = net.dwconv2d(x, k, name + '_conv_dw', stride, rate, 'same')
        x = net.bn(x, name + '_bn_dw')
    if se_ratio:
        x = _se(net, x, name + '_se')
    x = _ghost_module(net, x, out, False, name + '_ghost2')
    if x_in.v.shape[-1] == out and stride == 1:
        sc = x_in
    else:
        sc = net.dwconv2d(x_in, k, name + '_shortcut_0', stride, rate, 'same')
        sc = net.bn(sc, name + '_shortcut_1')
        sc = net.conv2d(sc, out, 1, name + '_shortcut_2', padding='valid')
        sc = net.bn(sc, name + '_shortcut_3')
    return net.add(x, sc)


def ghostnet_body(net, x, OS):
    x = net.conv2d(x, 16, 3, 'conv_stem', stride=2, padding='same')
    x = net.relu(net.bn(x, 'bn1'))
    skip = None
    exp = None
    for i, stage in enumerate(cfgs(OS)):
        for j, (k, exp, c, se, s, r) in enumerate(stage):
            keep = s == -1
            x = _bottleneck(net, x, make_divisible(exp, 4), make_divisible(c, 4), k, 1 if keep else s, r, keep, se,
                            'blocks_%d_%d' % (i, j))
            if i == 2 and j == 0:
                skip = x
    x = net.conv2d(x, make_divisible(exp, 4), 1, 'blocks_9_0_conv', padding='valid')
    x = net.relu(net.bn(x, 'blocks_9_0_bn1'))
    return x, skip


class GhostOracle(OracleModel):
    """OracleModel (oracle/np_net.py) for the two GhostNet types: same head, parameters, freeze levels and train step"""

    def __init__(self, model_type, num_classes, input_shape, output_stride, dtype=np.float64, seed=0, freeze_level=0,
                 bn_moving_variance='biased'):
        if model_type not in GHOST_TYPES:
            raise ValueError('This model type is not supported now')
        self.model_type = model_type
        self.num_classes = num_classes
        self.H, self.W = input_shape
        self.OS = output_stride
        self.net = self.net_class(dtype, seed)
        self.net.bn_moving_variance = bn_moving_variance
        self.velocity = {}
        self.freeze_level = freeze_level
        self._forward_graph(np.zeros((1, 33, 33, 3), dtype=np.float64), 33, 33, training=False)
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
        f, skip = ghostnet_body(net, xin, self.OS)
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

    class GhostTorchOracle(GhostOracle, TorchModel):
        pass
    return GhostTorchOracle(*args, **kw)


__all__ = ['GhostOracle', 'torch_oracle', 'ghostnet_body', 'cfgs', 'make_divisible', 'GHOST_TYPES', 'O', 'TOL', 'data', 'rel',
           'relu_derivs']
