"""DeepLabV3+ GhostNet graphs: counterpart of the reference's deeplabv3p/models/deeplabv3p_ghostnet.py (_make_divisible :67-74,
primary_conv :81-90, cheap_operations :93-101, SqueezeExcite :104-120, ConvBnAct :123-132, GhostModule :135-153,
GhostBottleneck :156-201, the output-stride tables :204-285, GhostNet body :287-489, Deeplabv3pGhostNet :493-551,
Deeplabv3pLiteGhostNet :555-613).  Every conv is a glorot_uniform DeeplabConv2D / DeeplabDepthwiseConv2D, every BatchNorm a
CustomBatchNormalization with the Keras defaults (eps 1e-3, momentum 0.99).

Buffers.  A ghost module owns ONE Concatenate buffer 2 c wide, c = ceil(out / 2) (every `out` of the tables is even, so the
reference's Concatenate is never sliced): the primary 1x1 conv writes its raw output z1 into channels [0, c), the cheap 3x3
depthwise conv reads act(BN1(z1)) lazily from that slice and writes its raw output z2 into [c, 2c).  Both BatchNorms own their
halves of the buffer's coefficient group, and Concatenate([x1, x2]) is the whole buffer read through that group (ReLU in
ghost1, no activation in ghost2): no copy.  With BatchNorm coefficients that are known before the launch (inference, frozen
backbone) the executor runs the pair as one fused launch (csrc/ghost_fwd.hip, Executor._find_ghost).

Alignment.  The half-widths c are 8, 12, 20, 24, 36, 40, 56, 60, 80, 92, 100, 120, 240, 336 and 480: multiples of 4 (the fp32
granule) but six of them not of 8, the granule of the bf16 kernels, so a slice [c, 2c) would start inside a 16-byte chunk there.
Under the mixed_bfloat16 policy both model types are therefore refused when they are built.

Input sizes.  Every stride-2 layer pads 'same' (ceil), the shortcut and main branch of a bottleneck use the same stride: every
size Keras can build is accepted (513 x 513 included)."""
import math

from .graph import GraphBuilder, ACT_NONE, ACT_RELU, ACT_HSIGMOID
from .layers import ASPP_block, ASPP_Lite_block, Decoder_block


def _make_divisible(v, divisor, min_value=None):
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    # Make sure that round down does not go down by more than 10%.
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


# k, t, c, SE, s, r   (s == -1: stride 1 but keep the downsample structure)
OS32_CFGS = [
    [[3, 16, 16, 0, 1, 1]],
    [[3, 48, 24, 0, 2, 1]],
    [[3, 72, 24, 0, 1, 1]],
    [[5, 72, 40, 0.25, 2, 1]],
    [[5, 120, 40, 0.25, 1, 1]],
    [[3, 240, 80, 0, 2, 1]],
    [[3, 200, 80, 0, 1, 1], [3, 184, 80, 0, 1, 1], [3, 184, 80, 0, 1, 1], [3, 480, 112, 0.25, 1, 1], [3, 672, 112, 0.25, 1, 1]],
    [[5, 672, 160, 0.25, 2, 1]],
    [[5, 960, 160, 0, 1, 1], [5, 960, 160, 0.25, 1, 1], [5, 960, 160, 0, 1, 1], [5, 960, 160, 0.25, 1, 1]],
]

OS16_CFGS = [
    [[3, 16, 16, 0, 1, 1]],
    [[3, 48, 24, 0, 2, 1]],
    [[3, 72, 24, 0, 1, 1]],
    [[5, 72, 40, 0.25, 2, 1]],
    [[5, 120, 40, 0.25, 1, 1]],
    [[3, 240, 80, 0, 2, 1]],
    [[3, 200, 80, 0, 1, 1], [3, 184, 80, 0, 1, 1], [3, 184, 80, 0, 1, 1], [3, 480, 112, 0.25, 1, 1], [3, 672, 112, 0.25, 1, 1]],
    [[5, 672, 160, 0.25, -1, 1]],
    [[5, 960, 160, 0, 1, 2], [5, 960, 160, 0.25, 1, 2], [5, 960, 160, 0, 1, 2], [5, 960, 160, 0.25, 1, 2]],
]

OS8_CFGS = [
    [[3, 16, 16, 0, 1, 1]],
    [[3, 48, 24, 0, 2, 1]],
    [[3, 72, 24, 0, 1, 1]],
    [[5, 72, 40, 0.25, 2, 1]],
    [[5, 120, 40, 0.25, 1, 1]],
    [[3, 240, 80, 0, -1, 1]],
    [[3, 200, 80, 0, 1, 2], [3, 184, 80, 0, 1, 2], [3, 184, 80, 0, 1, 2], [3, 480, 112, 0.25, 1, 2], [3, 672, 112, 0.25, 1, 2]],
    [[5, 672, 160, 0.25, -1, 2]],
    [[5, 960, 160, 0, 1, 4], [5, 960, 160, 0.25, 1, 4], [5, 960, 160, 0, 1, 4], [5, 960, 160, 0.25, 1, 4]],
]


def GhostModule(g, x, output_chs, act, name, ratio=2, dw_size=3):
    """GhostModule (:135-153) with kernel_size 1, stride 1: primary_conv (:81-90) and cheap_operations (:93-101) write the two
    halves of one buffer"""
    init_channels = int(math.ceil(output_chs / ratio))
    new_channels = int(init_channels * (ratio - 1))
    assert init_channels + new_channels == output_chs, 'an odd ghost width would need the Concatenate sliced'
    if init_channels % g.align:
        raise ValueError('GhostNet is not built under the mixed_bfloat16 policy: the ghost module %s is a Concatenate of two '
                         '%d-channel halves, and the bf16 kernels need every channel slice to start on a multiple of %d channels '
                         '(CHANNEL_ALIGN); build it under the float32 policy' % (name, init_channels, g.align))
    H, W, _ = x.shape
    base, slices, group = g.concat_buffer(H, W, [init_channels, new_channels], name + '_concat')
    a = ACT_RELU if act else ACT_NONE
    pname, cname = name + '_primary_conv', name + '_cheap_operation'
    x1 = g.conv2d(x, init_channels, 1, pname + '_0', stride=1, padding='valid', out=slices[0][0])
    x1 = g.batchnorm(x1, pname + '_1', group=group, goff=slices[0][1])
    if act:
        x1 = g.relu(x1, pname + '_relu')
    x2 = g.dwconv2d(x1, dw_size, cname + '_0', stride=1, padding='same', out=slices[1][0])
    x2 = g.batchnorm(x2, cname + '_1', group=group, goff=slices[1][1])
    if act:
        x2 = g.relu(x2, cname + '_relu')
    return g.concat_value(base, group, a, [x1, x2], name + '_concat')


def SqueezeExcite(g, input_x, name, se_ratio=0.25, divisor=4):
    """SqueezeExcite (:104-120): hard-sigmoid gate, both convs with bias"""
    C = input_x.shape[2]
    reduce_chs = _make_divisible(C * se_ratio, divisor)
    x = g.global_avgpool(input_x, name + '_avg_pool2d', kind='GlobalAveragePooling2D')
    x = g.passthrough(x, 'Reshape', (1, 1, C))
    x = g.conv2d(x, reduce_chs, 1, name + '_conv_reduce', use_bias=True)
    x = g.relu(x, name + '_act')
    x = g.conv2d(x, C, 1, name + '_conv_expand', use_bias=True)
    x = g.activation(x, ACT_HSIGMOID, name + '_hard_sigmoid', kind='Activation')
    return g.se_multiply(input_x, x)


def ConvBnAct(g, x, out_chs, kernel_size, name):
    """ConvBnAct (:123-132)"""
    x = g.conv2d(x, out_chs, kernel_size, name + '_conv', stride=1, padding='valid')
    x = g.batchnorm(x, name + '_bn1')
    return g.relu(x, name + '_relu')


def GhostBottleneck(g, input_x, mid_chs, out_chs, dw_kernel_size, stride, rate, keep, se_ratio, name):
    """GhostBottleneck (:156-201)"""
    has_se = se_ratio is not None and se_ratio > 0.
    x = GhostModule(g, input_x, mid_chs, True, name + '_ghost1')
    if stride > 1 or keep:
        x = g.dwconv2d(x, dw_kernel_size, name + '_conv_dw', stride=stride, rate=rate, padding='same')
        x = g.batchnorm(x, name + '_bn_dw')
    if has_se:
        x = SqueezeExcite(g, x, name + '_se', se_ratio=se_ratio)
    x = GhostModule(g, x, out_chs, False, name + '_ghost2')
    if input_x.shape[2] == out_chs and stride == 1:
        sc = input_x
    else:
        name1 = name + '_shortcut'
        sc = g.dwconv2d(input_x, dw_kernel_size, name1 + '_0', stride=stride, rate=rate, padding='same')
        sc = g.batchnorm(sc, name1 + '_1')
        sc = g.conv2d(sc, out_chs, 1, name1 + '_2', stride=1, padding='valid')
        sc = g.batchnorm(sc, name1 + '_3')
    return g.add(sc, x, name + '_add', keras_inputs=[x, sc])         # Add([x, sc]) (:200)


def GhostNet_body(g, input_tensor, OS, width=1.0):
    """GhostNet(include_top=False, pooling=None) (:287-489): returns (final feature, skip feature, backbone_len)"""
    if OS == 8:
        cfgs = OS8_CFGS
    elif OS == 16:
        cfgs = OS16_CFGS
    elif OS == 32:
        cfgs = OS32_CFGS
    else:
        raise ValueError('invalid output stride', OS)
    output_channel = int(_make_divisible(16 * width, 4))
    x = g.conv2d(input_tensor, output_channel, 3, 'conv_stem', stride=2, padding='same')
    x = g.batchnorm(x, 'bn1')
    x = g.relu(x, 'Conv2D_1_act')
    skip = None
    exp_size = None
    for index, cfg in enumerate(cfgs):
        sub_index = 0
        for k, exp_size, c, se_ratio, s, r in cfg:
            keep = s == -1
            if keep:
                s = 1
            output_channel = int(_make_divisible(c * width, 4))
            hidden_channel = int(_make_divisible(exp_size * width, 4))
            x = GhostBottleneck(g, x, hidden_channel, output_channel, k, s, r, keep, se_ratio,
                                'blocks_' + str(index) + '_' + str(sub_index))
            sub_index += 1
            if index == 2 and sub_index == 1:
                skip = x                                 # stride-4 skip feature (:417-419)
    output_channel = _make_divisible(exp_size * width, 4)
    x = ConvBnAct(g, x, output_channel, 1, 'blocks_9_0')
    return x, skip, len(g.layers)


def _check_weights(weights):
    if weights not in {'imagenet', None}:
        raise ValueError('The `weights` argument should be either `imagenet` (pre-trained on Imagenet) or '
                         '`None` (random initialization)')


def Deeplabv3pGhostNet(input_shape=(512, 512, 3), weights=None, input_tensor=None, num_classes=21, OS=8, seed=0):
    """GhostNet + ASPP + decoder; returns (graph, head_input, backbone_len) like the other builders"""
    _check_weights(weights)
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'deeplabv3p_ghostnet', seed)
    x, skip_feature, backbone_len = GhostNet_body(g, g.input, OS)
    g.tap('backbone_out', x)
    x = ASPP_block(g, x, OS)
    g.tap('aspp_out', x)
    x = Decoder_block(g, x, skip_feature)
    return g, x, backbone_len


def Deeplabv3pLiteGhostNet(input_shape=(512, 512, 3), weights=None, input_tensor=None, num_classes=21, OS=8, seed=0):
    """GhostNet + ASPP-Lite, no decoder"""
    _check_weights(weights)
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'deeplabv3p_ghostnet_lite', seed)
    x, _, backbone_len = GhostNet_body(g, g.input, OS)
    g.tap('backbone_out', x)
    x = ASPP_Lite_block(g, x)
    return g, x, backbone_len
