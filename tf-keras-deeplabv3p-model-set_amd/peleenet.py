"""DeepLabV3+ PeleeNet graphs: counterpart of the reference's deeplabv3p/models/deeplabv3p_peleenet.py (dense_graph :63-87,
dense_block_graph :90-94, stem_block_graph :97-113, basic_conv2d_graph :116-124, PeleeNet body :127-298 with its output-stride
table :247-253, Deeplabv3pPeleeNet :302-360, Deeplabv3pLitePeleeNet :363-423).  Every conv is a bias-free glorot_uniform
DeeplabConv2D followed by CustomBatchNormalization (Keras defaults eps 1e-3, momentum 0.99) and ReLU.

Buffers.  DenseNet growth maps onto the graph's Concatenate-as-channel-slices: each dense block owns ONE buffer
c_in + num_layers * 32 channels wide.  The block input sits in channels [0, c_in) -- written there by the stem3 conv, by a
transition conv, or by the transition's AveragePooling2D -- and the branch1b / branch2c convs of dense layer j write their raw
outputs into channels [c_in + 32 j, c_in + 32 j + 16) and [c_in + 32 j + 16, c_in + 32 (j + 1)).  Each of those slices keeps
its own BatchNorm + ReLU as the lazy prologue in the block's coefficient group; a pooled block input is already activated
(>= 0) and keeps identity coefficients, on which the ReLU of the group is a no-op.  Concatenate([x, branch1, branch2]) of
layer j is then the prefix [0, c_in + 32 (j + 1)) of the buffer: no copy.  The stem block's Concatenate([maxpool, stem2b])
is a 64-channel buffer in the same way.

Layer order.  model.layers and the weight order of save_weights / load_weights(by_name=False) come from
GraphBuilder.keras_layer_order, the restatement of Keras' functional-model ordering (decreasing depth, ties broken by a
depth-first walk from the output over each merge layer's inputs in list order).  The inputs recorded here are the
reference's call arguments as written: Concatenate([x, branch1, branch2]) (:85) and Concatenate([branch1, branch2]) of the
stem with branch1 the max pooling (:109).  branch1a / branch2a and branch1b / branch2b have identical weight shapes, so an
ordering mistake would swap weights silently on a positional load; the order has not been compared with the released
checkpoint's .h5 (no TensorFlow and no checkpoint here).

Input sizes.  MaxPooling2D(2, 2) of the stride-2 stem output floors, the 'same' stride-2 stem2b conv rounds up: for
ceil(H / 2) odd the two halves of the stem Concatenate differ in size and Keras cannot build the model (513: 128 against
129).  Such sizes raise ValueError here instead of being padded."""
from .graph import GraphBuilder, ACT_RELU, Value
from .layers import ASPP_block, ASPP_Lite_block, Decoder_block


def basic_conv2d(g, x, out_channels, kernel_size, stride, padding, name, out=None, group=None, goff=0):
    """basic_conv2d_graph (:116-124): conv (no bias) -> CustomBatchNormalization -> ReLU; `out` / `group`: write the raw conv
    output into a Concatenate slice whose BatchNorm owns channels [goff, goff + out_channels) of `group`"""
    x = g.conv2d(x, out_channels, kernel_size, name + '_conv', stride=stride, padding=padding, out=out)
    x = g.batchnorm(x, name + '_norm', group=group, goff=goff)
    return g.relu(x)


def _prefix(g, buf, group, C, inputs):
    """Concatenate(inputs) == channels [0, C) of the block buffer, activated by the slices' own BatchNorm + ReLU"""
    t = buf if C == buf.C else buf.slice(0, C, '%s[:%d]' % (buf.name, C))
    return g.concat_value(t, group, ACT_RELU, inputs)


def _input_view(buf, group, C, v):
    """the block input (channels [0, C) of the buffer) as the value its consumers read; `v`: its producer's output value"""
    return Value(buf.slice(0, C, '%s[:%d]' % (buf.name, C)), group, 0, ACT_RELU, None, klayer=v.klayer)


def dense_layer(g, x, buf, group, growth_rate, bottleneck_width, name):
    """dense_graph (:63-87): x is the buffer prefix [0, c); the two branches land in [c, c + growth_rate)"""
    growth_rate = int(growth_rate / 2)
    inter_channel = int(growth_rate * bottleneck_width / 4) * 4
    num_input_features = x.shape[2]
    if inter_channel > num_input_features / 2:
        inter_channel = int(num_input_features / 8) * 4
    c = num_input_features
    b1 = basic_conv2d(g, x, inter_channel, 1, 1, 'valid', name + '_branch1a')
    b1 = basic_conv2d(g, b1, growth_rate, 3, 1, 'same', name + '_branch1b', out=buf.slice(c, growth_rate), group=group, goff=c)
    b2 = basic_conv2d(g, x, inter_channel, 1, 1, 'valid', name + '_branch2a')
    b2 = basic_conv2d(g, b2, growth_rate, 3, 1, 'same', name + '_branch2b')
    b2 = basic_conv2d(g, b2, growth_rate, 3, 1, 'same', name + '_branch2c', out=buf.slice(c + growth_rate, growth_rate),
                      group=group, goff=c + growth_rate)
    return _prefix(g, buf, group, c + 2 * growth_rate, [x, b1, b2])


def stem_block(g, x, num_init_features, name):
    """stem_block_graph (:97-113); returns the stem2 concat value (stem3 is issued by the caller into the first block buffer)"""
    num_stem_features = int(num_init_features / 2)
    out = basic_conv2d(g, x, num_init_features, 3, 2, 'same', name + '_stem1')
    H, W, _ = out.shape
    base, slices, group = g.concat_buffer(H // 2, W // 2, [num_init_features, num_init_features], name + '_concat')
    branch2 = basic_conv2d(g, out, num_stem_features, 1, 1, 'valid', name + '_stem2a')
    branch2 = basic_conv2d(g, branch2, num_init_features, 3, 2, 'same', name + '_stem2b', out=slices[1][0], group=group,
                           goff=slices[1][1])
    branch1 = g.maxpool2d(out, 2, 2, (0, 0, 0, 0), out=slices[0][0])
    return g.concat_value(base, group, ACT_RELU, [branch1, branch2])


def check_input_size(H, W):
    for n, s in (('height', H), ('width', W)):
        h1 = -(-s // 2)
        if h1 % 2:
            raise ValueError('PeleeNet cannot take input %s %d: the stem block concatenates MaxPooling2D(2, 2) of the stride-2 stem '
                             '(%d rows) with a stride-2 \'same\' conv (%d rows); ceil(%s / 2) must be even'
                             % (n, s, h1 // 2, -(-h1 // 2), n))


def PeleeNet_body(g, input_tensor, OS, growth_rate=32, block_config=(3, 4, 8, 6), num_init_features=32,
                  bottleneck_width=(1, 2, 4, 4)):
    """PeleeNet(include_top=False, pooling=None) (:127-298): returns (features, skip, backbone_len)"""
    if OS not in (8, 16, 32):
        raise ValueError('invalid output stride', OS)
    H, W, _ = input_tensor.shape
    check_input_size(H, W)
    name = 'bbn_features'
    stem = stem_block(g, input_tensor, num_init_features, name + '_stemblock')
    h, w, _ = stem.shape
    num_features = num_init_features
    buf, _, group = g.concat_buffer(h, w, [num_features + block_config[0] * growth_rate], name + '_denseblock1_concat')
    v = basic_conv2d(g, stem, num_init_features, 1, 1, 'valid', name + '_stemblock_stem3', out=buf.slice(0, num_features),
                     group=group, goff=0)
    x = _input_view(buf, group, num_features, v)
    skip = None
    for i, num_layers in enumerate(block_config):
        for j in range(num_layers):
            x = dense_layer(g, x, buf, group, growth_rate, bottleneck_width[i], name + '_denseblock%d_denselayer%d' % (i + 1, j + 1))
        num_features = num_features + num_layers * growth_rate
        pool = (OS == 8 and i < 1) or (OS == 16 and i < 2) or (OS == 32 and i != len(block_config) - 1)
        last = i == len(block_config) - 1
        tname = name + '_transition%d' % (i + 1)
        if last or pool:
            t = basic_conv2d(g, x, num_features, 1, 1, 'valid', tname)
            if i == 0:
                skip = t                                   # stride-4 skip feature (:244-245)
            if last:
                x = t
                break
            h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
            buf, _, group = g.concat_buffer(h, w, [num_features + block_config[i + 1] * growth_rate],
                                            name + '_denseblock%d_concat' % (i + 2))
            v = g.avgpool2d(t, 2, 2, out=buf.slice(0, num_features))
        else:
            buf, _, group = g.concat_buffer(h, w, [num_features + block_config[i + 1] * growth_rate],
                                            name + '_denseblock%d_concat' % (i + 2))
            v = basic_conv2d(g, x, num_features, 1, 1, 'valid', tname, out=buf.slice(0, num_features), group=group, goff=0)
        x = _input_view(buf, group, num_features, v)
    return x, skip, len(g.layers)


def _check_weights(weights):
    if weights not in {'imagenet', None}:
        raise ValueError('The `weights` argument should be either `imagenet` (pre-trained on Imagenet) or '
                         '`None` (random initialization)')


def Deeplabv3pPeleeNet(input_shape=(512, 512, 3), weights=None, input_tensor=None, num_classes=21, OS=8, seed=0):
    """PeleeNet + ASPP + decoder; returns (graph, head_input, backbone_len) like the other builders"""
    _check_weights(weights)
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'deeplabv3p_peleenet', seed)
    x, skip_feature, backbone_len = PeleeNet_body(g, g.input, OS)
    g.tap('backbone_out', x)
    x = ASPP_block(g, x, OS)
    g.tap('aspp_out', x)
    x = Decoder_block(g, x, skip_feature)
    return g, x, backbone_len


def Deeplabv3pLitePeleeNet(input_shape=(512, 512, 3), weights=None, input_tensor=None, num_classes=21, OS=8, seed=0):
    """PeleeNet + ASPP-Lite, no decoder"""
    _check_weights(weights)
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'deeplabv3p_peleenet_lite', seed)
    x, _, backbone_len = PeleeNet_body(g, g.input, OS)
    g.tap('backbone_out', x)
    x = ASPP_Lite_block(g, x)
    return g, x, backbone_len
