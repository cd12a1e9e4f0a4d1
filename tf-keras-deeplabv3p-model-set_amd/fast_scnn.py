"""The Fast-SCNN family (reference fast_scnn/models/fast_scnn.py:18-153, fast_scnn/model.py): the same functional-API calls recorded
on a GraphBuilder, layer by layer, with the Keras auto-names (one counter per layer class; explicit names DSConv1_classifier,
DSConv2_classifier, pred_mask).

What is NOT executed literally (exact identities):
  * UpSampling2D((4, 4)) -> DeeplabSeparableConv2D(dilation 4) -> BatchNorm -> ReLU -> DeeplabConv2D 1x1 runs on the H/32 map with
    dilation 1: nearest upsampling commutes with pointwise convs, bias, ReLU and training-mode BatchNorm (same batch mean and biased
    variance), and a dilation-r 3x3 'same' depthwise conv of an r-times replicated map is the replicated dilation-1 conv of the small
    one, borders included.  Its result meets the H/8 branch in ONE fused launch (GraphBuilder.upsample_add, csrc/nearest.hip) that
    also leaves the statistics of the BatchNorm behind the Add; backward block-sums the gradient once.
  * UpSampling2D((8, 8)) -> Reshape -> Softmax: the dl3p_nearest_* head evaluates one softmax per logit pixel and sums the loss
    gradient over the 8 x 8 labels of its block (csrc/nearest_head.hip).
  * Concatenate of the pyramid pooling block: its producers write into the channel slices of one buffer.
  * DeeplabDepthwiseConv2D's bias in front of a BatchNorm: z stays raw, the BatchNorm carries the bias (GraphBuilder.dwconv2d).
"""
from .graph import GraphBuilder, L2_FACTOR, ACT_NONE

FAST_SCNN_TYPES = ('fast_scnn',)
BIN_SIZES = (2, 4, 6, 8)
_BASE = {'Conv2D': 'conv2d', 'BatchNormalization': 'batch_normalization', 'ReLU': 're_lu', 'SeparableConv2D': 'separable_conv2d',
         'DepthwiseConv2D': 'depthwise_conv2d', 'Add': 'add', 'AveragePooling2D': 'average_pooling2d', 'Lambda': 'lambda',
         'Concatenate': 'concatenate', 'UpSampling2D': 'up_sampling2d', 'Dropout': 'dropout', 'Reshape': 'reshape'}


class _Names:
    """Keras auto-names: '<snake class name>' for the first layer of a class, '<...>_<i>' for the i-th after it"""

    def __init__(self):
        self.n = {}

    def __call__(self, kind):
        i = self.n.get(kind, 0)
        self.n[kind] = i + 1
        return _BASE[kind] if i == 0 else '%s_%d' % (_BASE[kind], i)


def FastSCNN(num_classes, input_shape=(2048, 1024, 3), input_tensor=None, weights=None, training=True, seed=0, **kwargs):
    """fast_scnn.py:86-153 -> (graph, the logits at H/8 behind the Dropout: the tensor the nearest head reads)"""
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'Fast_SCNN', seed)
    H, W, _ = g.input_shape
    nm = _Names()

    def bn_relu(x, relu=True, channels=None):
        prod = g.producer_of(x.tensor)
        x = g.batchnorm(x, nm('BatchNormalization'), channels=channels)
        prod.bias_bn = x.bn                 # a bias in front of a training-mode BatchNorm has no gradient but its l2 term
        return g.relu(x, nm('ReLU')) if relu else x

    def conv_block(x, conv_type, filters, k, stride, relu=True, pad_to=None):                      # :18-33
        if conv_type == 'ds':
            x = g.separable_conv2d(x, filters, nm('SeparableConv2D'), stride=stride, l2=L2_FACTOR)
        else:
            x = g.conv2d(x, filters, k, nm('Conv2D'), stride=stride, use_bias=True, pad_to=pad_to)
        return bn_relu(x, relu, channels=filters if pad_to else None)

    def res_bottleneck(x, filters, t, s, residual=False, out=None):                                # :36-52
        inputs = x
        y = conv_block(x, 'conv', x.shape[2] * t, 1, 1)
        y = g.dwconv2d(y, 3, nm('DepthwiseConv2D'), stride=s, use_bias=True)
        y = bn_relu(y)
        y = conv_block(y, 'conv', filters, 1, 1, relu=False)
        if not residual:
            return y
        layer = g.add_layer(nm('Add'), 'Add', y.shape, inbound=[y, inputs])
        return g.materialize(y, residual=inputs, name=layer.name, out=out).from_layer(layer)

    def bottleneck_block(x, filters, t, stride, n, out=None):                                      # :55-64
        x = res_bottleneck(x, filters, t, stride)
        for i in range(1, n):
            x = res_bottleneck(x, filters, t, 1, True, out=out if i == n - 1 else None)
        return x

    # Step 1: learning to downsample (:102-104)
    lds = conv_block(g.input, 'conv', 32, 3, 2)
    lds = conv_block(lds, 'ds', 48, 3, 2)
    lds = conv_block(lds, 'ds', 64, 3, 2)
    # Step 2: global feature extractor (:109-112); the last Add writes into the first slice of the pyramid's Concatenate
    h, w = H // 32, W // 32
    base, slices, group = g.concat_buffer(h, w, [128] * (1 + len(BIN_SIZES)), 'ppm_concat')
    gfe = bottleneck_block(lds, 64, 6, 2, 3)
    gfe = bottleneck_block(gfe, 96, 6, 2, 3)
    gfe = bottleneck_block(gfe, 128, 6, 1, 3, out=slices[0][0])
    branches = [gfe]
    for (sl, _), bin_size in zip(slices[1:], BIN_SIZES):                                           # :67-83
        x = g.winpool2d(gfe, h // bin_size, w // bin_size, nm('AveragePooling2D'))
        x = g.conv2d(x, 128, 3, nm('Conv2D'), stride=2, use_bias=True)
        branches.append(g.resize(x, h, w, nm('Lambda'), out=sl))
    gfe = g.concat_value(base, group, ACT_NONE, branches, nm('Concatenate'))
    # Step 3: feature fusion (:115-128), the upsampled branch at H/32
    ff1 = conv_block(lds, 'conv', 128, 1, 1, relu=False)
    ff2 = g.passthrough(gfe, 'UpSampling2D', (4 * h, 4 * w, gfe.shape[2]), nm('UpSampling2D'))
    ff2 = g.separable_conv2d(ff2, 128, nm('SeparableConv2D'), l2=L2_FACTOR)            # dilation (4, 4) at H/8 = 1 here
    ff2.klayer.dilation_rate = (4, 4)
    folded = [ff2.klayer]                   # layers that Keras sees at H/8: `layers` / `summary` report its shapes, not the device's
    sep = g.producer_of(ff2.tensor)
    ff2 = g.batchnorm(ff2, nm('BatchNormalization'))
    sep.bias_bn = ff2.bn
    # this BatchNorm sees 1/16 of the elements Keras' does: same mean and biased variance, but Bessel's factor of the 'unbiased'
    # moving variance wants the literal count (dl3p_bn_finalize_counts)
    ff2.bn.count_scale = 16
    folded.append(ff2.klayer)
    ff2 = g.relu(ff2, nm('ReLU'))
    folded.append(ff2.klayer)
    ff2 = g.conv2d(ff2, 128, 1, nm('Conv2D'), use_bias=True)
    folded.append(ff2.klayer)
    for layer in folded:
        layer.output_shape = (4 * h, 4 * w, 128)
    ff = g.upsample_add(ff1, ff2, 4, nm('Add'))
    ff = bn_relu(ff)
    g.producer_of(ff2.tensor).bias_bn = ff.bn       # ... through the Add as well: the BatchNorm behind it centres the sum
    # Step 4: classifier (:131-149)
    x = g.separable_conv2d(ff, 128, 'DSConv1_classifier', l2=L2_FACTOR)
    x = bn_relu(x)
    x = g.separable_conv2d(x, 128, 'DSConv2_classifier', l2=L2_FACTOR)
    x = bn_relu(x)
    cpad = (num_classes + g.align - 1) // g.align * g.align
    x = conv_block(x, 'conv', num_classes, 1, 1, relu=False, pad_to=cpad)
    x = g.dropout(x, 0.3, nm('Dropout'))
    g.head_upsample = 'nearest'
    return g, x


fast_scnn_model_map = {
    'fast_scnn': FastSCNN,
}
