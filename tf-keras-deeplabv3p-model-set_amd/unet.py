"""The U-Net family (reference unet/models/unet.py, unet/model.py): unet_standard and unet_lite.

The same functional-API calls as the reference, recorded on a GraphBuilder:
  * every layer is conv + bias + ReLU with NO BatchNormalization: the conv output is stored raw and the ReLU is applied in each
    reader's prologue (GraphBuilder.activation's view route);
  * `concatenate([skip, up])` is not executed: the skip conv (or, for drop4, its Dropout) and the transposed conv write straight
    into the two channel slices of one buffer, skip first (GraphBuilder.concat_buffer_act);
  * Conv2DTranspose(filters, 2, strides=(2, 2)) is one GEMM with a scattering epilogue (csrc/deconv.hip);
  * plain Keras layers carry no regulariser: every parameter has l2 = 0;
  * the 2-channel ReLU bottleneck in front of the classifier is padded to 4 channels on the device, and unet_lite's first
    depthwise conv reads a 4-channel zero-padded copy of the image -- Keras-facing shapes stay the reference's and the pad
    weights stay exactly 0 (their gradients are: a pad activation is relu(0 w + 0) = 0).

unet_simple (unet.py:152-222) is not built: it needs three more operators.
"""
from .graph import GraphBuilder, ACT_RELU

UNET_TYPES = ('unet_standard', 'unet_lite')
UNET_SIMPLE_MISSING = ("3x3 stride-1 Conv2DTranspose", "UpSampling2D (nearest)", "'same' 3x3 stride-2 MaxPooling2D")
DEPTHS = (64, 128, 256, 512)


def _unet(g, conv):
    """the layer list both types share (unet.py:28-72 / :97-141); conv(x, filters, out=None, pad_to=None) is the type's 3x3 layer"""
    H, W, _ = g.input_shape
    x = g.input
    merges = []
    for i, f in enumerate(DEPTHS):                         # conv1 .. conv4 (+ drop4), pool1 .. pool4
        h, w = H >> i, W >> i
        base, (skip, up) = g.concat_buffer_act(h, w, [f, f], 'merge%d' % (9 - i), ACT_RELU)
        x = conv(x, f)
        if i < 3:
            x = conv(x, f, out=skip)
        else:
            x = conv(x, f)
            x = g.dropout(x, 0.5, out=skip)                # drop4 is materialised by its Dropout directly into its slice
        merges.append((base, up, x))
        x = g.maxpool2d(x, 2, 2, (0, 0, 0, 0))
    x = conv(x, 1024)
    x = conv(x, 1024)
    x = g.dropout(x, 0.5)                                  # drop5
    for i in (3, 2, 1, 0):                                 # up6 / merge6 / conv6 ... up9 / merge9 / conv9
        base, up, skip_v = merges[i]
        u = g.conv2d_transpose(x, DEPTHS[i], None, use_bias=True, out=up, activation=ACT_RELU)
        x = g.concat_act(base, [skip_v, u])
        x = conv(x, DEPTHS[i])
        x = conv(x, DEPTHS[i])
    x = conv(x, 2, pad_to=g.align)                         # Conv2D / SeparableConv2D(2, 3): 2 channels, 4 on the device
    return x


def UNetStandard(num_classes, input_shape=(512, 512, 3), input_tensor=None, weights=None, seed=0, **kwargs):
    """unet.py:14-79; returns (graph, the tensor in front of the classifier)"""
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'unet_standard', seed)

    def conv(x, f, out=None, pad_to=None):
        return g.conv2d(x, f, 3, None, use_bias=True, out=out, pad_to=pad_to, kernel_initializer='he_normal', l2=0.0,
                        activation=ACT_RELU)
    return g, _unet(g, conv)


def UNetLite(num_classes, input_shape=(512, 512, 3), input_tensor=None, weights=None, seed=0, **kwargs):
    """unet.py:83-148: every 3x3 Conv2D is a SeparableConv2D"""
    g = input_tensor if isinstance(input_tensor, GraphBuilder) else GraphBuilder(input_shape, 'unet_lite', seed)

    def conv(x, f, out=None, pad_to=None):
        if x.tensor.C % g.align:
            x = g.pad_channels(x, (x.tensor.C + g.align - 1) // g.align * g.align)     # the image: 3 -> 4 channels
        return g.separable_conv2d(x, f, None, activation=ACT_RELU, out=out, pad_to=pad_to)
    return g, _unet(g, conv)


def UNetSimple(*args, **kwargs):
    raise ValueError('unet_simple is not built: it needs ' + ', '.join(UNET_SIMPLE_MISSING))


unet_model_map = {
    'unet_standard': UNetStandard,
    'unet_lite': UNetLite,
    'unet_simple': UNetSimple,
}
