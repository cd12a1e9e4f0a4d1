"""The U-Net family (unet.py, model.get_unet_model) without a GPU: parameter counts against a table derived by hand from the
reference's layer list, names / shapes / order against the float64 restatement (tests/unet_oracle.py), l2 = 0 everywhere, the
.h5 round trip, the ValueErrors, the restatement's new tape ops and the whole restatement against torch, and the refusals of the
dl3p_deconv2x2_* entry points that need no device."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from unet_oracle import UNetOracle, torch_oracle, conv2d_transpose_fwd, conv2d_transpose_bwd, gpu_case

TYPES = ('unet_standard', 'unet_lite')

# unet/models/unet.py:28-72 written out: ('c', cin, cout) a 3x3 layer of the type (Conv2D / SeparableConv2D), ('t', cin, cout)
# a Conv2DTranspose(cout, 2, strides=2), ('h', cin) the Conv2D(num_classes, 1) classifier.  Every layer has a bias.
LAYERS = [('c', 3, 64), ('c', 64, 64), ('c', 64, 128), ('c', 128, 128), ('c', 128, 256), ('c', 256, 256), ('c', 256, 512),
          ('c', 512, 512), ('c', 512, 1024), ('c', 1024, 1024),
          ('t', 1024, 512), ('c', 1024, 512), ('c', 512, 512), ('t', 512, 256), ('c', 512, 256), ('c', 256, 256),
          ('t', 256, 128), ('c', 256, 128), ('c', 128, 128), ('t', 128, 64), ('c', 128, 64), ('c', 64, 64), ('c', 64, 2), ('h', 2)]
KNOWN = {('unet_standard', 21): 31032897, ('unet_standard', 2): 31032840, ('unet_lite', 21): 5983068, ('unet_lite', 2): 5983011}


def _count(mt, C):
    n = 0
    for kind, cin, *cout in LAYERS:
        if kind == 'c':
            n += (9 * cin * cout[0] if mt == 'unet_standard' else 9 * cin + cin * cout[0]) + cout[0]
        elif kind == 't':
            n += 4 * cin * cout[0] + cout[0]
        else:
            n += cin * C + C
    return n


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('C', [21, 2])
def test_parameter_counts(mt, C):
    assert _count(mt, C) == KNOWN[(mt, C)]
    m = load_pkg().get_unet_model(mt, C, (64, 48))
    assert m.count_params() == KNOWN[(mt, C)]
    assert sum(p.size for p in m.graph.all_params() if p.trainable) == KNOWN[(mt, C)]
    assert all(l.trainable for l in m.layers)
    assert not m.graph.bns


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('training', [True, False])
def test_names_shapes_and_order_match_restatement(mt, training):
    m = load_pkg().get_unet_model(mt, 21, (32, 48), training=training)
    o = UNetOracle(mt, 21, (32, 48))
    ps = m.graph.all_params()
    assert [p.name for p in ps] == o.net.order
    for p in ps:
        assert p.shape == o.net.params[p.name].shape, p.name
        assert p.l2 == 0.0 and o.net.l2[p.name] == 0.0, p.name              # plain Keras layers: no regulariser
    names = [l.name for l in m.layers]
    assert names == [l.name for l in m.graph.keras_layer_order(m.graph.output_layer)]
    assert names[0] == 'image_input' and names[-1] == 'pred_mask' and m.name == mt
    assert ('reshape' in names) == training and names.count('reshape') == int(training)
    conv = 'conv2d' if mt == 'unet_standard' else 'separable_conv2d'
    want = ([conv] + ['%s_%d' % (conv, i) for i in range(1, 19)] + ['conv2d_transpose'] + ['conv2d_transpose_%d' % i for i in (1, 2, 3)]
            + ['max_pooling2d'] + ['max_pooling2d_%d' % i for i in (1, 2, 3)] + ['dropout', 'dropout_1', 'concatenate']
            + ['concatenate_%d' % i for i in (1, 2, 3)] + ['conv2d_19' if mt == 'unet_standard' else 'conv2d', 'image_input', 'pred_mask']
            + (['reshape'] if training else []))
    assert sorted(names) == sorted(want)
    # a chain until the first skip: Keras' depth order is the creation order there
    assert names[1:5] == [conv, conv + '_1', 'max_pooling2d', conv + '_2']
    assert [l.name for l in m.get_layer('concatenate').inbound] == ['dropout', 'conv2d_transpose']            # [drop4, up6]
    assert [l.name for l in m.get_layer('concatenate_3').inbound] == [conv + '_1', 'conv2d_transpose_3']      # [conv1, up9]
    assert m.output_shape == ((None, 32 * 48, 21) if training else (None, 32, 48, 21))
    t = m.get_layer('conv2d_transpose')
    assert [p.key for p in t.params] == ['kernel', 'bias'] and t.params[0].shape == (2, 2, 512, 1024)
    assert t.output_shape == (4, 6, 512)
    if mt == 'unet_lite':
        s = m.get_layer('separable_conv2d')
        assert [p.key for p in s.params] == ['depthwise_kernel', 'pointwise_kernel', 'bias']
        assert [p.dev_shape for p in s.params] == [(3, 3, 4, 1), (1, 1, 4, 64), (64,)]           # the image padded to 4 channels
    last = m.get_layer(conv + '_18')
    assert last.output_shape == (32, 48, 2) and last.params[-1].shape == (2,) and last.params[-1].dev_shape == (4,)
    head = m.get_layer('conv2d_19' if mt == 'unet_standard' else 'conv2d')
    assert head.params[0].shape == (1, 1, 2, 21) and head.params[0].dev_shape == (1, 1, 4, 24)


@pytest.mark.parametrize('mt', TYPES)
def test_zero_copy_concatenation(mt):
    """the skip conv (drop4: its Dropout) and the transposed conv write the two slices of one buffer, skip first; no op copies"""
    g = load_pkg().get_unet_model(mt, 21, (32, 32)).graph
    ups = [op for op in g.ops if op.kind == 'conv_deconv']
    assert [(op.cin, op.cout) for op in ups] == [(1024, 512), (512, 256), (256, 128), (128, 64)]
    for op in ups:
        base = op.out.base
        assert base is not None and (op.out.c0, base.C) == (op.cout, 2 * op.cout)
        skip = [o for o in g.ops if getattr(o, 'out', None) is not None and o.out.base is base and o.out.c0 == 0]
        assert len(skip) == 1 and skip[0].kind == ('materialize' if op.cout == 512 else ('conv_dense' if mt == 'unet_standard' else 'conv_pw'))
    assert sum(1 for op in g.ops if op.kind == 'materialize') == 2                     # the two Dropout layers, nothing else


@pytest.mark.parametrize('mt', TYPES)
def test_h5_round_trip(mt, tmp_path):
    pkg = load_pkg()
    m = pkg.get_unet_model(mt, 21, (32, 32), seed=3)
    rng = np.random.default_rng(0)
    w = [rng.standard_normal(a.shape).astype(np.float32) for a in m.get_weights()]
    m.set_weights(w)
    p = str(tmp_path / 'w.h5')
    m.save_weights(p)
    m2 = pkg.get_unet_model(mt, 21, (32, 32), seed=4)
    m2.load_weights(p)
    for a, b in zip(w, m2.get_weights()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_initialisers():
    """he_normal with Keras' fans (the transposed kernel's from its stored shape: fan_in = 4 Cout), glorot_uniform for the
    classifier and the separable kernels, zero biases"""
    m = load_pkg().get_unet_model('unet_standard', 21, (32, 32), seed=1)
    k = m.get_layer('conv2d_transpose').params[0].value                   # (2, 2, 512, 1024)
    s = np.sqrt(2.0 / (4 * 512))
    assert abs(k.std() / s - 1) < 0.02 and np.abs(k).max() <= 2 * s / 0.87962566103423978 + 1e-6
    k = m.get_layer('conv2d_9').params[0].value                           # (3, 3, 1024, 1024)
    assert abs(k.std() / np.sqrt(2.0 / (9 * 1024)) - 1) < 0.02
    h = m.get_layer('conv2d_19').params[0].value
    assert np.abs(h).max() <= np.sqrt(6.0 / (2 + 21))
    assert all(not p.value.any() for p in m.graph.all_params() if p.key == 'bias')
    lite = load_pkg().get_unet_model('unet_lite', 21, (32, 32), seed=1)
    d, p, _ = [q.value for q in lite.get_layer('separable_conv2d_9').params]
    assert np.abs(d).max() <= np.sqrt(6.0 / (9 * 1024 + 9)) and np.abs(p).max() <= np.sqrt(6.0 / (1024 + 1024))
    assert np.abs(p).max() > 0.9 * np.sqrt(6.0 / 2048)


def test_value_errors():
    pkg = load_pkg()
    for shape in ((40, 32), (32, 40), (33, 33)):
        with pytest.raises(ValueError, match='multiples of 16'):
            pkg.get_unet_model('unet_lite', 21, shape)
    with pytest.raises(ValueError, match='Conv2DTranspose.*UpSampling2D.*MaxPooling2D'):
        pkg.get_unet_model('unet_simple', 21, (32, 32))
    with pytest.raises(ValueError, match='This model type is not supported now'):
        pkg.get_unet_model('unet_huge', 21, (32, 32))
    pkg.get_unet_model('unet_lite', 21, (32, 32), 2)                    # freeze_level: accepted, ignored
    import importlib
    shim = importlib.import_module('unet.model')
    assert shim.get_unet_model is pkg.get_unet_model and sorted(shim.unet_model_map) == ['unet_lite', 'unet_simple', 'unet_standard']


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('training', [True, False])
def test_mixed_bfloat16_is_refused_at_build_time(mt, training):
    pkg = load_pkg()
    mp = pkg.mixed_precision
    mp.set_policy(mp.Policy('mixed_bfloat16'))
    try:
        with pytest.raises(ValueError, match='mixed_bfloat16'):
            pkg.get_unet_model(mt, 21, (32, 32), training=training)
    finally:
        mp.set_policy(mp.Policy('float32'))
    pkg.get_unet_model(mt, 21, (32, 32), training=training)


@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 3, 5, 6, 4), (1, 1, 1, 3, 7)])
def test_tape_conv2d_transpose_against_torch(N, H, W, Cin, Cout):
    """forward and all three gradients of the restatement's op against torch.nn.functional.conv_transpose2d, to 1e-10"""
    rng = np.random.default_rng(N + H)
    x, w, b = rng.standard_normal((N, H, W, Cin)), rng.standard_normal((2, 2, Cout, Cin)), rng.standard_normal(Cout)
    gy = rng.standard_normal((N, 2 * H, 2 * W, Cout))
    tx = torch.tensor(x.transpose(0, 3, 1, 2), requires_grad=True)
    tw = torch.tensor(w, requires_grad=True)
    tb = torch.tensor(b, requires_grad=True)
    ty = torch.nn.functional.conv_transpose2d(tx, tw.permute(3, 2, 0, 1), tb, stride=2)
    ty.backward(torch.tensor(gy.transpose(0, 3, 1, 2)))
    assert np.abs(conv2d_transpose_fwd(x, w, b) - ty.detach().numpy().transpose(0, 2, 3, 1)).max() < 1e-10
    gx, gw, gb = conv2d_transpose_bwd(x, w, gy)
    assert np.abs(gx - tx.grad.numpy().transpose(0, 2, 3, 1)).max() < 1e-10
    assert np.abs(gw - tw.grad.numpy()).max() < 1e-10
    assert np.abs(gb - tb.grad.numpy()).max() < 1e-10


@pytest.fixture(scope='module', params=TYPES)
def case(request):
    """the GPU test's case (tests/test_unet_gpu.py: 2 x 32 x 32, 21 classes, the same seeds) on both restatements, once"""
    mt = request.param
    o, x, y, masks = gpu_case(mt, UNetOracle)
    t, _, _, _ = gpu_case(mt, torch_oracle)
    lo, _ = o.predict(x)
    lt, _ = t.predict(x)
    _, co, _ = o.loss_and_grads(x, y, masks)
    _, ct, _ = t.loss_and_grads(x, y, masks)
    return mt, o, t, lo, lt, co, ct


def test_restatement_matches_torch_autograd(case):
    """loss to 1e-11, every gradient to 1e-7 of its scale"""
    mt, o, t, lo, lt, co, ct = case
    assert list(o.net.order) == list(t.net.order)
    np.testing.assert_allclose(lo, lt, atol=1e-10, rtol=0)
    assert abs(co - ct) < 1e-11, (co, ct)
    for k in o.trainable_param_names():
        g = o.net.grads[k]
        assert np.abs(g - t.net.grads[k]).max() < 1e-7 * np.abs(g).max(), k


def test_no_reference_gradient_is_dead(case):
    """with the biases randomised the 2-channel ReLU bottleneck in front of the classifier is alive: every trainable parameter's
    reference gradient has max |g| > 1e-7, so no comparison of the GPU test falls back to its absolute branch (the dropout masks
    here are drawn on the host; the GPU test passes the device's across)"""
    mt, o = case[:2]
    names = o.trainable_param_names()
    assert len(names) == len(o.net.order)
    for k in names:
        assert np.abs(o.net.grads[k]).max() > 1e-7, k


# ---- the C entry points refuse what they do not serve before any launch (callable without a device, like the ABI test)
A = 1 << 20       # a 16-byte aligned stand-in for a device address: a refused call never dereferences it


def _lib():
    return load_pkg('_lib').lib()


@pytest.mark.parametrize('Cin,Cout', [(6, 8), (8, 6), (0, 4), (3, 64)])
def test_deconv_refuses_channels_that_are_no_multiple_of_4(Cin, Cout):
    L = _lib()
    Err = load_pkg('_lib').Dl3pError
    assert L.deconv2x2_supported(Cin, Cout) == 0 and L.deconv2x2_supported(8, 12) == 1
    with pytest.raises(Err, match='multiples of 4'):
        L.deconv2x2_fwd(A, 8, None, None, 0, A, None, A, 8, 1, 2, 2, Cin, Cout, None)
    with pytest.raises(Err, match='multiples of 4'):
        L.deconv2x2_bwd_data(A, 8, A, A, 8, 0, 1, 2, 2, Cin, Cout, None)
    with pytest.raises(Err, match='multiples of 4'):
        L.deconv2x2_bwd_weight(A, 8, None, None, 0, A, 8, A, None, A, 1 << 20, 1, 2, 2, Cin, Cout, None)
    assert L.deconv2x2_bwd_weight_workspace(1, 2, 2, Cin, Cout) == 0


def test_deconv_refuses_operands_of_4_gib():
    """8 x 512 x 512 up9 at batch 32: the 128-channel merge9 buffer (ldy = 128) is exactly 4 GiB -- refused; so is an input of
    4 GiB.  (One row less passes the guard; that call would launch, so it is not made here.)"""
    L = _lib()
    Err = load_pkg('_lib').Dl3pError
    N, H, W, Cin, Cout = 32, 256, 256, 128, 64
    assert 4 * N * H * W * 128 * 4 == 1 << 32
    with pytest.raises(Err, match='4 GiB'):
        L.deconv2x2_fwd(A, Cin, None, None, 0, A, None, A, 128, N, H, W, Cin, Cout, None)
    with pytest.raises(Err, match='4 GiB'):
        L.deconv2x2_bwd_data(A, 128, A, A, Cin, 0, N, H, W, Cin, Cout, None)
    with pytest.raises(Err, match='4 GiB'):
        L.deconv2x2_bwd_weight(A, Cin, None, None, 0, A, 128, A, None, A, 1 << 30, N, H, W, Cin, Cout, None)
    with pytest.raises(Err, match='4 GiB'):                                    # the input: 2^20 rows of 1024 floats
        L.deconv2x2_fwd(A, 1024, None, None, 0, A, None, A, 4, 16, 256, 256, 1024, 4, None)
