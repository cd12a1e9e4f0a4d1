"""The nearest-upsampling entry points (csrc/nearest.hip, csrc/nearest_head.hip) without a device: the library exports every symbol
the header declares for them, and every entry point refuses the arguments it cannot serve with DL3P_EINVAL before anything is
launched (C % 4, a misaligned base, ld < C, r outside 1..8, H != r h, windows the map does not hold, more classes than a wave holds)."""
import ctypes
import subprocess

import pytest

from conftest import load_pkg

NEW = ('dl3p_upsample_add_fwd', 'dl3p_block_sum_bwd', 'dl3p_winpool2d_fwd', 'dl3p_winpool2d_bwd', 'dl3p_nearest_softmax_probs',
       'dl3p_nearest_head_train', 'dl3p_nearest_argmax_confusion', 'dl3p_nearest_class_counts', 'dl3p_bn_finalize_counts')
P = 1 << 20                # a 16-byte aligned address that no refused call reads


def test_header_declares_and_library_exports_the_entry_points():
    libm = load_pkg('_lib')
    protos = libm.parse_header()
    for name in NEW:
        ret, args = protos[name]
        assert ret == 'int' and args[-1] == 'void*', name
    out = subprocess.run(['nm', '-D', '--defined-only', libm.LIBPATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    assert set(NEW) <= exported, set(NEW) - exported


def _upadd(a=P, lda=8, asc=None, ash=None, b=P, ldb=8, bsc=None, bsh=None, out=P, ldo=8, part=None, N=2, h=3, w=5, C=8, H=6, W=10,
           r=2):
    rows = ctypes.c_int(0)
    return 'upsample_add_fwd', (a, lda, asc, ash, 0, b, ldb, bsc, bsh, 0, out, ldo, part, ctypes.byref(rows), N, h, w, C, H, W, r,
                                None)


def _bsum(g=P, ldg=8, gl=P, ldgl=8, N=2, h=3, w=5, C=8, H=6, W=10, r=2):
    return 'block_sum_bwd', (g, ldg, gl, ldgl, 0, N, h, w, C, H, W, r, None)


def _pfwd(x=P, ldx=8, sc=None, sh=None, y=P, ldy=8, N=2, H=9, W=10, C=8, kh=4, kw=5, Ho=2, Wo=2):
    return 'winpool2d_fwd', (x, ldx, sc, sh, 0, y, ldy, N, H, W, C, kh, kw, Ho, Wo, None)


def _pbwd(dy=P, lddy=8, gx=P, ldgx=8, N=2, H=9, W=10, C=8, kh=4, kw=5, Ho=2, Wo=2):
    return 'winpool2d_bwd', (dy, lddy, gx, ldgx, 0, N, H, W, C, kh, kw, Ho, Wo, None)


def _probs(z=P, ldz=24, probs=P, N=2, h=3, w=5, C=21, H=24, W=40):
    return 'nearest_softmax_probs', (z, ldz, probs, N, h, w, C, H, W, None)


def _train(z=P, ldz=24, labels=P, kind=0, cw=None, gz=P, ldgz=24, part=P, N=2, h=3, w=5, C=21, H=24, W=40):
    rows = ctypes.c_int(0)
    return 'nearest_head_train', (z, ldz, labels, 255, 1.0, kind, cw, 0.0, 0.0, None, gz, ldgz, 0, part, ctypes.byref(rows), N, h, w,
                                  C, H, W, None)


def _argmax(z=P, ldz=24, labels=P, pred=P, cm=P, N=2, h=3, w=5, C=21, H=24, W=40):
    return 'nearest_argmax_confusion', (z, ldz, labels, pred, cm, N, h, w, C, H, W, None)


def _counts(z=P, ldz=24, labels=P, counts=P, N=2, h=3, w=5, C=21, H=24, W=40):
    return 'nearest_class_counts', (z, ldz, labels, counts, N, h, w, C, H, W, None)


def _fin(part=P, rows=4, C=8, count=32.0, mcount=512.0, mm=P, mv=P, update=2):
    return 'bn_finalize_counts', (part, rows, None, C, count, mcount, P, P, 1e-3, 0.99, mm, mv, update, P, P, P, P, None)


BAD = [
    ('at least count', _fin(mcount=16.0)), ('at least count', _fin(count=0.0)), ('partial rows or sums', _fin(part=None)),
    ('moving stats', _fin(mm=None)),
    ('multiple of 4', _upadd(C=6)), ('aligned', _upadd(a=P + 4)), ('aligned', _upadd(b=P + 8)), ('aligned', _upadd(out=P + 12)),
    ('leading dimension', _upadd(lda=4)), ('leading dimension', _upadd(ldb=4)), ('leading dimension', _upadd(ldo=6)),
    ('outside 1..8', _upadd(r=0, H=0, W=0)), ('outside 1..8', _upadd(r=9, H=27, W=45)), ('is not r', _upadd(H=7)),
    ('is not r', _upadd(W=11)), ('null', _upadd(a=None)), ('come together', _upadd(asc=P)), ('come together', _upadd(bsh=P)),
    ('come together', _upadd(asc=P + 4, ash=P)), ('stat_partials', _upadd(part=P + 4)),
    ('multiple of 4', _bsum(C=2)), ('aligned', _bsum(g=P + 4)), ('aligned', _bsum(gl=P + 4)), ('leading dimension', _bsum(ldg=4)),
    ('leading dimension', _bsum(ldgl=7)), ('outside 1..8', _bsum(r=16, H=48, W=80)), ('is not r', _bsum(H=8)), ('null', _bsum(gl=None)),
    ('multiple of 4', _pfwd(C=5)), ('aligned', _pfwd(x=P + 4)), ('aligned', _pfwd(y=P + 4)), ('leading dimension', _pfwd(ldx=4)),
    ('leading dimension', _pfwd(ldy=4)), ('bad dims', _pfwd(Ho=3)), ('bad dims', _pfwd(kh=0)), ('bad dims', _pfwd(kh=10, Ho=0)),
    ('bad dims', _pfwd(H=258, W=129, kh=129, kw=129, Ho=2, Wo=1)), ('come together', _pfwd(sc=P)),
    ('multiple of 4', _pbwd(C=5)), ('aligned', _pbwd(dy=P + 4)), ('aligned', _pbwd(gx=P + 4)), ('leading dimension', _pbwd(lddy=4)),
    ('leading dimension', _pbwd(ldgx=4)), ('bad dims', _pbwd(Wo=1)), ('bad dims', _pbwd(kw=11, Wo=0)),
    ('aligned', _probs(z=P + 4)), ('unsupported', _probs(ldz=20)), ('unsupported', _probs(C=257, ldz=260)), ('unsupported', _probs(C=0)),
    ('must be r', _probs(H=25)), ('must be r', _probs(H=48)), ('must be r', _probs(H=27, W=45)), ('null', _probs(probs=None)),
    ('aligned', _train(z=P + 4)), ('aligned', _train(ldz=22)), ('unsupported', _train(ldz=20)), ('must be r', _train(W=41)), ('loss kind', _train(kind=3)),
    ('loss kind', _train(kind=1)), ('required', _train(labels=None)), ('required', _train(part=None)), ('gradient layout', _train(gz=P + 4)),
    ('gradient layout', _train(ldgz=20)),
    ('aligned', _argmax(z=P + 8)), ('unsupported', _argmax(ldz=20)), ('must be r', _argmax(H=23)), ('nothing to produce', _argmax(pred=None, cm=None)),
    ('needs labels', _argmax(labels=None)),
    ('aligned', _counts(z=P + 4)), ('unsupported', _counts(C=300, ldz=300)), ('must be r', _counts(W=80)), ('required', _counts(counts=None)),
    ('required', _counts(labels=None)),
]


@pytest.mark.parametrize('word,call', BAD, ids=['%s-%d' % (c[0], i) for i, (_, c) in enumerate(BAD)])
def test_entry_points_refuse_what_they_cannot_serve(word, call):
    libm = load_pkg('_lib')
    L = libm.lib()
    name, args = call
    fn = getattr(L, name)
    assert fn.raw(*args) == -1, (name, word)                          # DL3P_EINVAL, and nothing was launched
    with pytest.raises(libm.Dl3pError, match=word):
        fn(*args)


def test_the_small_window_pooling_entry_points_still_refuse_large_windows():
    """dl3p_avgpool2d_* keeps its k <= 3 contract: the large windows have their own entry points"""
    L = load_pkg('_lib').lib()
    assert L.avgpool2d_fwd.raw(P, 8, None, None, 0, P, 8, 1, 8, 8, 8, 4, 4, 2, 2, None) == -1
    assert L.avgpool2d_bwd.raw(P, 8, P, 8, 0, 1, 8, 8, 8, 4, 4, 2, 2, None) == -1


# ------------------------------------------------------------------------------------------------ the family, without a device
import importlib                                                      # noqa: E402

import numpy as np                                                    # noqa: E402

from fast_scnn_oracle import FastSCNNOracle, FastSCNNTorch, data as _data            # noqa: E402


def _layer_table(C):
    """(kind, cin, cout) of every layer with weights, written down from reference fast_scnn/models/fast_scnn.py:86-153"""
    t = [('conv3', 3, 32), ('bn', 32), ('sep', 32, 48), ('bn', 48), ('sep', 48, 64), ('bn', 64)]                 # :102-104
    for cin, cout in ((64, 64), (64, 64), (64, 64), (64, 96), (96, 96), (96, 96), (96, 128), (128, 128), (128, 128)):   # :109-111, t = 6
        t += [('conv1', cin, 6 * cin), ('bn', 6 * cin), ('dw', 6 * cin), ('bn', 6 * cin), ('conv1', 6 * cin, cout), ('bn', cout)]
    t += [('conv3', 128, 128)] * 4                                                                                  # :77, bins 2 4 6 8
    t += [('conv1', 64, 128), ('bn', 128), ('sep', 128 * 5, 128), ('bn', 128), ('conv1', 128, 128), ('bn', 128)]    # :115-127
    t += [('sep', 128, 128), ('bn', 128), ('sep', 128, 128), ('bn', 128), ('conv1', 128, C), ('bn', C)]             # :131-139
    return t


def _count(t):
    n = {'conv3': lambda i, o: 9 * i * o + o, 'conv1': lambda i, o: i * o + o, 'sep': lambda i, o: 9 * i + i * o + o,
         'dw': lambda c: 9 * c + c, 'bn': lambda c: 4 * c}
    return sum(n[e[0]](*e[1:]) for e in t)


@pytest.mark.parametrize('C', [2, 21, 150])
def test_parameter_count_against_the_layer_table(C):
    m = load_pkg().get_fast_scnn_model('fast_scnn', C, (256, 320))
    want = _count(_layer_table(C))
    assert sum(p.size for p in m.graph.all_params()) == want == FastSCNNOracle(C, (256, 320)).count_params()
    assert m.graph.count_params(False) == sum(2 * e[1] for e in _layer_table(C) if e[0] == 'bn')


@pytest.mark.parametrize('training', [True, False])
def test_names_order_and_shapes_match_the_restatement(training):
    C = 21
    m = load_pkg().get_fast_scnn_model('fast_scnn', C, (256, 256), training=training)
    o = FastSCNNOracle(C, (256, 256))
    with_weights = [(l.name, {p.key: p.shape for p in l.params}) for l in m.graph.layers if l.params]
    assert with_weights == [(name, ws) for name, _, ws in o.table]           # construction order, names, Keras shapes
    assert sorted(m.get_weights_by_name()) == sorted(o.params)
    names = [l.name for l in m.layers]
    assert names[0] == 'image_input' and names[-1] == 'pred_mask' and len(set(names)) == len(names)
    assert ('reshape' in names) == training and 'up_sampling2d' in names and 'up_sampling2d_1' in names
    for explicit in ('DSConv1_classifier', 'DSConv2_classifier', 'concatenate', 'dropout', 'add_6', 'lambda_3', 'average_pooling2d_3'):
        assert explicit in names, explicit
    # the layers computed in front of the folded UpSampling2D((4, 4)) report the shapes Keras gives them (H/8), like every other layer
    shapes = {l.name: tuple(l.output_shape) for l in m.layers if l.output_shape}
    for name in ('up_sampling2d', 'separable_conv2d_2', 'batch_normalization_31', 're_lu_21', 'conv2d_24', 'add_6', 'DSConv1_classifier'):
        assert shapes[name][:2] == (32, 32), (name, shapes[name])
    assert shapes['concatenate'] == (8, 8, 640) and shapes['up_sampling2d'] == (32, 32, 640) and shapes['conv2d_24'] == (32, 32, 128)
    assert shapes['dropout'][:2] == (32, 32) and shapes['up_sampling2d_1'] == (256, 256, C)
    # l2: DeeplabConv2D kernel and bias; the bias only of the separable and depthwise layers
    for p in m.graph.all_params():
        assert abs(p.l2 - o.l2_of(p.name)) < 1e-12, p.name


def test_value_errors_and_shim():
    pkg = load_pkg()
    with pytest.raises(ValueError, match='This model type is not supported now'):
        pkg.get_fast_scnn_model('fast_scnn_v2', 21, (256, 256))
    for C in (0, 254):
        with pytest.raises(ValueError, match='num_classes'):
            pkg.get_fast_scnn_model('fast_scnn', C, (256, 256))
    for shape in ((224, 256), (256, 224), (256, 300), (264, 256), (128, 128)):
        with pytest.raises(ValueError, match='pool_size'):
            pkg.get_fast_scnn_model('fast_scnn', 21, shape)
    with pytest.raises(ValueError, match='bn_moving_variance'):
        pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256), bn_moving_variance='other')
    assert pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256), bn_moving_variance='unbiased').bn_moving_variance == 'unbiased'
    shim = importlib.import_module('fast_scnn.model')
    assert shim.get_fast_scnn_model is pkg.get_fast_scnn_model and sorted(shim.fast_scnn_model_map) == ['fast_scnn']
    assert callable(shim.fast_scnn_model_map['fast_scnn'])


@pytest.mark.parametrize('training', [True, False])
def test_mixed_bfloat16_is_refused_at_build_time(training):
    pkg = load_pkg()
    mp = pkg.mixed_precision
    mp.set_policy(mp.Policy('mixed_bfloat16'))
    try:
        with pytest.raises(ValueError, match='mixed_bfloat16'):
            pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256), training=training)
    finally:
        mp.set_policy(mp.Policy('float32'))
    pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256), training=training)


@pytest.mark.parametrize('ext', ['h5', 'npz'])
def test_weight_file_round_trip(ext, tmp_path):
    pkg = load_pkg()
    m = pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256), seed=3)
    rng = np.random.default_rng(0)
    w = [rng.standard_normal(a.shape).astype(np.float32) for a in m.get_weights()]
    m.set_weights(w)
    p = str(tmp_path / ('w.' + ext))
    m.save_weights(p)
    m2 = pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256), seed=4)
    m2.load_weights(p)
    for a, b in zip(w, m2.get_weights()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('mv', ['biased', 'unbiased'])
def test_restatement_matches_its_torch_twin(mv):
    """the NumPy restatement (oracle.np_net) against the separately written torch-autograd one at 256 x 256, both literal: layer table,
    predict, the loss, EVERY gradient (with its l2 term) and, through one SGD step, every BatchNorm's moving statistics.  Two float64
    evaluations of the same arithmetic in different orders: 1e-9 relative"""
    C, N, H, W = 21, 1, 256, 256
    a, b = FastSCNNOracle(C, (H, W)), FastSCNNTorch(C, (H, W))
    assert [(n, k, dict(w)) for n, k, w in a.table] == [(n, k, dict(w)) for n, k, w in b.table]
    assert all(a.l2_of(k) == b.l2_of(k) and a.trainable(k) == b.trainable(k) for k in b.params)
    a.moving_variance = mv
    for o in (a, b):
        o.params = {k: v.copy() for k, v in b.params.items()}
    x, y = _data(N, H, W, C, seed=2)
    mask = (np.random.default_rng(1).uniform(size=(N, H // 8, W // 8, C)) >= 0.3).astype(np.float64)
    if mv == 'biased':
        pa, pb = a.predict(x), b.predict(x)
        assert pa.shape == pb.shape == (N, H, W, C) and np.abs(pa - pb).max() < 1e-9
    la, lb = a.loss_and_grads(x, y, mask), b.loss_and_grads(x, y, mask)
    assert abs(la - lb) < 1e-9 * abs(lb) and abs(lb - np.log(C)) < 0.5 * np.log(C)
    assert sorted(a.grads) == sorted(b.grads) == sorted(k for k in b.params if b.trainable(k))
    for k, gb in b.grads.items():
        scale = max(np.abs(gb).max(), 1e-12)
        assert np.abs(a.grads[k] - gb).max() < 1e-9 * scale + 1e-15, (k, np.abs(a.grads[k] - gb).max(), scale)
    a.sgd_step(0.01, 0.9, moving_variance=mv)
    b.sgd_step(0.01, 0.9, moving_variance=mv)
    for k, v in b.params.items():
        assert np.abs(a.params[k] - v).max() < 1e-9 * max(1.0, np.abs(v).max()), k
    # a bias in front of a training-mode BatchNorm: the l2 term alone
    w0 = FastSCNNTorch(C, (H, W)).params['depthwise_conv2d/bias']
    assert np.abs(b.grads['depthwise_conv2d/bias'] - 2 * 2e-5 * w0).max() < 1e-12
