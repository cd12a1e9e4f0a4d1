"""The model front end without a device (models build on the CPU): the one input rule as a table, which of two broken factory
arguments is reported, the names model.py has always exported, the factory record with the model_config save() writes from it, and
that compile() adds no attribute.  Every expected string below was recorded from the tree before the front end was restructured."""
import contextlib
import io

import numpy as np
import pytest

from conftest import load_pkg


# ------------------------------------------------------------------------------------------------ the input rule
def _readonly():
    a = np.zeros((1, 2, 2, 3), np.float32)
    a.flags.writeable = False
    return a


def _strided():
    return np.zeros((1, 4, 4, 3), np.float32)[:, ::2]


# input -> (dtype of the result, the result IS the input, C-contiguous): what predict, predict_mask, evaluate, evaluate_miou (both
# protocols, for the labels) and DeepLab.predict each spelled out as `np.asarray(a)`, kept if uint8, else astype(float32, copy=False)
RULE = [('host uint8', lambda: np.zeros((1, 2, 2, 3), np.uint8), np.uint8, True, True),
        ('host float32', lambda: np.zeros((1, 2, 2, 3), np.float32), np.float32, True, True),
        ('host float64', lambda: np.zeros((1, 2, 2, 3), np.float64), np.float32, False, True),
        ('host int64 labels', lambda: np.arange(4, dtype=np.int64).reshape(1, 4, 1), np.float32, False, True),
        ('read-only float32', _readonly, np.float32, True, True),
        ('read-only uint8', lambda: np.frombuffer(bytes(12), np.uint8).reshape(1, 2, 2, 3), np.uint8, True, True),
        ('strided float32', _strided, np.float32, True, False)]


@pytest.mark.parametrize('what,make,dtype,same,contiguous', RULE, ids=[r[0].replace(' ', '_') for r in RULE])
def test_input_rule(what, make, dtype, same, contiguous):
    batch_input = load_pkg('model').batch_input
    a = make()
    out = batch_input(a)
    assert isinstance(out, np.ndarray) and out.dtype == dtype
    assert (out is a) == same
    assert out.flags.c_contiguous == contiguous
    assert out.flags.writeable == a.flags.writeable or not same
    assert np.array_equal(out, a)
    assert batch_input(out) is out                                  # (applying the rule again changes nothing)


def test_input_rule_takes_lists_like_asarray():
    out = load_pkg('model').batch_input([[1, 2], [3, 4]])
    assert out.dtype == np.float32 and out.tolist() == [[1.0, 2.0], [3.0, 4.0]]


# ------------------------------------------------------------------------------------------------ refusal precedence
NOT_SUPPORTED = 'This model type is not supported now'
SUBPIXEL = 'Subpixel head is experimental in the reference (README TODO) and not on the hot path'
CLASSES = 'num_classes must be in [1, 253] (got %d)'
BN = "bn_moving_variance must be 'biased' or 'unbiased' (got 'x')"
UNET_SIMPLE = "unet_simple is not built: it needs 3x3 stride-1 Conv2DTranspose, UpSampling2D (nearest), 'same' 3x3 stride-2 MaxPooling2D"
UNET_SHAPE = 'U-Net input height and width must be multiples of 16 (got %s)'
FS_SHAPE = ('Fast-SCNN input height and width must be multiples of 32 and at least 256: the pyramid pooling block pools with '
            'pool_size = (H/32)//8, which Keras cannot build for smaller inputs (got %s)')
BF16_TRAINING = "mixed_bfloat16 training is not built for model type 'mobilenetv2_lite' (test entry); build it under the float32 policy"
BF16_UNET = ("model type 'unet_lite' is not built for the mixed_bfloat16 policy (dl3p_deconv2x2_* has no bf16 kernels); build it under "
             "the float32 policy")
BF16_FS = ("model type 'fast_scnn' is not built for the mixed_bfloat16 policy (the nearest-upsampling and window-pooling kernels have "
           "no bf16 twins); build it under the float32 policy")

# (factory, keywords [, 'bf16': build under the mixed_bfloat16 policy], the ValueError's text or None for a model that builds).  The
# DeepLab types all have bf16 training kernels, so their refusal is reached with a test entry in _NO_BF16_TRAINING, as
# test_topology_and_abi.py does.
DL = dict(model_type='mobilenetv2_lite', num_classes=21, model_input_shape=(65, 65), output_stride=16)
UN = dict(model_type='unet_lite', num_classes=4, model_input_shape=(32, 32))
FS = dict(model_type='fast_scnn', num_classes=4, model_input_shape=(256, 256))
REFUSALS = [
    ('get_deeplabv3p_model', dict(DL, model_type='nope', num_classes=0), NOT_SUPPORTED),
    ('get_deeplabv3p_model', dict(DL, model_type='nope', use_subpixel=True), NOT_SUPPORTED),
    ('get_deeplabv3p_model', dict(DL, num_classes=0, use_subpixel=True), SUBPIXEL),
    ('get_deeplabv3p_model', dict(DL, num_classes=0, model_input_shape=(65,)), CLASSES % 0),
    ('get_deeplabv3p_model', dict(DL, num_classes=254), CLASSES % 254),
    ('get_deeplabv3p_model', dict(DL, model_type='nope', bn_moving_variance='x'), BN),
    ('get_deeplabv3p_model', dict(DL, num_classes=0, bn_moving_variance='x'), BN),
    ('get_deeplabv3p_model', dict(DL, model_input_shape=(65,), bn_moving_variance='x'), BN),
    ('get_deeplabv3p_model', dict(DL, use_subpixel=True, bn_moving_variance='x'), BN),
    ('get_deeplabv3p_model', dict(DL, bf16=True, training=True), BF16_TRAINING),
    ('get_deeplabv3p_model', dict(DL, bf16=True, training=False), None),
    ('get_deeplabv3p_model', dict(DL, bf16=True, training=True, num_classes=0), CLASSES % 0),
    ('get_deeplabv3p_model', dict(DL, bf16=True, training=True, bn_moving_variance='x'), BN),
    ('get_unet_model', dict(UN, model_type='nope', num_classes=0), NOT_SUPPORTED),
    ('get_unet_model', dict(UN, model_type='unet_simple', num_classes=0), UNET_SIMPLE),
    ('get_unet_model', dict(UN, num_classes=0, model_input_shape=(30, 30)), CLASSES % 0),
    ('get_unet_model', dict(UN, num_classes=254), CLASSES % 254),
    ('get_unet_model', dict(UN, model_input_shape=(30, 32)), UNET_SHAPE % '(30, 32)'),
    ('get_unet_model', dict(UN, bf16=True, training=True), BF16_UNET),
    ('get_unet_model', dict(UN, bf16=True, training=False), BF16_UNET),
    ('get_unet_model', dict(UN, bf16=True, training=True, num_classes=0), CLASSES % 0),
    ('get_unet_model', dict(UN, bf16=True, training=False, model_input_shape=(30, 30)), UNET_SHAPE % '(30, 30)'),
    ('get_fast_scnn_model', dict(FS, model_type='nope', num_classes=0), NOT_SUPPORTED),
    ('get_fast_scnn_model', dict(FS, num_classes=0, model_input_shape=(100, 100)), CLASSES % 0),
    ('get_fast_scnn_model', dict(FS, num_classes=254), CLASSES % 254),
    ('get_fast_scnn_model', dict(FS, model_type='nope', bn_moving_variance='x'), NOT_SUPPORTED),
    ('get_fast_scnn_model', dict(FS, num_classes=0, bn_moving_variance='x'), CLASSES % 0),
    ('get_fast_scnn_model', dict(FS, model_input_shape=(100, 100), bn_moving_variance='x'), BN),
    ('get_fast_scnn_model', dict(FS, model_input_shape=(288, 250)), FS_SHAPE % '(288, 250)'),
    ('get_fast_scnn_model', dict(FS, bf16=True, training=True), BF16_FS),
    ('get_fast_scnn_model', dict(FS, bf16=True, training=False), BF16_FS),
    ('get_fast_scnn_model', dict(FS, bf16=True, training=True, bn_moving_variance='x'), BN),
    ('get_fast_scnn_model', dict(FS, bf16=True, training=False, model_input_shape=(100, 100)), FS_SHAPE % '(100, 100)'),
]


@pytest.mark.parametrize('factory,kw,text', REFUSALS, ids=['%s-%d' % (r[0][4:-6], i) for i, r in enumerate(REFUSALS)])
def test_refusal_precedence(factory, kw, text):
    model_mod, mixed_precision = load_pkg('model'), load_pkg('mixed_precision')
    kw = dict(kw)
    bf16 = kw.pop('bf16', False)
    policy = mixed_precision._GLOBAL
    mixed_precision._GLOBAL = 'mixed_bfloat16' if bf16 else 'float32'
    if bf16 and factory == 'get_deeplabv3p_model':
        model_mod._NO_BF16_TRAINING['mobilenetv2_lite'] = 'test entry'
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            if text is None:
                assert getattr(model_mod, factory)(**kw).bf16
            else:
                with pytest.raises(ValueError) as e:
                    getattr(model_mod, factory)(**kw)
                assert type(e.value) is ValueError and str(e.value) == text
    finally:
        mixed_precision._GLOBAL = policy
        model_mod._NO_BF16_TRAINING.pop('mobilenetv2_lite', None)


# ------------------------------------------------------------------------------------------------ names
# what `from <package>.model import ...` could name before optimizers.py, losses.py, feed.py and callbacks.py existed, without the
# private functions that were evaluation code outside the class and are methods of DeeplabModel now
MOVED = {'optimizers': ['Adam', 'Lookahead', 'MovingAverage', 'RMSprop', 'SGD', 'SWA', '_AveragedOptimizer', '_clip_args',
                        'get_averaged_optimizer', 'get_optimizer'],
         'losses': ['Jaccard', 'SparseCategoricalCrossEntropy', 'SparseSoftmaxFocalLoss', 'WeightedSparseCategoricalCrossEntropy',
                    '_wants_jaccard', 'jaccard_from_counts', 'loss_spec', 'miou_from_confusion'],
         'feed': ['BatchFeeder', 'DistContext', 'LateScalar', 'StagedBatch'],
         'callbacks': ['AverageModelCheckpoint', 'EvalCallBack']}
STAYED = ['ACT_NONE', 'DeeplabModel', 'Deeplabv3pLiteMobileNetV2', 'Deeplabv3pMobileNetV2', '_NO_BF16_TRAINING', '_build_model',
          '_on_device_u8', '_register_optional', 'deeplab_model_map', 'get_deeplabv3p_model', 'get_fast_scnn_model', 'get_unet_model',
          'np', 'os', 'partial', 'sys', 'time', 'tta_size']


def test_every_name_is_still_importable_from_model():
    model_mod = load_pkg('model')
    for name in STAYED:
        assert hasattr(model_mod, name), name
    for sub, names in MOVED.items():
        mod = load_pkg(sub)
        for name in names:
            assert getattr(model_mod, name) is getattr(mod, name), name
            assert getattr(mod, name).__module__ == mod.__name__, name
    pkg = load_pkg()
    for name in pkg.__all__:
        if hasattr(model_mod, name):
            assert getattr(pkg, name) is getattr(model_mod, name), name


def test_evaluation_is_defined_in_the_class_body():
    model_mod = load_pkg('model')
    for name in ('evaluate', 'evaluate_miou', 'predict_tta', '_tta_siblings', 'class_ids', 'predict_mask'):
        fn = model_mod.DeeplabModel.__dict__[name]
        assert fn.__qualname__ == 'DeeplabModel.' + name, fn.__qualname__


# ------------------------------------------------------------------------------------------------ the factory record
CONFIG = ('{"class_name": "DeeplabV3p", "config": {"name": "%s", "factory": {"model_type": "%s", "num_classes": %d, '
          '"model_input_shape": [%d, %d], "output_stride": null, "training": %s, "bn_moving_variance": "%s"}}}')


@pytest.fixture(scope='module')
def families():
    model_mod = load_pkg('model')
    with contextlib.redirect_stdout(io.StringIO()):
        return {'deeplab': model_mod.get_deeplabv3p_model('mobilenetv2_lite', 21, (65, 65), 16, training=False,
                                                          bn_moving_variance='unbiased'),
                'deeplab_train': model_mod.get_deeplabv3p_model('mobilenetv2_lite', 5, (65, 65), 8, training=True),
                'unet': model_mod.get_unet_model('unet_lite', 4, (32, 32), training=False),
                'fast_scnn': model_mod.get_fast_scnn_model('fast_scnn', 4, (256, 256), training=True, bn_moving_variance='unbiased')}


RECORDS = {'deeplab': ({'family': 'deeplabv3p', 'model_type': 'mobilenetv2_lite', 'output_stride': 16, 'bn_moving_variance': 'unbiased'},
                       CONFIG % ('deeplabv3p_mobilenetv2_lite', 'mobilenetv2_lite', 21, 65, 65, 'false', 'unbiased')),
           'deeplab_train': ({'family': 'deeplabv3p', 'model_type': 'mobilenetv2_lite', 'output_stride': 8, 'bn_moving_variance': 'biased'},
                             CONFIG % ('deeplabv3p_mobilenetv2_lite', 'mobilenetv2_lite', 5, 65, 65, 'true', 'biased')),
           'unet': ({'family': 'unet', 'model_type': 'unet_lite', 'output_stride': None, 'bn_moving_variance': 'biased'},
                    CONFIG % ('unet_lite', 'unet_lite', 4, 32, 32, 'false', 'biased')),
           'fast_scnn': ({'family': 'fast_scnn', 'model_type': 'fast_scnn', 'output_stride': None, 'bn_moving_variance': 'unbiased'},
                         CONFIG % ('Fast_SCNN', 'fast_scnn', 4, 256, 256, 'true', 'unbiased'))}


@pytest.mark.parametrize('which', sorted(RECORDS))
def test_factory_record_and_model_config(which, families, tmp_path):
    m = families[which]
    record, config = RECORDS[which]
    assert m.factory == record
    assert m.bn_moving_variance == m.graph.bn_moving_variance == record['bn_moving_variance']
    path = str(tmp_path / 'model.h5')
    m.save(path)
    got = load_pkg('h5io').read_keras_h5(path)[1]['model_config']
    assert (got.decode() if isinstance(got, bytes) else got) == config


# ------------------------------------------------------------------------------------------------ explicit state
STATE = {'metrics', '_jaccard', 'sample_weight_mode', '_feed', '_late_loss', '_last_train_ex', 'last_metrics', 'last_val_metrics',
         'bn_moving_variance', '_tta_cache', 'factory'}


@pytest.mark.parametrize('which', sorted(RECORDS))
def test_compile_adds_no_attribute(which, families):
    pkg = load_pkg()
    m = families[which]
    before = set(vars(m))
    assert STATE <= before
    assert (m.metrics, m._jaccard, m.sample_weight_mode, m._feed, m._late_loss, m._last_train_ex) == (None, False, None, None, None, None)
    assert m.last_metrics == {} and m.last_val_metrics == {} and m._tta_cache == {} and m.last_grad_norm is None
    m.compile(optimizer=pkg.get_optimizer('sgd', 0.01, average_type='ema', clipnorm=1.0), metrics={'pred_mask': pkg.Jaccard},
              loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255), sample_weight_mode='temporal', distributed=False)
    assert set(vars(m)) == before
    assert m._jaccard is True and m.sample_weight_mode == 'temporal'
    m.compile(optimizer=pkg.SGD(0.01), distributed=False)
    assert set(vars(m)) == before and m._jaccard is False and m.sample_weight_mode is None
