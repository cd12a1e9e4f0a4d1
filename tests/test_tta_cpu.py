"""Multi-scale / mirrored evaluation without a device: the C entry point exists and refuses out-of-contract arguments with
DL3P_EINVAL before anything is launched, the scaled-size rule, properties of the float64 rule the GPU tests compare against
(tests/tta_rules.py), the condition on its near-ties that bounds what those tests may leave unchecked, and the ValueErrors of the
Python layers on models built on the CPU."""
import inspect
import subprocess

import numpy as np
import pytest

import tta_rules
from conftest import load_pkg

P = 1 << 20                 # a 16-byte aligned address that no refused call reads


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_point():
    libm = load_pkg('_lib')
    ret, args = libm.parse_header()['dl3p_tta_accumulate']
    assert ret == 'int' and len(args) == 18 and args[-1] == 'void*'
    assert args[:7] == ['const float*', 'int', 'const float*', 'int', 'int', 'int', 'float']
    out = subprocess.run(['nm', '-D', '--defined-only', libm.LIBPATH], capture_output=True, text=True, check=True).stdout
    assert 'dl3p_tta_accumulate' in {line.split()[-1] for line in out.splitlines()}


def _call(z=P, ldz=24, zm=2 * P, ldzm=24, h=9, w=9, weight=0.5, acc_in=3 * P, acc_out=3 * P, ld_acc=24, labels=4 * P, pred=5 * P,
          cm=6 * P, N=2, C=21, H=33, W=33):
    return (z, ldz, zm, ldzm, h, w, weight, acc_in, acc_out, ld_acc, labels, pred, cm, N, C, H, W, None)


BAD = [('C=0', _call(C=0)), ('C=257', _call(C=257, ldz=260, ldzm=260, ld_acc=260)), ('larger', _call(h=34)), ('larger', _call(w=34)),
       ('needs a plain or a mirrored', _call(z=None, zm=None)),
       ('logits must be 16-byte', _call(z=P + 4)), ('mirrored logits must be 16-byte', _call(zm=2 * P + 8)),
       ('logits must be 16-byte', _call(ldz=22)), ('logits must be 16-byte', _call(ldz=20)),
       ('mirrored logits', _call(ldzm=26)), ('mirrored logits', _call(ldzm=16)),
       ('the sum must be', _call(acc_in=3 * P + 4)), ('the sum must be', _call(acc_out=3 * P + 4)),
       ('the sum must be', _call(ld_acc=22)), ('the sum must be', _call(ld_acc=20)), ('the sum must be', _call(acc_in=None, ld_acc=20)),
       ('nothing to produce', _call(acc_out=None, pred=None, labels=None, cm=None)),
       ('come together', _call(cm=None)), ('come together', _call(labels=None)),
       ('bad dims', _call(N=0)), ('bad dims', _call(h=0))]


@pytest.mark.parametrize('word,args', BAD, ids=['%s-%d' % (w.split()[0], i) for i, (w, _) in enumerate(BAD)])
def test_entry_point_refuses_what_it_cannot_serve(word, args):
    libm = load_pkg('_lib')
    fn = libm.lib().tta_accumulate
    assert fn.raw(*args) == -1, word                                        # DL3P_EINVAL, and nothing was launched
    with pytest.raises(libm.Dl3pError, match=word):
        fn(*args)


# ------------------------------------------------------------------------------------------------ the scaled size
def test_tta_size_is_the_crop_size_rule():
    tta_size = load_pkg('model').tta_size
    scales = (0.5, 0.75, 1.25, 1.5, 1.75)
    assert [tta_size(513, s) for s in scales] == [257, 385, 641, 769, 897]
    assert [tta_size(512, s) for s in scales] == [256, 384, 639, 767, 895]
    assert all(tta_size(n, 1.0) == n for n in (1, 33, 65, 512, 513, 1025))
    assert [tta_size(65, s) for s in (0.5, 1.0, 1.5)] == [33, 65, 97]


# ------------------------------------------------------------------------------------------------ the rule itself
def test_one_pass_is_the_softmax_of_the_resize():
    from oracle import np_ops
    zs, _ = tta_rules.case_inputs(0)
    want = np_ops.softmax_fwd(np_ops.resize_bilinear_fwd(zs[0].astype(np.float64), 33, 33))
    assert np.array_equal(tta_rules.rule(zs[:1], None, 33, 33), want)


@pytest.mark.parametrize('i', range(len(tta_rules.CASES)), ids=tta_rules.CASE_IDS)
def test_the_weights_sum_to_one(i):
    acc, _, _ = tta_rules.case_rule(i)
    assert np.abs(acc.sum(-1) - 1.0).max() < 1e-12


def test_a_mirrored_pass_of_mirrored_logits_is_the_plain_pass():
    """The resize takes its source coordinates in float32, as TensorFlow and the kernels do.  Where in / out is not a float32 number
    (9 / 33) the coordinate of column x and that of column W - 1 - x round differently, and the two sides differ by 1e-7: a property
    of the coordinate rounding, not of the mirroring.  So the identity is checked at ratios that are exact in float32 (1/4, 1/2, 1,
    3/4), even and odd widths, where only the float64 summation order differs."""
    rng = np.random.default_rng(7)
    for (h, w), (H, W) in (((8, 6), (32, 24)), ((5, 7), (20, 28)), ((9, 9), (18, 18)), ((17, 23), (17, 23)), ((6, 9), (8, 12))):
        z = rng.standard_normal((2, h, w, 5)) * 3.0
        plain = tta_rules.pass_probs(z, H, W)
        again = tta_rules.pass_probs(z[:, :, ::-1, :], H, W, mirrored=True)
        assert np.abs(plain - again).max() <= 1e-12


@pytest.mark.parametrize('i', range(len(tta_rules.CASES)), ids=tta_rules.CASE_IDS)
def test_near_ties_of_the_rule_are_rare_enough_to_leave_out(i):
    """a condition, not a measurement: the GPU test compares the argmax only where the rule's two best sums are at least NEAR_TIE
    apart, so at most this share of a case's pixels may go unchecked"""
    _, _, gap = tta_rules.case_rule(i)
    assert float((gap < tta_rules.NEAR_TIE).mean()) <= 1e-3


def test_inputs_follow_the_recipe():
    zs, zms = tta_rules.case_inputs(1)
    assert [z.shape for z in zs] == [(1, 5, 7, 4), (1, 10, 14, 4)] == [z.shape for z in zms]
    assert all(z.dtype == np.float32 for z in zs + zms)
    # the scene class carries + 4: the mirrored map's favourite classes are the plain map's, reversed along x (3 x 3 blocks)
    blocks = lambda z: z[0].argmax(-1)[np.ix_([0, 2, 4], [0, 3, 6])]
    assert np.array_equal(blocks(zs[0]), blocks(zms[0])[:, ::-1])


# ------------------------------------------------------------------------------------------------ the Python layers
def test_evaluate_miou_and_deeplab_accept_the_keywords():
    model, inf = load_pkg('model'), load_pkg('inference')
    sig = inspect.signature(model.DeeplabModel.evaluate_miou)
    assert sig.parameters['scales'].default == (1.0,) and sig.parameters['flip'].default is False
    assert sig.parameters['scales'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig.parameters)[:5] == ['self', 'gen', 'steps', 'class_names', 'verbose']
    assert inf.DeepLab._defaults['scales'] == (1.0,) and inf.DeepLab._defaults['flip'] is False
    sig = inspect.signature(model.DeeplabModel.predict_tta)
    assert sig.parameters['scales'].default == (1.0,) and sig.parameters['flip'].default is False
    assert 'write' in inspect.signature(load_pkg('ops').tta_accumulate).parameters
    assert hasattr(load_pkg('executor').Executor, 'eval_logits')


@pytest.fixture(scope='module')
def small_model():
    return load_pkg().get_deeplabv3p_model('mobilenetv2_lite', 21, (65, 65), 16, training=False)


U8 = np.zeros((1, 65, 65, 3), np.uint8)


def test_empty_and_non_positive_scales_are_refused(small_model):
    with pytest.raises(ValueError, match='at least one scale'):
        small_model.predict_tta(U8, scales=())
    with pytest.raises(ValueError, match='positive'):
        small_model.predict_tta(U8, scales=(1.0, 0.0))
    with pytest.raises(ValueError, match='positive'):
        small_model.evaluate_miou([(U8, U8[..., 0])], scales=(-0.5,), flip=True)


def test_frames_that_are_not_bytes_are_refused(small_model):
    with pytest.raises(ValueError, match='uint8'):
        small_model.predict_tta(U8.astype(np.float32), scales=(0.5, 1.0))
    with pytest.raises(ValueError, match='uint8'):
        small_model.evaluate_miou([(U8.astype(np.float32), U8[..., 0])], scales=(0.5, 1.0))


def test_a_scaled_shape_the_factory_refuses_names_the_scale():
    m = load_pkg().get_deeplabv3p_model('peleenet_lite', 21, (64, 64), 16, training=False)
    # PeleeNet's stem needs ceil(size / 2) even: 64 * 0.6 -> 38 -> 19 is refused by the factory, before any device is asked for
    with pytest.raises(ValueError, match=r'scale 0\.6:.*\(38, 38\).*PeleeNet cannot take input'):
        m._tta_siblings((1.0, 0.6))
    with pytest.raises(ValueError, match=r'scale 0\.6'):
        m.predict_tta(np.zeros((1, 64, 64, 3), np.uint8), scales=(0.6,), flip=True)


def test_unet_and_fast_scnn_models_are_refused(tmp_path):
    pkg = load_pkg()
    unet = pkg.get_unet_model('unet_lite', 4, (32, 32), training=False)
    with pytest.raises(ValueError, match='get_unet_model'):
        unet.predict_tta(np.zeros((1, 32, 32, 3), np.uint8), scales=(0.5,))
    with pytest.raises(ValueError, match='get_unet_model'):
        unet.evaluate_miou([], scales=(1.0,), flip=True)
    fs = pkg.get_fast_scnn_model('fast_scnn', 4, (256, 256), training=False)
    with pytest.raises(ValueError, match='get_fast_scnn_model'):
        fs.predict_tta(np.zeros((1, 256, 256, 3), np.uint8), flip=True)
    classes = tmp_path / 'classes.txt'
    classes.write_text('\n'.join('class%d' % i for i in range(4)) + '\n')
    with pytest.raises(ValueError, match='get_unet_model'):
        load_pkg('inference').DeepLab(model_type='unet_lite', model_input_shape=(32, 32), classes_path=str(classes), weights_path=None,
                                      scales=(0.5, 1.0))
