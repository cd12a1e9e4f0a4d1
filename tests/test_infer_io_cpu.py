"""The inference front end (csrc/infer_io.hip, augment.pil_resize, inference.py, the deeplab shim) without a device: the NumPy
restatement of Pillow's 8-bit bicubic resize (tests/pil_rules.py) is Pillow's -- golden outputs everywhere, live where PIL imports --
the product's coefficient tables are the restatement's, the colour map is the PASCAL one, the DeepLab class builds through the right
factory, and the library refuses out-of-contract arguments with DL3P_EINVAL before anything is launched."""
import os
import subprocess

import numpy as np
import pytest

import pil_rules
from conftest import load_pkg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pil_bicubic.npz')
CASE_IDS = ['%dx%d-%dx%d' % (hw + HW) for hw, HW in pil_rules.CASES]
# the size pairs of real use on top of the small cases: VOC and video frames to 512 / 513, a thin strip, a shrink by one sample
LIVE_EXTRA = (((375, 500), (512, 512)), ((1080, 1920), (512, 512)), ((720, 1280), (513, 513)), ((5, 300), (16, 16)), ((33, 33), (32, 32)))
P = 1 << 20                 # a 16-byte aligned address that no refused call reads


# ------------------------------------------------------------------------------------------------ the restatement is Pillow's
@pytest.mark.parametrize('kind', pil_rules.KINDS)
@pytest.mark.parametrize('i', range(len(pil_rules.CASES)), ids=CASE_IDS)
def test_restated_resize_equals_pillows_stored_output(i, kind):
    hw, HW = pil_rules.CASES[i]
    want = np.load(GOLDEN)['out%d_%s' % (i, kind)]
    got = pil_rules.resize_bicubic(pil_rules.case_input(hw, kind), HW)
    assert got.shape == HW + (3,) and got.dtype == np.uint8
    assert np.array_equal(got, want)


def test_binary_noise_reaches_both_clamps_in_pillow_itself():
    """the stored Pillow outputs hold 0 and 255 where the bicubic overshoot leaves the byte range (the upscale of 0 / 255 noise)"""
    out = np.load(GOLDEN)['out0_binary']
    assert out.min() == 0 and out.max() == 255


@pytest.mark.parametrize('kind', pil_rules.KINDS)
@pytest.mark.parametrize('hw,HW', pil_rules.CASES + LIVE_EXTRA, ids=CASE_IDS + ['%dx%d-%dx%d' % (a + b) for a, b in LIVE_EXTRA])
def test_restated_resize_equals_live_pillow(hw, HW, kind):
    Image = pytest.importorskip('PIL.Image')
    x = pil_rules.case_input(hw, kind)
    want = np.asarray(Image.fromarray(x).resize(HW[::-1], Image.BICUBIC))
    assert np.array_equal(pil_rules.resize_bicubic(x, HW), want)


# ------------------------------------------------------------------------------------------------ the product's tables
TABLE_CASES = tuple(c for c in pil_rules.CASES + LIVE_EXTRA if c[0][0] <= 16 * c[1][0] and c[0][1] <= 16 * c[1][1])    # within the cap


@pytest.mark.parametrize('hw,HW', TABLE_CASES, ids=['%dx%d-%dx%d' % (a + b) for a, b in TABLE_CASES])
def test_product_tables_equal_the_restatement(hw, HW):
    aug = load_pkg('augment')
    tables, kx, ky = aug.pil_resize_tables(hw[0], hw[1], HW[0], HW[1])
    assert tables.dtype == np.int32
    o = 0
    for src, dst, ks in ((hw[1], HW[1], kx), (hw[0], HW[0], ky)):        # the horizontal axis first
        if src == dst:
            assert ks == 0
            continue
        lo, cnt, k = pil_rules.axis_tables(src, dst)
        assert ks == k.shape[1]
        assert np.array_equal(tables[o:o + dst], lo) and np.array_equal(tables[o + dst:o + 2 * dst], cnt)
        assert np.array_equal(tables[o + 2 * dst:o + (2 + ks) * dst].reshape(dst, ks), k)
        o += (2 + ks) * dst
    assert o == tables.size


def test_a_shrink_beyond_sixteen_is_refused_by_the_table_builder():
    aug = load_pkg('augment')
    assert aug.pil_resize_tables(8, 300, 8, 19)[1] == 65                  # 15.8: the cap itself
    with pytest.raises(ValueError, match='coefficients'):
        aug.pil_resize_tables(8, 340, 8, 19)                              # 17.9: ksize 73
    with pytest.raises(ValueError, match='coefficients'):
        aug.pil_resize_tables(340, 8, 19, 8)
    with pytest.raises(ValueError, match='coefficients'):
        aug.pil_resize_tables(5, 300, 16, 16)                             # 18.75 (Pillow serves it: tests/pil_rules.py does too)
    with pytest.raises(ValueError, match='bicubic'):
        aug.pil_resize_tables(8, 8, 4, 4, filter='lanczos')


# ------------------------------------------------------------------------------------------------ colour map
def test_colormap_is_the_pascal_one():
    inf = load_pkg('inference')
    cm = inf.create_pascal_label_colormap()
    assert cm.shape == (256, 3)
    assert cm[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]]
    assert np.array_equal(cm, pil_rules.colormap())


def test_label_to_color_image_takes_rank_two_only():
    inf = load_pkg('inference')
    lab = np.array([[0, 1], [2, 15]], np.uint8)
    assert np.array_equal(inf.label_to_color_image(lab), pil_rules.colormap()[lab])
    with pytest.raises(ValueError):
        inf.label_to_color_image(np.zeros((2, 2, 3), np.uint8))


def test_overlay_tables_are_the_restated_nearest_indices():
    inf = load_pkg('inference')
    for (H, W), (h0, w0) in (((16, 24), (37, 53)), ((65, 65), (48, 80)), ((512, 512), (1080, 1920))):
        t = inf.overlay_tables(H, W, h0, w0)
        assert t.dtype == np.int32
        assert np.array_equal(t[:w0], pil_rules.nearest_index(w0, W)) and np.array_equal(t[w0:], pil_rules.nearest_index(h0, H))


# ------------------------------------------------------------------------------------------------ the DeepLab class
@pytest.fixture
def classes_path(tmp_path):
    p = tmp_path / 'classes.txt'
    p.write_text('\n'.join('class%d' % i for i in range(21)) + '\n')
    return str(p)


def test_the_root_shim_resolves_to_the_package_class():
    from deeplab import DeepLab
    assert DeepLab is load_pkg('inference').DeepLab and DeepLab is load_pkg().DeepLab


def test_deeplab_builds_a_random_model_without_weights(classes_path):
    from deeplab import DeepLab
    d = DeepLab(model_type='mobilenetv2_lite', model_input_shape=(65, 65), output_stride=16, classes_path=classes_path,
                weights_path=None)
    assert len(d.class_names) == 21 and d.deeplab_model.num_classes == 21
    assert d.deeplab_model.model_type == 'mobilenetv2_lite' and not d.deeplab_model.flatten_output
    assert tuple(d.deeplab_model.input_shape_hw) == (65, 65)


def test_do_crf_is_refused(classes_path):
    from deeplab import DeepLab
    with pytest.raises(ValueError, match='CRF'):
        DeepLab(model_type='mobilenetv2_lite', model_input_shape=(65, 65), output_stride=16, classes_path=classes_path,
                weights_path=None, do_crf=True)


def test_unet_types_build_through_the_unet_factory(classes_path, monkeypatch):
    inf = load_pkg('inference')
    seen = []
    real = inf.get_unet_model
    monkeypatch.setattr(inf, 'get_unet_model', lambda *a, **k: seen.append(a[0]) or real(*a, **k))
    d = inf.DeepLab(model_type='unet_lite', model_input_shape=(32, 32), classes_path=classes_path, weights_path=None)
    assert seen == ['unet_lite'] and d.deeplab_model.model_type == 'unet_lite' and not d.deeplab_model.flatten_output


# ------------------------------------------------------------------------------------------------ the C ABI
NEW = ('dl3p_pil_resize_workspace', 'dl3p_pil_resize_u8', 'dl3p_mask_overlay_u8')


def test_header_declares_and_library_exports_the_entry_points():
    libm = load_pkg('_lib')
    protos = libm.parse_header()
    assert protos['dl3p_pil_resize_workspace'][0] == 'size_t'
    for name in NEW[1:]:
        ret, args = protos[name]
        assert ret == 'int' and args[-1] == 'void*', name
    out = subprocess.run(['nm', '-D', '--defined-only', libm.LIBPATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    assert set(NEW) <= exported, set(NEW) - exported


def test_workspace_is_the_byte_intermediate_of_two_passes():
    L = load_pkg('_lib').lib()
    assert L.pil_resize_workspace(2, 37, 53, 16, 12) == 2 * 37 * 36          # N h rows of 3 W bytes
    assert L.pil_resize_workspace(1, 33, 50, 13, 17) == 33 * 52              # rows padded to 4 bytes
    assert L.pil_resize_workspace(1, 40, 64, 20, 64) == 0 and L.pil_resize_workspace(1, 40, 64, 40, 32) == 0
    assert L.pil_resize_workspace(1, 24, 24, 24, 24) == 0


def _resize(img=P, pitch=3 * 53, out=2 * P, ws=3 * P, ws_bytes=1 << 20, tab=4 * P, kx=19, ky=13, N=1, h=37, w=53, H=16, W=12):
    return 'pil_resize_u8', (img, pitch, out, ws, ws_bytes, tab, kx, ky, N, h, w, H, W, None)


def _overlay(pred=P, img=2 * P, mask=3 * P, over=4 * P, tab=5 * P, cmap=6 * P, n_valid=21, alpha=179, N=1, H=16, W=24, h0=37, w0=53):
    return 'mask_overlay_u8', (pred, img, mask, over, tab, cmap, n_valid, alpha, N, H, W, h0, w0, None)


BAD = [('coefficients', _resize(kx=67)), ('coefficients', _resize(ky=67)), ('coefficients', _resize(kx=-1)),
       ('workspace', _resize(ws_bytes=37 * 36 - 1)), ('workspace', _resize(ws=None)), ('workspace', _resize(ws=3 * P + 1)),
       ('output size', _resize(H=0)), ('output size', _resize(W=0)), ('output size', _resize(W=-3)),
       ('skipped', _resize(kx=0)), ('skipped', _resize(w=12, pitch=36)), ('tables', _resize(tab=None)),
       ('pitch', _resize(pitch=3 * 53 - 1)), ('bad arguments', _resize(out=P)), ('bad arguments', _resize(N=0)),
       ('bad arguments', _overlay(mask=None, over=None)), ('bad arguments', _overlay(h0=0)), ('bad arguments', _overlay(pred=None)),
       ('overlay needs', _overlay(img=None)), ('overlay needs', _overlay(cmap=None)), ('overlay needs', _overlay(over=2 * P)),
       ('alpha', _overlay(alpha=257)), ('alpha', _overlay(n_valid=256))]


@pytest.mark.parametrize('word,call', BAD, ids=['%s-%d' % (c[0], i) for i, (_, c) in enumerate(BAD)])
def test_entry_points_refuse_what_they_cannot_serve(word, call):
    libm = load_pkg('_lib')
    L = libm.lib()
    name, args = call
    fn = getattr(L, name)
    assert fn.raw(*args) == -1, (name, word)                              # DL3P_EINVAL, and nothing was launched
    with pytest.raises(libm.Dl3pError, match=word):
        fn(*args)
