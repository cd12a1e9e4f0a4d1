"""PeleeNet / PeleeNet-Lite DeepLabV3+ graphs (peleenet.py): topology against the reference README's published figures,
the output-stride table, the input-size rule, freeze levels, names / shapes / order against a float64 restatement
(tests/peleenet_oracle.py), the .h5 round trip, and that restatement against torch-CPU autograd.  No GPU needed."""
import numpy as np
import pytest

from conftest import load_pkg
from peleenet_oracle import PeleeOracle, torch_oracle, avgpool2d_fwd, avgpool2d_bwd

TYPES = ('peleenet', 'peleenet_lite')


def _conv_gflops(m):
    macs = 0
    for op in m.graph.ops:
        if op.kind in ('conv_pw', 'conv_dense'):
            kh, kw, cin, cout = op.w.shape
            macs += op.Ho * op.Wo * kh * kw * cin * cout
        elif op.kind == 'conv_dw':
            macs += op.Ho * op.Wo * op.k * op.k * op.c
    return 2.0 * macs / 1e9


def test_lite_matches_readme_row():
    """README.md:312-317: PeleeNet Lite, 512 x 512, OS 16 -- 2.59 M parameters, 7.64 G FLOPs (convolutions from below, within 1 %)"""
    m = load_pkg().get_deeplabv3p_model('peleenet_lite', 21, (512, 512), 16, training=False)
    assert m.graph.count_params(True) == 2595701
    assert m.graph.count_params(False) == 11264
    g = _conv_gflops(m)
    assert 0.99 * 7.64 <= g <= 7.64, g


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('OS,backbone_len', [(8, 364), (16, 365), (32, 366)])
def test_builds_at_every_output_stride(mt, OS, backbone_len):
    m = load_pkg().get_deeplabv3p_model(mt, 21, (512, 512), OS)
    assert m.backbone_len == backbone_len
    assert m.graph.taps['backbone_out'].shape == (512 // OS, 512 // OS, 704)
    assert sum(1 for l in m.graph.layers if l.kind == 'AveragePooling2D') == {8: 1, 16: 2, 32: 3}[OS] + 1   # (+ image pooling)
    # one buffer per dense block: every Concatenate of a block is a prefix of it
    dense = [op for op in m.graph.ops if op.kind == 'conv_dense' and '_denselayer' in op.name and op.name.endswith(('1b_conv', '2c_conv'))]
    assert len(dense) == 2 * 21 and all(op.out.base is not None and op.out.C == 16 for op in dense)
    assert len({op.out.root.id for op in dense}) == 4


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('H,W', [(513, 513), (512, 513), (66, 64)])
def test_odd_stem_concat_is_refused(mt, H, W):
    with pytest.raises(ValueError, match='stem block concatenates'):
        load_pkg().get_deeplabv3p_model(mt, 21, (H, W), 16)


@pytest.mark.parametrize('H', [512, 256, 64])
def test_valid_sizes(H):
    for mt in TYPES:
        load_pkg().get_deeplabv3p_model(mt, 21, (H, H), 16)


@pytest.mark.parametrize('mt', TYPES)
def test_freeze_levels(mt):
    pkg = load_pkg()
    m0 = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16)
    for level in (1, 2):
        m = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, freeze_level=level)
        num = m.backbone_len if level == 1 else len(m.layers) - 4     # base_len: every layer but the new head (4 layers)
        assert [l.trainable for l in m.layers] == [i >= num for i in range(len(m.layers))]
        assert [l.name for l in m.layers] == [l.name for l in m0.layers]
    m1 = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, freeze_level=1)
    assert not m1.get_layer('bbn_features_transition4_conv').trainable and m1.get_layer('aspp0').trainable
    m2 = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, freeze_level=2)
    assert not m2.get_layer('concat_projection').trainable and m2.get_layer('conv_upsample').trainable


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('OS', [8, 16])
def test_names_and_shapes_match_restatement(mt, OS):
    m = load_pkg().get_deeplabv3p_model(mt, 21, (64, 64), OS)
    o = PeleeOracle(mt, 21, (64, 64), OS)
    ps = m.graph.all_params()
    assert [p.name for p in ps] == o.net.order
    for p in ps:
        assert p.shape == o.net.params[p.name].shape, p.name
    assert {l.name for l in m.layers if l.params} == {n.rsplit('/', 1)[0] for n in o.net.order}
    # the Keras order (save_weights / load_weights by position) keeps every parameterised layer once
    assert sorted(l.name for l in m.layers) == sorted(l.name for l in m.graph.layers)


@pytest.mark.parametrize('mt', TYPES)
def test_h5_round_trip(mt, tmp_path):
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, seed=3)
    rng = np.random.default_rng(0)
    w = [rng.standard_normal(a.shape).astype(np.float32) for a in m.get_weights()]
    m.set_weights(w)
    p = str(tmp_path / 'w.h5')
    m.save_weights(p)
    m2 = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, seed=4)
    m2.load_weights(p)
    for a, b in zip(w, m2.get_weights()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('k,s', [(2, 2), (3, 2), (3, 3), (2, 1)])
def test_numpy_avgpool_matches_torch(k, s):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(k * 10 + s)
    x = rng.standard_normal((2, 11, 8, 5))
    g = rng.standard_normal(avgpool2d_fwd(x, k, s).shape)
    xt = torch.tensor(x, requires_grad=True)
    yt = F.avg_pool2d(xt.permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1)
    yt.backward(torch.tensor(g))
    np.testing.assert_allclose(avgpool2d_fwd(x, k, s), yt.detach().numpy(), atol=1e-14, rtol=0)
    np.testing.assert_allclose(avgpool2d_bwd(g, x.shape, k, s), xt.grad.numpy(), atol=1e-14, rtol=0)


@pytest.mark.parametrize('mt,OS', [('peleenet', 16), ('peleenet_lite', 8)])
def test_restatement_matches_torch_autograd(mt, OS):
    """the float64 restatement's forward and hand-written backward against torch-CPU autograd on the same graph (cf.
    tests/test_oracle_ops.py::test_whole_model_matches_torch_autograd)"""
    H = W = 64
    N, C = 2, 5
    o = PeleeOracle(mt, C, (H, W), OS)
    t = torch_oracle(mt, C, (H, W), OS)
    assert list(o.net.order) == list(t.net.order)
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (N, H, W, 3))
    y = rng.integers(0, C, (N, H * W, 1)).astype(np.float64)
    y[rng.uniform(size=y.shape) < 0.05] = 255
    mask = (rng.uniform(size=(N, H // OS, W // OS, 256)) >= 0.5).astype(np.float64)
    lo, _ = o.predict(x)
    lt, _ = t.predict(x)
    np.testing.assert_allclose(lo, lt, atol=1e-6, rtol=0)
    _, co, _ = o.loss_and_grads(x, y, {'aspp_dropout': mask})
    _, ct, _ = t.loss_and_grads(x, y, {'aspp_dropout': mask})
    np.testing.assert_allclose(o.net.taps['backbone_out'].v, t.net.taps['backbone_out'].v.detach().numpy(), atol=1e-10, rtol=0)
    assert abs(co - ct) < 1e-7
    for k, g in o.net.grads.items():
        if np.abs(g).max() > 1e-7:
            assert np.abs(g - t.net.grads[k]).max() < 1e-5 * np.abs(g).max(), k
