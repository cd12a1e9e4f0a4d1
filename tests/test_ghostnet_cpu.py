"""GhostNet / GhostNet-Lite DeepLabV3+ graphs (ghostnet.py): topology against counts derived from the reference's tables
(deeplabv3p_ghostnet.py:204-285), the one-buffer-per-ghost-module layout, freeze levels, names / shapes / order against a
float64 restatement (tests/ghostnet_oracle.py), the .h5 round trip, the refusal under mixed_bfloat16, and that restatement
against torch-CPU autograd.  No GPU needed."""
from collections import Counter

import numpy as np
import pytest

from conftest import load_pkg
from ghostnet_oracle import GhostOracle, torch_oracle

TYPES = ('ghostnet', 'ghostnet_lite')

# Derived from the tables, not from the code under test.  Sixteen bottlenecks, each with two ghost modules (primary 1x1 conv,
# BN, cheap 3x3 depthwise conv, BN): 32 Conv2D + 32 DepthwiseConv2D + 64 BN.  Four bottlenecks change the resolution or keep
# that structure (blocks 1_0, 3_0, 5_0, 7_0): + 4 DepthwiseConv2D + 4 BN.  Five change the width or the resolution (those four
# and 6_3, 80 -> 112) and have a conv shortcut: + 5 DepthwiseConv2D + 5 Conv2D + 10 BN.  Seven have squeeze-excite (3_0, 4_0,
# 6_3, 6_4, 7_0, 8_1, 8_3): + 14 Conv2D.  Stem and blocks_9_0: + 2 Conv2D + 2 BN.  Total 53 Conv2D, 41 DepthwiseConv2D, 80 BN.
N_BN, N_CONV, N_DW, N_ADD, N_SE = 80, 53, 41, 16, 7
N_TRAINABLE, N_NON_TRAINABLE = 2671428, 21968


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('OS', [8, 16, 32])
def test_topology(mt, OS):
    m = load_pkg().get_deeplabv3p_model(mt, 21, (512, 512), OS)
    body = m.layers[:m.backbone_len]
    assert sum(p.size for l in body for p in l.params if p.weight_trainable) == N_TRAINABLE
    assert sum(p.size for l in body for p in l.params if not p.weight_trainable) == N_NON_TRAINABLE
    kinds = Counter(l.kind for l in body)
    assert (kinds['BatchNormalization'], kinds['Conv2D'], kinds['DepthwiseConv2D']) == (N_BN, N_CONV, N_DW)
    assert sum(1 for l in body if l.name.endswith('_add')) == N_ADD
    assert sum(1 for l in body if l.name.endswith('_se_conv_reduce')) == N_SE
    assert sum(1 for l in body if l.name.endswith('_se_hard_sigmoid')) == N_SE
    shortcuts = {l.name[:-len('_shortcut_0')] for l in body if l.name.endswith('_shortcut_0')}
    kept = {l.name[:-len('_conv_dw')] for l in body if l.name.endswith('_conv_dw')}
    if OS == 32:
        assert len(shortcuts) == 5
    # s = -1 keeps the downsample structure of the stages an output stride flattens
    assert {8: {'blocks_5_0', 'blocks_7_0'}, 16: {'blocks_7_0'}, 32: set()}[OS] <= shortcuts
    assert kept == {'blocks_1_0', 'blocks_3_0', 'blocks_5_0', 'blocks_7_0'}
    assert m.graph.taps['backbone_out'].shape == (512 // OS, 512 // OS, 960)
    assert m.graph.taps['backbone_out'].klayer.name == 'blocks_9_0_relu'
    skip = m.get_layer('blocks_2_0_add')
    assert skip.output_shape == (128, 128, 24)
    if not mt.endswith('_lite'):
        assert m.get_layer('feature_projection0').inbound[0] is skip
    names = {l.name for l in body}
    for n in ('conv_stem', 'bn1', 'Conv2D_1_act', 'blocks_0_0_ghost1_primary_conv_0', 'blocks_0_0_ghost1_primary_conv_1',
              'blocks_0_0_ghost1_primary_conv_relu', 'blocks_0_0_ghost1_cheap_operation_0', 'blocks_0_0_ghost1_cheap_operation_1',
              'blocks_0_0_ghost1_cheap_operation_relu', 'blocks_0_0_ghost1_concat', 'blocks_0_0_ghost2_concat', 'blocks_1_0_conv_dw',
              'blocks_1_0_bn_dw', 'blocks_3_0_se_avg_pool2d', 'blocks_3_0_se_conv_reduce', 'blocks_3_0_se_act',
              'blocks_3_0_se_conv_expand', 'blocks_3_0_se_hard_sigmoid', 'blocks_1_0_shortcut_0', 'blocks_1_0_shortcut_1',
              'blocks_1_0_shortcut_2', 'blocks_1_0_shortcut_3', 'blocks_8_3_add', 'blocks_9_0_conv', 'blocks_9_0_bn1',
              'blocks_9_0_relu', 'reshape', 'multiply', 'reshape_6', 'multiply_6'):
        assert n in names, n
    assert 'blocks_0_0_ghost2_primary_conv_relu' not in names           # ghost2 has no activation
    add = m.get_layer('blocks_1_0_add')                                 # Add([x, sc]) in that order
    assert [l.name for l in add.inbound] == ['blocks_1_0_ghost2_concat', 'blocks_1_0_shortcut_3']
    bn = m.get_layer('bn1')
    spec = [b for b in m.graph.bns if b.layer is bn][0]
    assert (spec.eps, spec.momentum) == (1e-3, 0.99)


@pytest.mark.parametrize('mt', TYPES)
def test_builds_at_513(mt):
    m = load_pkg().get_deeplabv3p_model(mt, 21, (513, 513), 16)
    assert m.graph.taps['backbone_out'].shape == (33, 33, 960)
    assert m.get_layer('blocks_2_0_add').output_shape == (129, 129, 24)


@pytest.mark.parametrize('mt', TYPES)
def test_every_ghost_module_owns_one_buffer(mt):
    m = load_pkg().get_deeplabv3p_model(mt, 21, (64, 64), 16)
    g = m.graph
    prim = {op.name: op for op in g.ops if op.kind == 'conv_pw' and op.name.endswith('_primary_conv_0')}
    cheap = {op.name: op for op in g.ops if op.kind == 'conv_dw' and op.name.endswith('_cheap_operation_0')}
    assert len(prim) == 32 and len(cheap) == 32
    roots = set()
    for name, p in prim.items():
        d = cheap[name.replace('_primary_conv_0', '_cheap_operation_0')]
        c = p.out.C
        assert p.out.base is not None and d.out.base is p.out.base             # both halves are slices of one root
        assert (p.out.c0, d.out.c0, d.out.C, p.out.base.C) == (0, c, c, 2 * c)
        assert d.x.tensor is p.out and d.x.bn is p.bn                          # the cheap conv reads act(BN1(z1)) lazily, no copy
        assert p.bn.group is d.bn.group and (p.bn.offset, d.bn.offset) == (0, c)
        roots.add(p.out.base.id)
    assert len(roots) == 32
    concat = [l for l in m.layers if l.kind == 'Concatenate' and '_ghost' in l.name]
    assert len(concat) == 32
    assert not any(op.kind == 'materialize' and '_ghost' in op.name for op in g.ops)     # no Concatenate copy


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
    assert not m1.get_layer('blocks_9_0_conv').trainable and m1.get_layer('aspp0').trainable
    assert not m1.get_layer('blocks_0_0_ghost1_primary_conv_1').trainable
    m2 = pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, freeze_level=2)
    assert not m2.get_layer('concat_projection').trainable and m2.get_layer('conv_upsample').trainable


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('OS', [8, 16])
def test_names_and_shapes_match_restatement(mt, OS):
    m = load_pkg().get_deeplabv3p_model(mt, 21, (64, 64), OS)
    o = GhostOracle(mt, 21, (64, 64), OS)
    ps = m.graph.all_params()
    assert [p.name for p in ps] == o.net.order
    for p in ps:
        assert p.shape == o.net.params[p.name].shape, p.name
    assert {l.name for l in m.layers if l.params} == {n.rsplit('/', 1)[0] for n in o.net.order}
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


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('training', [True, False])
def test_mixed_bfloat16_is_refused_at_build_time(mt, training):
    pkg = load_pkg()
    mp = pkg.mixed_precision
    mp.set_policy(mp.Policy('mixed_bfloat16'))
    try:
        with pytest.raises(ValueError, match='CHANNEL_ALIGN'):
            pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, training=training)
    finally:
        mp.set_policy(mp.Policy('float32'))
    pkg.get_deeplabv3p_model(mt, 21, (64, 64), 16, training=training)          # ... and the float32 policy builds it again


def test_weights_argument():
    ghost = load_pkg('ghostnet')
    with pytest.raises(ValueError, match='weights'):
        ghost.Deeplabv3pGhostNet(input_shape=(64, 64, 3), weights='somewhere.h5')
    g, x, n = ghost.Deeplabv3pLiteGhostNet(input_shape=(64, 64, 3), weights='imagenet', OS=16)
    assert g.layers[n - 1].name == 'blocks_9_0_relu' and g.taps['backbone_out'].shape == (4, 4, 960)
    with pytest.raises(ValueError, match='output stride'):
        ghost.Deeplabv3pGhostNet(input_shape=(64, 64, 3), OS=4)


@pytest.mark.parametrize('mt,OS', [('ghostnet', 16), ('ghostnet_lite', 8)])
def test_restatement_matches_torch_autograd(mt, OS):
    """the float64 restatement's forward and hand-written backward against torch-CPU autograd on the same graph (the bounds of
    tests/test_peleenet_cpu.py::test_restatement_matches_torch_autograd)"""
    H = W = 64
    N, C = 2, 5
    o = GhostOracle(mt, C, (H, W), OS)
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
