"""GhostNet on the MI355X: the two model types end to end -- predict against the float64 restatement (tests/ghostnet_oracle.py)
with every eligible ghost module on the fused forward (dl3p_ghost_fwd, Executor._find_ghost) and with none, one train step
against the restatement, the same step with a frozen backbone on the fused forward, hipGraph replay against eager, the default
dispatch at 2 x 512 x 512 and a full-size fp32 step.  Tolerances are those of tests/test_peleenet_gpu.py."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from ghostnet_oracle import GhostOracle, TOL, data as _data, rel as _rel, relu_derivs

pytestmark = pytest.mark.gpu
TYPES = ('ghostnet', 'ghostnet_lite')


def _randomise(o):
    rng = np.random.default_rng(42)
    for k, v in o.net.params.items():     # non-trivial BN parameters / moving statistics / biases
        if k.endswith('/gamma'):
            v[...] = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith('/beta') or k.endswith('/moving_mean'):
            v[...] = rng.standard_normal(v.shape) * 0.1
        elif k.endswith('/moving_variance'):
            v[...] = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith('/bias'):
            v[...] = rng.standard_normal(v.shape) * 0.1


def _pair(mt, H, W, C, OS, freeze_level=0, training=True):
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model(mt, C, (H, W), OS, freeze_level=freeze_level, training=training)
    if training:
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    o = GhostOracle(mt, C, (H, W), OS, freeze_level=freeze_level)
    _randomise(o)
    m.set_weights_by_name(dict(o.net.params))
    return m, o


def _eligible(m, N):
    """ghost modules whose shape dl3p_ghost_fwd serves (all of them stride 1, 3x3, one buffer: tests/test_ghostnet_cpu.py)"""
    ops = load_pkg('ops')
    return [op for op in m.graph.ops if op.kind == 'conv_pw' and op.name.endswith('_primary_conv_0')
            and ops.ghost_fwd_supported((N, op.Ho, op.Wo, op.cin), op.cout)]


@pytest.mark.parametrize('mt', TYPES)
@pytest.mark.parametrize('OS', [8, 16])
@pytest.mark.parametrize('fused', [True, False])
def test_predict_matches_restatement(mt, OS, fused, monkeypatch):
    if fused:
        monkeypatch.setenv('DL3P_GHOST_MIN_ROWS', '0')
        monkeypatch.setenv('DL3P_GHOST', '1')
    else:
        monkeypatch.setenv('DL3P_GHOST', '0')
    H = W = 64
    m, o = _pair(mt, H, W, 21, OS, training=False)
    x, _ = _data(2, H, W, 21)
    p = m.predict(x)
    _, p_ref = o.predict(x)
    assert p.shape == (2, H, W, 21)
    assert np.abs(p - p_ref).max() < TOL
    ex = m._executor(2, False)
    n = len(_eligible(m, 2))
    # 64 x 64: 16 -> 8 twice and 16 -> 24 on the 32 x 32 map, 48 -> 12, 24 -> 36 twice and 72 -> 12 on the 16 x 16 map
    assert n == 7
    assert ex.ghost_launches() == (n if fused else 0)
    names = [name for name, _ in ex.fwd.labels]
    assert names.count('dl3p_dwconv2d_fwd') + ex.ghost_launches() == sum(1 for op in m.graph.ops if op.kind == 'conv_dw')


def _train_step_vs_restatement(mt, OS, H, W, freeze_level=0):
    from test_model_gpu import _act_derivs_seq
    N, C = 2, 21
    m, o = _pair(mt, H, W, C, OS, freeze_level=freeze_level)
    m.use_graphs = False
    w0 = m.get_weights_by_name()
    x, y = _data(N, H, W, C, seed=3)
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    drop = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0][0]
    mask = ex.dropout_mask(drop).cpu().numpy()
    # the ReLU / hard-sigmoid branch pattern of the float32 run goes into the float64 restatement (oracle/np_net.py
    # Net.act_derivs): BatchNorm + ReLU by name, the squeeze-excite activations in creation order
    o.net.act_derivs = relu_derivs(m, ex, load_pkg('ops'))
    o.net.act_derivs_seq = _act_derivs_seq(m, ex, o.net.act_derivs)
    total, ce, logits = o.loss_and_grads(x, y, {'aspp_dropout': mask})
    assert abs(loss - ce) < TOL * max(1.0, abs(ce)), (loss, ce)
    st = m._store
    worst = ('', 0.0)
    for p in m.graph.all_params():
        if not p.trainable:
            continue
        g = st.get(p, st.G)
        gref = o.net.grads[p.name]
        r = _rel(g, gref) if np.abs(gref).max() > 1e-7 else float(np.abs(g).max())
        if r > worst[1]:
            worst = (p.name, r)
    print('worst gradient', worst, 'flips', o.net.flip_count, o.net.flip_total)
    gtol = 1e-2
    assert worst[1] < gtol, worst
    assert o.net.flip_count <= max(8, 2e-4 * o.net.flip_total), (o.net.flip_count, o.net.flip_total)
    grads = {k: v.copy() for k, v in o.net.grads.items()}
    o.sgd_step(0.01, 0.9)
    w1 = m.get_weights_by_name()
    for k, v in w1.items():
        lim = TOL * max(1.0, np.abs(o.net.params[k]).max())
        if k in grads:
            lim += 0.01 * gtol * np.abs(grads[k]).max()
        assert np.abs(v - o.net.params[k]).max() < lim, k
    return m, o, ex, w0, w1


@pytest.mark.parametrize('mt,H,W', [('ghostnet', 64, 64), ('ghostnet_lite', 64, 64), ('ghostnet', 72, 104)])
def test_train_step_matches_restatement(mt, H, W):
    """one SGD step against float64 with the activation pattern injected; 72 x 104 is ragged at every stride (36 x 52, 18 x 26,
    9 x 13, 5 x 7).  Every BatchNorm trains: no module is fused"""
    m, o, ex, w0, w1 = _train_step_vs_restatement(mt, 16, H, W)
    assert ex.ghost_launches() == 0


@pytest.mark.parametrize('mt', TYPES)
def test_frozen_backbone_step_runs_fused(mt, monkeypatch):
    """freeze_level=1 (the first stage of train.py): the backbone's BatchNorms run on their moving statistics, so its ghost
    modules take the fused forward; the head's gradients agree with the restatement (moving statistics in the frozen part) and
    the backbone does not move by a bit"""
    monkeypatch.setenv('DL3P_GHOST_MIN_ROWS', '0')
    monkeypatch.setenv('DL3P_GHOST', '1')
    m, o, ex, w0, w1 = _train_step_vs_restatement(mt, 16, 64, 64, freeze_level=1)
    assert ex.ghost_launches() == len(_eligible(m, 2)) == 7
    backbone = {p.name for l in m.layers[:m.backbone_len] for p in l.params}
    assert len(backbone) > 400
    for k in backbone:
        assert np.array_equal(w0[k].view(np.uint32), w1[k].view(np.uint32)), k
    assert any(not np.array_equal(w0[k], w1[k]) for k in w1 if k not in backbone)


@pytest.mark.parametrize('freeze_level', [0, 1])
def test_graph_replay_equals_eager(freeze_level, monkeypatch):
    monkeypatch.setenv('DL3P_GHOST_MIN_ROWS', '0')
    monkeypatch.setenv('DL3P_GHOST', '1')
    N, C, H, W = 2, 21, 64, 64
    ma, _ = _pair('ghostnet', H, W, C, 16, freeze_level=freeze_level)
    mb, _ = _pair('ghostnet', H, W, C, 16, freeze_level=freeze_level)
    ma.use_graphs, mb.use_graphs = False, True
    la, lb = [], []
    for s in range(3):
        x, y = _data(N, H, W, C, seed=10 + s)
        la.append(ma.train_on_batch(x, y))
        lb.append(mb.train_on_batch(x, y))
    assert mb._executor(N, True).graphed
    assert mb._executor(N, True).ghost_launches() == (7 if freeze_level else 0)
    assert np.allclose(la, lb, rtol=1e-5, atol=1e-6), (la, lb)
    wa, wb = ma.get_weights_by_name(), mb.get_weights_by_name()
    assert max(float(np.abs(wa[k] - wb[k]).max()) for k in wa) < 1e-5


def test_default_dispatch_at_512(monkeypatch):
    """no environment set: the default decides -- no fused launch while the kernel is opt-in (executor.GHOST_ON_BY_DEFAULT False:
    not measured), else the executor.GHOST_DEFAULT shapes from executor.GHOST_MIN_ROWS rows up; finite probabilities
    that sum to 1"""
    monkeypatch.delenv('DL3P_GHOST_MIN_ROWS', raising=False)
    monkeypatch.delenv('DL3P_GHOST', raising=False)
    pkg = load_pkg()
    exe = load_pkg('executor')
    N, H, W = 2, 512, 512
    m = pkg.get_deeplabv3p_model('ghostnet', 21, (H, W), 16, training=False)
    x, _ = _data(N, H, W, 21, seed=2)
    p = m.predict(x)
    assert p.shape == (N, H, W, 21) and np.isfinite(p).all()
    assert np.abs(p.sum(-1) - 1).max() < 1e-4
    el = _eligible(m, N)
    assert sorted((op.cin, op.cout, op.Ho) for op in el) == [(16, 8, 256), (16, 8, 256), (16, 24, 256), (24, 36, 128), (24, 36, 128),
                                                            (48, 12, 128), (72, 12, 128)]
    want = sum(1 for op in el if (op.cin, op.cout) in exe.GHOST_DEFAULT and N * op.Ho * op.Wo >= exe.GHOST_MIN_ROWS)
    if not exe.GHOST_ON_BY_DEFAULT:
        want = 0
    assert m._executor(N, False).ghost_launches() == want
    del m
    torch.cuda.empty_cache()


def test_full_size_step_is_finite():
    pkg = load_pkg()
    N, C, H, W = 16, 21, 512, 512
    m = pkg.get_deeplabv3p_model('ghostnet', C, (H, W), 16)
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    x, y = _data(N, H, W, C, seed=1)
    loss = m.train_on_batch(x, y)
    assert np.isfinite(loss) and abs(loss - np.log(C)) < 1.0, loss
    del m
    torch.cuda.empty_cache()
