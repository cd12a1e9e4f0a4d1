"""PeleeNet on the MI355X: local average pooling (dl3p_avgpool2d_*, fp32 and bf16) against float64, and the two PeleeNet
model types end to end -- predict and one train step against the float64 restatement (tests/peleenet_oracle.py), hipGraph
replay against eager, a bf16 step against the fp32 one, and a full-size fp32 step."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from oracle import np_ops as O
from peleenet_oracle import PeleeOracle, avgpool2d_fwd, avgpool2d_bwd, TOL, data as _data, rel as _rel, relu_derivs

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dt)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# (N, H, W, C, k, stride, prologue, out_slice)
POOL_CASES = [(2, 16, 16, 32, 2, 2, True, False), (2, 15, 17, 8, 2, 2, True, True), (1, 13, 11, 12, 3, 2, True, False),
              (2, 9, 10, 4, 3, 3, False, True), (1, 7, 7, 16, 3, 1, True, True), (3, 32, 32, 128, 2, 2, True, True)]


@pytest.mark.parametrize('case', POOL_CASES)
@pytest.mark.parametrize('bf16', [False, True])
def test_avgpool(ops, case, bf16):
    N, H, W, C, k, s, prologue, out_slice = case
    rng = np.random.default_rng(H * 31 + C + k)
    q = O.bf16_round if bf16 else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    rel = 2.0 ** -6 if bf16 else 1e-6      # bf16: a prologue value at a rounding boundary + the rounding of the store
    dt = torch.bfloat16 if bf16 else torch.float32
    fwd, bwd = (ops.avgpool2d_fwd_bf16, ops.avgpool2d_bwd_bf16) if bf16 else (ops.avgpool2d_fwd, ops.avgpool2d_bwd)
    z = q(rng.standard_normal((N, H, W, C)))
    sc, sh = q(rng.uniform(0.5, 1.5, C)), q(rng.standard_normal(C) * 0.3)
    a = q(np.maximum(z * sc + sh, 0.0)) if prologue else z
    want = avgpool2d_fwd(a, k, s)
    Ho, Wo = want.shape[1:3]
    kw = dict(in_scale=_t(sc), in_shift=_t(sh), in_act=ops.ACT_RELU) if prologue else {}
    wide = None
    if out_slice:       # the result lands in channels [4, 4 + C) of a wider buffer; the rest stays untouched
        wide = torch.full((N, Ho, Wo, C + 8), 7.0, dtype=dt, device=DEV)
        kw['out'] = wide[..., 4:4 + C]
    got = fwd(_t(z, dt), k, s, **kw)
    tol = rel * (np.abs(want) + np.abs(want).max()) + 1e-30
    assert np.all(np.abs(_np(got) - want) <= tol), float(np.abs(_np(got) - want).max())
    if wide is not None:
        rest = torch.cat([wide[..., :4], wide[..., 4 + C:]], -1)
        assert bool((rest == 7.0).all())
    gy = q(rng.standard_normal(want.shape))
    gref = avgpool2d_bwd(gy, (N, H, W, C), k, s)
    g1 = bwd(_t(gy, dt), (N, H, W, C), k, s)
    g2 = bwd(_t(gy, dt), (N, H, W, C), k, s)
    tol = rel * (np.abs(gref) + np.abs(gref).max()) + 1e-30
    assert np.all(np.abs(_np(g1) - gref) <= tol), float(np.abs(_np(g1) - gref).max())
    assert torch.equal(g1, g2)                                     # gather form: deterministic
    # rows / columns no window covers (floor-sized output) have zero gradient
    assert bool((g1[:, (Ho - 1) * s + k:] == 0).all()) and bool((g1[:, :, (Wo - 1) * s + k:] == 0).all())
    base = q(rng.standard_normal((N, H, W, C + 4)))
    acc = _t(base, dt)
    bwd(_t(gy, dt), (N, H, W, C), k, s, out=acc[..., :C], accumulate=True)
    want_acc = base.copy()
    want_acc[..., :C] += gref
    tol = rel * (np.abs(want_acc) + np.abs(want_acc).max())
    assert np.all(np.abs(_np(acc) - want_acc) <= tol)


def test_avgpool_rejects_bad_geometry(ops):
    x = torch.zeros((1, 8, 8, 4), device=DEV)
    with pytest.raises(Exception):
        ops.avgpool2d_fwd(x, 4, 2)                  # k up to 3
    with pytest.raises(Exception):
        ops.avgpool2d_fwd(torch.zeros((1, 8, 8, 6), device=DEV), 2, 2)     # C a multiple of 4


def _pair(mt, H, W, C, OS):
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model(mt, C, (H, W), OS)
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    o = PeleeOracle(mt, C, (H, W), OS)
    rng = np.random.default_rng(42)
    for k, v in o.net.params.items():
        if k.endswith('/gamma'):
            v[...] = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith('/beta') or k.endswith('/moving_mean'):
            v[...] = rng.standard_normal(v.shape) * 0.1
        elif k.endswith('/moving_variance'):
            v[...] = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith('/bias'):
            v[...] = rng.standard_normal(v.shape) * 0.1
    m.set_weights_by_name(dict(o.net.params))
    return m, o


@pytest.mark.parametrize('mt', ['peleenet', 'peleenet_lite'])
@pytest.mark.parametrize('OS', [8, 16])
def test_predict_matches_restatement(mt, OS):
    pkg = load_pkg()
    H = W = 64
    m = pkg.get_deeplabv3p_model(mt, 21, (H, W), OS, training=False)
    _, o = _pair(mt, H, W, 21, OS)
    m.set_weights_by_name(dict(o.net.params))
    x, _ = _data(2, H, W, 21)
    p = m.predict(x)
    _, p_ref = o.predict(x)
    assert p.shape == (2, H, W, 21)
    assert np.abs(p - p_ref).max() < TOL


@pytest.mark.parametrize('mt', ['peleenet', 'peleenet_lite'])
@pytest.mark.parametrize('OS', [8, 16])
@pytest.mark.parametrize('narrow', ['1', '0'])
def test_train_step_matches_restatement(mt, OS, narrow, monkeypatch):
    """one SGD step against float64 with the ReLU branch pattern of the float32 run injected (as
    tests/test_model_gpu.py::test_train_step_matches_oracle), with the dense layers' 3x3 convs on either route:
    the direct narrow kernels (DL3P_NARROW_CONV=1, csrc/conv_narrow.hip) or the implicit GEMM (0)"""
    _train_step_vs_restatement(mt, OS, narrow, 64, 64, monkeypatch)


@pytest.mark.parametrize('OS', [8, 16])
@pytest.mark.parametrize('narrow', ['1', '0'])
def test_train_step_matches_restatement_ragged(OS, narrow, monkeypatch):
    """the same step at 72 x 104: block 1 is 18 x 26 (the narrow kernels' 8 x 16 tiles ragged both ways), block 2 9 x 13, the OS-16
    transition pooling floors 9 x 13 to 4 x 6 (a row and a column no window covers: zero gradient) and the ASPP rates exceed the map"""
    _train_step_vs_restatement('peleenet', OS, narrow, 72, 104, monkeypatch)


def _train_step_vs_restatement(mt, OS, narrow, H, W, monkeypatch):
    monkeypatch.setenv('DL3P_NARROW_CONV', narrow)
    N, C = 2, 21
    m, o = _pair(mt, H, W, C, OS)
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=3)
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    dense = [op for op in m.graph.ops if op.kind == 'conv_dense' and '_denselayer' in op.name]
    assert len(dense) == 63 and all(ex._narrow(op) == (narrow == '1') for op in dense)
    drop = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0][0]
    mask = ex.dropout_mask(drop).cpu().numpy()
    o.net.act_derivs = relu_derivs(m, ex, load_pkg('ops'))
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
    gtol = 1e-2        # 104 BatchNorm layers in front of the head, as deep as Xception's chain
    assert worst[1] < gtol, worst
    assert o.net.flip_count <= max(8, 2e-4 * o.net.flip_total), (o.net.flip_count, o.net.flip_total)
    grads = {k: v.copy() for k, v in o.net.grads.items()}
    o.sgd_step(0.01, 0.9)
    for k, v in m.get_weights_by_name().items():
        lim = TOL * max(1.0, np.abs(o.net.params[k]).max())
        if k in grads:
            lim += 0.01 * gtol * np.abs(grads[k]).max()
        assert np.abs(v - o.net.params[k]).max() < lim, k


@pytest.mark.parametrize('mt', ['peleenet', 'peleenet_lite'])
def test_graph_replay_equals_eager(mt):
    N, C, H, W = 2, 21, 64, 64
    ma, _ = _pair(mt, H, W, C, 16)
    mb, _ = _pair(mt, H, W, C, 16)
    ma.use_graphs, mb.use_graphs = False, True
    la, lb = [], []
    for s in range(3):
        x, y = _data(N, H, W, C, seed=10 + s)
        la.append(ma.train_on_batch(x, y))
        lb.append(mb.train_on_batch(x, y))
    assert mb._executor(N, True).graphed
    assert np.allclose(la, lb, rtol=1e-5, atol=1e-6), (la, lb)
    wa, wb = ma.get_weights_by_name(), mb.get_weights_by_name()
    assert max(float(np.abs(wa[k] - wb[k]).max()) for k in wa) < 1e-5


def test_bf16_step_close_to_fp32():
    """mixed_bfloat16 trains PeleeNet (AveragePooling2D has its bf16 pair): one step at 256 x 256 against the fp32 step from the
    same weights -- loss to the 1e-2 relative the mixed path keeps on whole steps, finite weights"""
    pkg = load_pkg()
    mp = pkg.mixed_precision
    N, C, H, W = 2, 21, 256, 256
    x, y = _data(N, H, W, C, seed=7)
    m32 = pkg.get_deeplabv3p_model('peleenet', C, (H, W), 16)
    m32.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    w0 = m32.get_weights_by_name()
    l32 = m32.train_on_batch(x, y)
    del m32
    torch.cuda.empty_cache()
    mp.set_policy(mp.Policy('mixed_bfloat16'))
    try:
        mb = pkg.get_deeplabv3p_model('peleenet', C, (H, W), 16)
    finally:
        mp.set_policy(mp.Policy('float32'))
    mb.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    mb.set_weights_by_name(w0)
    assert any(op.kind == 'avgpool' for op in mb.graph.ops)
    lb = mb.train_on_batch(x, y)
    # the loss of a whole bf16 step moves with every rounding of ~200 layers: a loose bound, only against a broken path
    assert np.isfinite(lb) and abs(lb - l32) < 1e-2 * max(1.0, abs(l32)), (lb, l32)
    # the pooling itself, inside the bf16 graph, on the device's own inputs: act(BN(z)) rounded to bf16, then the mean (a wrong
    # scale or a missed tap is an O(1) error here)
    ex = mb._executor(N, True)
    for op in [op for op in mb.graph.ops if op.kind == 'avgpool']:
        v = op.x
        z = _np(ex.view(v.tensor))
        sc = _np(ex.gscale[v.group.id][v.goff:v.goff + v.tensor.C])
        sh = _np(ex.gshift[v.group.id][v.goff:v.goff + v.tensor.C])
        want = avgpool2d_fwd(O.bf16_round(np.maximum(z * sc + sh, 0.0)), op.k, op.stride)
        got = _np(ex.view(op.out))
        assert np.all(np.abs(got - want) <= 2.0 ** -6 * (np.abs(want) + np.abs(want).max())), op.name
    assert all(np.isfinite(v).all() for v in mb.get_weights_by_name().values())


def test_full_size_step_is_finite():
    pkg = load_pkg()
    N, C, H, W = 16, 21, 512, 512
    m = pkg.get_deeplabv3p_model('peleenet', C, (H, W), 16)
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    x, y = _data(N, H, W, C, seed=1)
    loss = m.train_on_batch(x, y)
    assert np.isfinite(loss) and abs(loss - np.log(C)) < 1.0, loss
    del m
    torch.cuda.empty_cache()
