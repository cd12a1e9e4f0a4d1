"""The U-Net family on the MI355X: predict and one SGD step against the float64 restatement (tests/unet_oracle.py), hipGraph replay
against eager, the channel pads, evaluation against the host argmax, the head ops with logits already at full resolution, and
one full-size step.  Bounds: TOL = 1e-3 (tests/peleenet_oracle.py) on probabilities and loss, 1e-2 in relative L2 on every
trainable gradient, at most max(8, 2e-4 total) injected ReLU branch flips -- the conditions of tests/test_ghostnet_gpu.py.
At 32 x 32 the maps go 32 -> 2: the 1024-channel bottleneck is a 2 x 2 map."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from oracle import np_ops as O
from unet_oracle import UNetOracle, TOL, GPU_CASE, data as _data, relu_derivs, randomise

pytestmark = pytest.mark.gpu
TYPES = ('unet_standard', 'unet_lite')
DEV = 'cuda'


def _pair(mt, H, W, C=21, training=True):
    pkg = load_pkg()
    m = pkg.get_unet_model(mt, C, (H, W), training=training)
    if training:
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    o = UNetOracle(mt, C, (H, W))
    randomise(o)
    m.set_weights_by_name(dict(o.net.params))
    return m, o


def _pads_are_zero(m):
    """pad rows / columns of every channel-padded kernel or bias: exactly 0 in the weights, the gradient and the momentum"""
    st = m._store
    n = 0
    for p in m.graph.all_params():
        if p.dev_shape == p.shape:
            continue
        logical = st._pad(p, np.ones(p.shape, np.float32)).reshape(-1)
        if logical.all():
            continue                    # (a dense kernel stored as its GEMM operand with nothing to pad)
        for buf in (st.P, st.G, st.V):
            dev = st.view(p, buf).detach().cpu().numpy().reshape(-1)
            assert not dev[logical == 0].any(), p.name
        n += 1
    return n


@pytest.mark.parametrize('mt,H,W', [('unet_standard', 32, 32), ('unet_lite', 32, 32), ('unet_lite', 48, 80)])
def test_predict_matches_restatement(mt, H, W):
    m, o = _pair(mt, H, W, training=False)
    x, _ = _data(2, H, W, 21)
    p = m.predict(x)
    _, p_ref = o.predict(x)
    assert p.shape == (2, H, W, 21)
    err = np.abs(p - p_ref).max()
    print('max |p - p_ref|', err)
    assert err < TOL
    # evaluation on the device agrees with the host argmax of predict (ties aside: none at this margin)
    mask = m.predict_mask(x)
    assert mask.shape == (2, H, W)
    top2 = np.sort(p, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-5
    assert clear.mean() > 0.99 and np.array_equal(np.asarray(mask)[clear], p.argmax(-1)[clear])


def _train_step_vs_restatement(mt, H, W):
    N, C = GPU_CASE['N'], GPU_CASE['C']
    m, o = _pair(mt, H, W, C)
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=GPU_CASE['seed'])
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    drops = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0]
    assert len(drops) == 2
    masks = {'dropout': ex.dropout_mask(drops[0]).cpu().numpy(), 'dropout_1': ex.dropout_mask(drops[1]).cpu().numpy()}
    o.net.act_derivs = relu_derivs(m, ex)         # the ReLU branch pattern of the float32 run goes into the restatement
    total, ce, logits = o.loss_and_grads(x, y, masks)
    print('loss', loss, 'reference', ce)
    assert abs(loss - ce) < TOL * max(1.0, abs(ce)), (loss, ce)
    st = m._store
    worst = ('', 0.0)
    for p in m.graph.all_params():
        assert p.trainable
        g = st.get(p, st.G)
        gref = o.net.grads[p.name]
        assert np.abs(gref).max() > 1e-7, p.name           # (tests/test_unet_cpu.py::test_no_reference_gradient_is_dead)
        r = float(np.linalg.norm((g - gref).ravel()) / np.linalg.norm(gref.ravel()))
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
        lim = TOL * max(1.0, np.abs(o.net.params[k]).max()) + 0.01 * gtol * np.abs(grads[k]).max()
        assert np.abs(v - o.net.params[k]).max() < lim, k
    return m


@pytest.mark.parametrize('mt,H,W', [('unet_standard', 32, 32), ('unet_lite', 32, 32), ('unet_lite', 48, 80)])
def test_train_step_matches_restatement(mt, H, W):
    m = _train_step_vs_restatement(mt, H, W)
    # standard: the first kernel's 28th row, Conv2D(2, 3) kernel + bias, classifier kernel + bias; lite: the first layer's two
    # kernels (the image's 4th channel), SeparableConv2D(2, 3) pointwise kernel + bias, classifier kernel + bias
    assert _pads_are_zero(m) == (5 if mt == 'unet_standard' else 6)


@pytest.mark.parametrize('mt', TYPES)
def test_graph_replay_equals_eager_bit_for_bit(mt):
    N, C, H, W = 2, 21, 32, 32
    ma, _ = _pair(mt, H, W, C)
    mb, _ = _pair(mt, H, W, C)
    ma.use_graphs, mb.use_graphs = False, True
    la, lb = [], []
    for s in range(3):
        x, y = _data(N, H, W, C, seed=10 + s)
        la.append(ma.train_on_batch(x, y))
        lb.append(mb.train_on_batch(x, y))
    assert mb._executor(N, True).graphed and not ma._executor(N, True).graphed
    assert np.array_equal(np.asarray(la, np.float32).view(np.uint32), np.asarray(lb, np.float32).view(np.uint32)), (la, lb)
    wa, wb = ma.get_weights_by_name(), mb.get_weights_by_name()
    for k in wa:
        assert np.array_equal(wa[k].view(np.uint32), wb[k].view(np.uint32)), k
    assert any(np.abs(wa[k]).max() > 0 for k in wa)
    assert _pads_are_zero(ma) and _pads_are_zero(mb)              # ... after three steps


def test_evaluate_miou_agrees_with_host_argmax():
    """the confusion matrix of evaluate_miou (argmax of the logits on the device) against the host argmax of predict's
    probabilities.  A pixel whose two best classes are within an ulp can fall either way between logits and rounded
    probabilities: at most 2 of the 2048 pixels may differ (each moves two counters)"""
    pkg = load_pkg()
    N, C, H, W = 2, 21, 32, 32
    m, _ = _pair('unet_lite', H, W, C, training=False)
    x, y = _data(N, H, W, C, seed=5)
    lab = y.reshape(N, H, W).astype(np.int64)
    res = m.evaluate_miou([(x, y)], steps=1)
    pred = m.predict(x).argmax(-1)
    cm = np.zeros((C, C), np.int64)
    keep = lab != 255
    np.add.at(cm, (lab[keep], pred[keep]), 1)
    got = np.asarray(res['confusion_matrix'], np.int64)
    assert got.sum() == keep.sum() and np.abs(got - cm).sum() <= 4, np.abs(got - cm).sum()
    if np.array_equal(got, cm):
        assert res['mIoU'] == pkg.miou_from_confusion(cm)['mIoU']


@pytest.mark.parametrize('C', [21, 2])
def test_head_ops_with_logits_at_full_resolution(ops, C):
    """h == H, w == W (the U-Net head: no pred_resize): loss, probabilities, gradient, argmax and the fused training heads where
    their _supported says yes, against the float64 head"""
    rng = np.random.default_rng(C)
    N, H, W = 2, 16, 48
    cp = (C + 3) // 4 * 4
    z = np.zeros((N, H, W, cp))
    z[..., :C] = rng.standard_normal((N, H, W, C)) * 3
    lab = rng.integers(0, C, (N, H, W)).astype(np.float64)
    lab[rng.uniform(size=lab.shape) < 0.1] = 255
    loss_ref, p_ref, g_ref = O.loss_fwd_bwd(z[..., :C], lab, None, 255)
    zt = torch.from_numpy(z.astype(np.float32)).to(DEV)
    labels = torch.from_numpy(lab.reshape(N, H * W, 1).astype(np.float32)).to(DEV)
    out = ops.upsample_softmax_ce(zt, C, H, W, labels, 255, want_probs=True, want_logits=True, want_grad=True)

    def close(got, want, rtol, atol, what):
        got = got.detach().cpu().numpy().astype(np.float64)
        want = np.asarray(want, np.float64)
        scale = max(1.0, float(np.abs(want).max()))
        assert got.shape == want.shape and np.abs(got - want).max() <= (atol + rtol) * scale, what
    assert torch.equal(out['logits'][..., :C], zt[..., :C])            # an identity resize moves no value
    close(out['probs'], p_ref, 1e-4, 1e-6, 'probs')
    close(out['loss'], [loss_ref], 1e-4, 2e-5, 'loss')
    close(out['dlogits'][..., :C], g_ref, 1e-4, 1e-9, 'dlogits')
    assert C == cp or float(out['dlogits'][..., C:].abs().max()) == 0.0
    pred, cm = ops.argmax_confusion(zt, C, H, W, labels)
    want = z[..., :C].astype(np.float32).argmax(-1)
    assert np.array_equal(ops.argmax_confusion(zt, C, H, W, want_mask=True)[0].cpu().numpy(), want)
    ref_cm = np.zeros((C, C), np.int64)
    keep = lab != 255
    np.add.at(ref_cm, (lab[keep].astype(np.int64), want[keep]), 1)
    assert np.array_equal(cm.cpu().numpy(), ref_cm)
    for rows_form, supported in ((False, ops.head_train_supported), (True, ops.head_train_rows_supported)):
        if supported(H, W, C, H, W):
            loss, gz = ops.head_train(zt, C, H, W, labels, 255, rows_form=rows_form)
            close(loss, [loss_ref], 1e-4, 2e-5, 'fused loss')
            close(gz[..., :C], g_ref, 1e-4, 1e-9, 'fused gradient')
            assert C == cp or float(gz[..., C:].abs().max()) == 0.0


def test_full_size_lite_step():
    """1 x 512 x 512 unet_lite: build, train, a finite first loss within 20 % of ln 21, eager == graph bit for bit (two steps: the
    second one is the captured graph's first replay).  The size works; parity is the small cases' business"""
    pkg = load_pkg()
    N, C, H, W = 1, 21, 512, 512
    x, y = _data(N, H, W, C, seed=1)
    losses = []
    for graphs in (False, True):
        m = pkg.get_unet_model('unet_lite', C, (H, W), seed=0)
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        m.use_graphs = graphs
        losses.append([m.train_on_batch(x, y), m.train_on_batch(x, y)])
        assert m._executor(N, True).graphed == graphs
        del m
        torch.cuda.empty_cache()
    print('losses', losses)
    assert np.isfinite(losses[0]).all() and abs(losses[0][0] - np.log(C)) < 0.2 * np.log(C), losses
    assert np.array_equal(np.asarray(losses[0], np.float32).view(np.uint32), np.asarray(losses[1], np.float32).view(np.uint32)), losses
