"""The Fast-SCNN family on the MI355X against its literal float64 restatement (tests/fast_scnn_oracle.py): predict and one SGD step at
256 x 256, 256 x 320 (rectangular pooling windows) and 288 x 256 (a pooling row no window covers), hipGraph replay against eager,
evaluation against the host argmax, one full-size step.  Bounds as in tests/test_unet_gpu.py: TOL = 1e-3 on probabilities and loss,
1e-2 in relative L2 on every trainable gradient.  Gradients are compared WITH their l2 term (the product adds 2 l2 w in the optimiser,
the restatement differentiates the penalty): the depthwise biases in front of a BatchNorm have no other gradient.  A few betas have none at all (see the test).  The restatement
takes the product's Dropout mask and its ReLU branch pattern; at most max(8, 2e-4 total) branches may differ."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from fast_scnn_oracle import FastSCNNOracle, TOL, data as _data

pytestmark = pytest.mark.gpu
SIZES = [(256, 256), (256, 320), (288, 256)]
# Betas with NO gradient, by architecture: the last BatchNorm of each bottleneck of the 64- and 96-channel groups (its output reaches,
# through the residual Adds too, nothing but 1x1 convs in front of another training-mode BatchNorm, which removes any per-channel
# constant) and the BatchNorm of the feature-fusion 1x1 conv (an Add, then a BatchNorm).  The 128-channel group's outputs reach the
# zero-padded 3x3 convs of the pyramid pooling block and the fusion conv: live.
DEAD_BETAS = frozenset('batch_normalization_%d/beta' % i for i in (5, 8, 11, 14, 17, 20, 30))


def _pair(H, W, C=21, training=True, mv='biased'):
    pkg = load_pkg()
    m = pkg.get_fast_scnn_model('fast_scnn', C, (H, W), training=training, bn_moving_variance=mv)
    if training:
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    o = FastSCNNOracle(C, (H, W))
    o.moving_variance = mv
    if mv == 'unbiased':
        # moving variances start at 0: after one step they are (1 - momentum) x the batch variance x Bessel's factor, so the factor
        # shows at fp32 resolution (behind a moving variance near 1 a wrong count moves the result by less than 1e-5)
        o.params = {k: (v * 0 if k.endswith('moving_variance') else v) for k, v in o.params.items()}
    m.set_weights_by_name({k: v.astype(np.float32) for k, v in o.params.items()})
    o.params = {k: v.astype(np.float64) for k, v in m.get_weights_by_name().items()}     # both start from the same fp32 numbers
    return m, o


@pytest.mark.parametrize('H,W', SIZES)
def test_predict_matches_restatement(H, W):
    m, o = _pair(H, W, training=False)
    x, _ = _data(2, H, W, 21)
    p = m.predict(x)
    p_ref = o.predict(x)
    assert p.shape == (2, H, W, 21)
    err = np.abs(p - p_ref).max()
    print('max |p - p_ref|', err)
    assert err < TOL
    mask = m.predict_mask(x)
    top2 = np.sort(p, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-5
    assert clear.mean() > 0.99 and np.array_equal(np.asarray(mask)[clear], p.argmax(-1)[clear])


def _relu_pattern(m, ex):
    """{BatchNorm name: 1 where the ReLU behind it passed the element in the float32 run}"""
    ops = load_pkg('ops')
    out = {}
    for bn in m.graph.bns:
        if bn.act == ops.ACT_RELU:
            sc = ex.gscale[bn.group.id][bn.offset:bn.offset + bn.C]
            sh = ex.gshift[bn.group.id][bn.offset:bn.offset + bn.C]
            out[bn.name] = (ops.affine_act(ex.view(bn.z), sc, sh, bn.act) > 0).cpu().numpy()
    return out


@pytest.mark.parametrize('H,W,mv', [s + ('biased',) for s in SIZES] + [SIZES[0] + ('unbiased',)])
def test_train_step_matches_restatement(H, W, mv):
    N, C = 2, 21
    m, o = _pair(H, W, C, mv=mv)
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=3)
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    drops = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0]
    assert len(drops) == 1
    mask = ex.dropout_mask(drops[0]).cpu().numpy().reshape(N, H // 8, W // 8, -1)[..., :C]
    o.act_derivs = _relu_pattern(m, ex)
    assert len(o.act_derivs) == 25
    ce = o.loss_and_grads(x, y, mask)
    print('loss', loss, 'reference', ce)
    assert abs(loss - ce) < TOL * max(1.0, abs(ce)), (loss, ce)
    st = m._store
    w0 = {k: v.astype(np.float64) for k, v in o.params.items()}
    worst, dead = ('', 0.0), []
    for p in m.graph.all_params():
        if not p.trainable:
            continue
        assert p.l2 == np.float32(o.l2_of(p.name)) or abs(p.l2 - o.l2_of(p.name)) < 1e-12, p.name
        g = st.get(p, st.G).astype(np.float64) + 2.0 * p.l2 * w0[p.name]
        gref = o.grads[p.name]
        if p.name in DEAD_BETAS:
            # exactly 0: float64 rounding noise in the restatement, a sum that cancels in fp32 in the product -- noise far below
            # every live gradient here
            dead.append(p.name)
            assert np.abs(gref).max() < 1e-12, (p.name, np.abs(gref).max())
            assert np.abs(g).max() < 1e-6, (p.name, np.abs(g).max())
            continue
        assert np.abs(gref).max() > 1e-7, p.name
        r = float(np.linalg.norm((g - gref).ravel()) / np.linalg.norm(gref.ravel()))
        if r > worst[1]:
            worst = (p.name, r)
    print('worst gradient', worst, 'betas with no gradient', dead)
    assert sorted(dead) == sorted(DEAD_BETAS)
    print('flips', o.flip_count, o.flip_total)
    assert o.flip_count <= max(8, 2e-4 * o.flip_total), (o.flip_count, o.flip_total)
    assert worst[1] < 1e-2, worst
    grads = dict(o.grads)
    o.sgd_step(0.01, 0.9, moving_variance=mv)     # (the restatement's counts are the literal ones: its tensors are)
    w1 = m.get_weights_by_name()
    for k, v in w1.items():
        lim = TOL * max(1.0, np.abs(o.params[k]).max()) + 1e-4 * (np.abs(grads[k]).max() if k in grads else 0.0)
        assert np.abs(v - o.params[k]).max() < lim, k
    # the moving statistics on their own, tighter: a wrong element count or a lost depthwise bias shows here
    for k, v in w1.items():
        if k.endswith(('moving_mean', 'moving_variance')):
            assert np.abs(v - o.params[k]).max() < 1e-5 * max(1.0, np.abs(o.params[k]).max()), k
        if mv == 'unbiased' and k.endswith('moving_variance'):
            # per element, relative: the fp32 sums behind a batch variance carry a few hundred roundings per thread (about 1.5e-5) on
            # sum and sum of squares, times 1 + mean^2 / var in the difference -> 1e-4.  N (H/32) (W/32) = 128 in place of the literal
            # N (H/8) (W/8) = 2048 elements would move batch_normalization_31 by 7.3e-3, the biased variance by 4.9e-4
            rel = np.abs(v - o.params[k]) / np.abs(o.params[k])
            assert rel.max() < 1e-4, (k, rel.max())


def test_graph_replay_equals_eager_bit_for_bit():
    N, C, H, W = 2, 21, 256, 256
    ma, _ = _pair(H, W, C)
    mb, _ = _pair(H, W, C)
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
    # the biases a training-mode BatchNorm cancels: no launch writes their gradient, it is still exactly 0 after three steps
    for m in (ma, mb):
        ex, st = m._executor(N, True), m._store
        quiet = [op for op in m.graph.ops if getattr(op, 'b', None) is not None and ex._bias_grad(op) is None]
        assert len(quiet) == 27 and all(not st.get(op.b, st.G).any() for op in quiet)


def test_evaluate_miou_agrees_with_host_argmax():
    """at most 2 pixels whose two best classes tie within an ulp may differ (each moves two counters), as in the U-Net test"""
    pkg = load_pkg()
    N, C, H, W = 2, 21, 256, 256
    m, _ = _pair(H, W, C, training=False)
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


def test_losses_weights_and_metric_run_through_the_nearest_head():
    """the focal loss with sample weights and the Jaccard metric: the step runs and the loss is finite (the head's numbers
    are tests/test_fast_scnn_ops_gpu.py's business)"""
    pkg = load_pkg()
    N, C, H, W = 1, 5, 256, 256
    m = pkg.get_fast_scnn_model('fast_scnn', C, (H, W))
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseSoftmaxFocalLoss(), metrics=[pkg.Jaccard], sample_weight_mode='temporal')
    x, y = _data(N, H, W, C, seed=7)
    out = m.train_on_batch(x, y, sample_weight=np.full((N, H * W), 0.5, np.float32))
    assert np.all(np.isfinite(np.asarray(out, np.float64)))


def test_full_size_step():
    pkg = load_pkg()
    N, C, H, W = 1, 21, 512, 512
    x, y = _data(N, H, W, C, seed=1)
    losses = []
    for graphs in (False, True):
        m = pkg.get_fast_scnn_model('fast_scnn', C, (H, W), seed=0)
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        m.use_graphs = graphs
        losses.append([m.train_on_batch(x, y), m.train_on_batch(x, y)])
        assert m._executor(N, True).graphed == graphs
        del m
        torch.cuda.empty_cache()
    print('losses', losses)
    assert np.isfinite(losses[0]).all() and abs(losses[0][0] - np.log(C)) < 0.2 * np.log(C), losses
    assert np.array_equal(np.asarray(losses[0], np.float32).view(np.uint32), np.asarray(losses[1], np.float32).view(np.uint32)), losses
