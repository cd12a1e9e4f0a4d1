"""Parity at the PRODUCTION shapes and with the PRODUCTION dispatch ("what's weak" 2).

The other GPU parity tests run at 65x65 / 97x97 with `pw_small_min_rows` lowered so that small shapes reach the
streaming GEMM kernels.  The kernels that carry the headline number -- the tiled GEMM over thousands of row tiles,
`pw_wgrad_kernel` slabs, the depthwise row-band splits at 257x257 / 129x129, the XCD chunking and the rate-18 lattice
kernel at batch 16 -- run a different dispatch at BASELINE.json configs[1].  Here:

  * whole-model train step + predict of `mobilenetv2` / `mobilenetv2_lite` at 513x513 (batch 2: the fp64 oracle
    needs about a minute per step on 8 cores) with the production threshold restored,
  * the ten costliest launches of profiles/r01_step_table_mobilenetv2.txt at their exact configs[1] shapes
    (batch 16) against float64 NumPy.
"""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from layer_walk import _taps
from oracle import np_ops as O
from oracle.np_net import OracleModel

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def production_dispatch():
    L = load_pkg('_lib').lib()
    L.set_option(b'pw_small_min_rows', -1)        # production threshold (2^17 rows)
    yield
    L.set_option(b'pw_small_min_rows', 64)        # what conftest.py sets for the small-shape tests


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def rel(got, want):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(1e-30, np.abs(want).max()))


# ------------------------------------------------------------------------------------------- whole model, 513 x 513
# (+ Xception, BASELINE configs[2]: the fp64 oracle needs ~50 s per image for it on 8 cores)
@pytest.mark.parametrize('model_type', ['mobilenetv2', 'mobilenetv2_lite', 'xception'])
def test_train_step_513_production_dispatch(model_type):
    from test_model_gpu import _pair, _data, _act_derivs, _act_derivs_seq, _rel
    N, C, H, W = 2, 21, 513, 513
    m, o = _pair(model_type, H, W, C)
    m.use_graphs = False
    x, y = _data(N, H, W, C, seed=11)
    loss = m.train_on_batch(x, y)
    ex = m._executor(N, True)
    drop = [op for op in m.graph.ops if op.kind == 'materialize' and op.rate > 0][0]
    mask = ex.dropout_mask(drop).cpu().numpy()
    o.net.act_derivs = _act_derivs(m, ex, o.net.params)
    o.net.act_derivs_seq = _act_derivs_seq(m, ex, o.net.act_derivs)
    total, ce, logits_ref = o.loss_and_grads(x, y, {'aspp_dropout': mask})
    assert abs(loss - ce) < 1e-3 * max(1.0, abs(ce)), (loss, ce)
    # north_star: per-pixel class logits within 1e-3 (training-mode BN, the same dropout mask)
    ops = load_pkg('ops')
    out = ops.upsample_softmax_ce(ex.view(m.head.tensor), C, H, W, want_logits=True)
    lg = out['logits'][..., :C].cpu().numpy()
    assert np.abs(lg - logits_ref).max() < 1e-3 * max(1.0, np.abs(logits_ref).max())
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
    assert worst[1] < 5e-3, worst
    o.sgd_step(0.01, 0.9)
    w = m.get_weights_by_name()
    for k, v in w.items():
        assert np.abs(v - o.net.params[k]).max() < 1e-3 * max(1.0, np.abs(o.net.params[k]).max()), k
    # predict (inference BN from the updated moving statistics) with the same weights
    pkg = load_pkg()
    mi = pkg.get_deeplabv3p_model(model_type, C, (H, W), 16, training=False)
    mi.set_weights_by_name(w)
    p = mi.predict(x[:1])
    _, p_ref = o.predict(x[:1])
    assert np.abs(p - p_ref).max() < 1e-3


# ------------------------------------------------------------------------------------------- configs[1] launches
# (M, K, N) of the pointwise convolutions at batch 16, 513 x 513: decoder_conv0 / decoder_conv1 (129 x 129 maps),
# expanded_conv_1_expand / expanded_conv_1_project (257 x 257 -> tiled + streaming kernels), feature_projection0,
# concat_projection (33 x 33, K = 1280) and the 21-class head (N padded to 24)
PW_PROD = [(16 * 129 * 129, 304, 256), (16 * 129 * 129, 256, 256), (16 * 257 * 257, 16, 96), (16 * 257 * 257, 96, 24),
           (16 * 129 * 129, 24, 48), (16 * 33 * 33, 1280, 256), (16 * 129 * 129, 256, 24), (16 * 33 * 33, 960, 160),
           # BASELINE configs[2] / [3] / [4] at their per-GPU launch shapes: Xception 513 x 513 batch 4
           # (33 x 33 maps: middle flow 728 -> 728, exit flow 1536 -> 2048, ASPP 2048 -> 256, concat 1280 -> 256; decoder
           # 129 x 129), Xception 769 x 769 OS 8 batch 2 (97 x 97 and 193 x 193 maps), MobileNetV3-Large 1024 x 2048 batch 1
           # in fp32 (decoder 256 x 512 x 304 -> 256)
           (4 * 33 * 33, 728, 728), (4 * 33 * 33, 1536, 2048), (4 * 33 * 33, 2048, 256), (4 * 33 * 33, 1280, 256),
           (4 * 129 * 129, 304, 256), (4 * 65 * 65, 256, 728), (2 * 97 * 97, 728, 728), (2 * 97 * 97, 2048, 256),
           (2 * 97 * 97, 1536, 2048), (2 * 193 * 193, 304, 256), (2 * 193 * 193, 256, 20), (256 * 512, 304, 256),
           (256 * 512, 256, 20), (64 * 128, 960, 160)]


@pytest.mark.parametrize('case', PW_PROD)
def test_pointwise_at_config1_shapes(ops, case):
    M, K, Nn = case
    rng = np.random.default_rng(M % 1000 + K * 3 + Nn)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, Nn)) / np.sqrt(K)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, K).astype(np.float32)
    sh = (rng.standard_normal(K) * 0.3).astype(np.float32)
    a = O.act_fwd(x.astype(np.float64) * sc + sh, O.ACT_RELU6)
    y_ref = a @ w.astype(np.float64)
    part = ops.new_partials(Nn, DEV)
    xt, wt = T(x), T(w)
    y, rows = ops.pwconv_fwd(xt, wt, None, T(sc), T(sh), ops.ACT_RELU6, partials=part)
    assert rel(y, y_ref) < 2e-5, 'forward'
    p = part[:rows * 2 * Nn].reshape(rows, 2, Nn).double().sum(0).cpu().numpy()
    assert rel(p[0], y_ref.sum(0)) < 1e-4 + 1e-4 * np.sqrt(M) / max(1.0, np.abs(y_ref.sum(0)).max()), 'stat sum'
    assert rel(p[1], (y_ref ** 2).sum(0)) < 1e-4, 'stat sum of squares'
    # transposed-kernel forward: the path the executor launches
    y2, _ = ops.pwconv_fwd_wt(xt, T(np.ascontiguousarray(w.T)), None, T(sc), T(sh), ops.ACT_RELU6,
                              partials=ops.new_partials(Nn, DEV))
    assert rel(y2, y_ref) < 2e-5, 'forward (transposed kernel)'
    del y, y2, xt
    gy = rng.standard_normal((M, Nn)).astype(np.float32)
    gyt = T(gy)
    gx = ops.pwconv_bwd_data(gyt, wt)
    gx_ref = gy.astype(np.float64) @ w.astype(np.float64).T
    assert rel(gx, gx_ref) < 2e-5, 'data gradient'
    # data gradient with the fused BatchNorm-backward sums (what the executor launches behind a BN + activation)
    z = rng.standard_normal((M, K)).astype(np.float32)
    mean, invstd = z.mean(0), 1.0 / np.sqrt(z.var(0) + 1e-3)
    part = ops.new_partials(K, DEV)
    gx2, rows = ops.pwconv_bwd_data_bn(gyt, wt, T(z), T(sc), T(sh), ops.ACT_RELU6, T(mean), T(invstd), part)
    assert rel(gx2, gx_ref) < 2e-5, 'data gradient (+BN sums)'
    u = z.astype(np.float64) * sc + sh
    d = gx_ref * ((u > 0) & (u < 6))
    xh = (z.astype(np.float64) - mean) * invstd
    p = part[:rows * 2 * K].reshape(rows, 2, K).double().sum(0).cpu().numpy()
    assert np.abs(p[0] - d.sum(0)).max() < 2e-4 * np.abs(d).sum(0).max(), 'BN backward sum'
    assert np.abs(p[1] - (d * xh).sum(0)).max() < 2e-4 * np.abs(d * xh).sum(0).max(), 'BN backward sum * xhat'
    del gx, gx2, u, d, xh, z
    gw, gb = ops.pwconv_bwd_weight(T(x), gyt, T(sc), T(sh), ops.ACT_RELU6, with_bias=True)
    gw_ref = a.T @ gy.astype(np.float64)
    # M = 266 256 .. 1 056 784 products per entry: fp32 accumulation in fixed-order slabs
    assert np.abs(gw.cpu().numpy() - gw_ref).max() < 3e-5 * np.sqrt(M) * max(1.0, float(np.abs(a).max())), 'weight gradient'
    assert rel(gw, gw_ref) < 5e-3, 'weight gradient (relative to the largest entry)'
    assert rel(gb, gy.astype(np.float64).sum(0)) < 1e-3, 'bias gradient'


# (N, H, W, C, k, stride, rate): decoder_conv0_depthwise, expanded_conv_1_depthwise (257 -> 129, stride 2),
# expanded_conv_depthwise (257 x 257 x 32), the three ASPP branches (rate 18 = the roofline kernel) and a rate-2 block
DW_PROD = [(16, 129, 129, 304, 3, 1, 1), (16, 257, 257, 96, 3, 2, 1), (16, 257, 257, 32, 3, 1, 1),
           (16, 33, 33, 320, 3, 1, 18), (16, 33, 33, 320, 3, 1, 12), (16, 33, 33, 320, 3, 1, 6),
           (16, 33, 33, 960, 3, 1, 2), (16, 65, 65, 192, 3, 2, 1),
           # configs[2]: Xception batch 4, the three ASPP rates on 33 x 33 x 2048 (rate 18 = dw_fwd_lattice2 at N = 4), exit flow
           # rate 2, entry flow stride 2; configs[3]: OS 8 batch 2, ASPP 12 / 24 / 36 on 97 x 97 x 2048, middle flow rate 2, exit
           # flow rate 4; configs[4] (fp32 twin): 5 x 5 rate 2 on 64 x 128 x 960, ASPP on 64 x 128 x 160
           (4, 33, 33, 2048, 3, 1, 6), (4, 33, 33, 2048, 3, 1, 12), (4, 33, 33, 2048, 3, 1, 18), (4, 33, 33, 1536, 3, 1, 2),
           (4, 65, 65, 728, 3, 2, 1), (2, 97, 97, 2048, 3, 1, 12), (2, 97, 97, 2048, 3, 1, 24), (2, 97, 97, 2048, 3, 1, 36),
           (2, 97, 97, 728, 3, 1, 2), (2, 97, 97, 1536, 3, 1, 4), (1, 64, 128, 960, 5, 1, 2), (1, 64, 128, 160, 3, 1, 6),
           (1, 64, 128, 160, 3, 1, 12), (1, 64, 128, 160, 3, 1, 18)]


@pytest.mark.parametrize('case', DW_PROD)
def test_depthwise_at_config1_shapes(ops, case):
    N, H, W, C, k, s, r = case
    rng = np.random.default_rng(H * 7 + C + r)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((k, k, C)) * 0.3).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, C).astype(np.float32)
    sh = (rng.standard_normal(C) * 0.3).astype(np.float32)
    a = O.act_fwd(x.astype(np.float64) * sc + sh, O.ACT_RELU6)
    y_ref = O.dwconv2d_fwd(a, w.astype(np.float64), s, r, 'same')
    part = ops.new_partials(C, DEV)
    y, rows = ops.dwconv2d_fwd(T(x), T(w), s, r, 'same', T(sc), T(sh), ops.ACT_RELU6, partials=part)
    assert rel(y, y_ref) < 1e-5, 'forward'
    p = part[:rows * 2 * C].reshape(rows, 2, C).double().sum(0).cpu().numpy()
    assert np.abs(p[0] - y_ref.reshape(-1, C).sum(0)).max() < 1e-4 * np.abs(y_ref).reshape(-1, C).sum(0).max(), 'stat sum'
    assert rel(p[1], (y_ref ** 2).reshape(-1, C).sum(0)) < 1e-4, 'stat sum of squares'
    del y
    gy = rng.standard_normal(y_ref.shape).astype(np.float32)
    gx_ref, gw_ref = O.dwconv2d_bwd(a, w.astype(np.float64), gy.astype(np.float64), s, r, 'same')
    gx = ops.dwconv2d_bwd_data(T(gy), T(w), (N, H, W, C), s, r, 'same')
    assert rel(gx, gx_ref) < 1e-5, 'data gradient'
    z = rng.standard_normal((N, H, W, C)).astype(np.float32)
    mean = z.reshape(-1, C).mean(0)
    invstd = 1.0 / np.sqrt(z.reshape(-1, C).var(0) + 1e-3)
    part = ops.new_partials(C, DEV)
    gx2, rows = ops.dwconv2d_bwd_data_bn(T(gy), T(w), (N, H, W, C), T(z), T(sc), T(sh), ops.ACT_RELU6, T(mean), T(invstd),
                                         part, s, r, 'same')
    assert rel(gx2, gx_ref) < 1e-5, 'data gradient (+BN sums)'
    u = z.astype(np.float64) * sc + sh
    d = (gx_ref * ((u > 0) & (u < 6))).reshape(-1, C)
    xh = ((z.astype(np.float64) - mean) * invstd).reshape(-1, C)
    p = part[:rows * 2 * C].reshape(rows, 2, C).double().sum(0).cpu().numpy()
    assert np.abs(p[0] - d.sum(0)).max() < 2e-4 * np.abs(d).sum(0).max(), 'BN backward sum'
    assert np.abs(p[1] - (d * xh).sum(0)).max() < 2e-4 * np.abs(d * xh).sum(0).max(), 'BN backward sum * xhat'
    del gx, gx2, u, d, xh
    gw = ops.dwconv2d_bwd_weight(T(x), T(gy), k, s, r, 'same', T(sc), T(sh), ops.ACT_RELU6)
    M = N * y_ref.shape[1] * y_ref.shape[2]
    assert np.abs(gw.cpu().numpy() - gw_ref).max() < 3e-5 * np.sqrt(M) * max(1.0, float(np.abs(a).max())), 'weight gradient'
    assert rel(gw, gw_ref) < 5e-3, 'weight gradient (relative to the largest entry)'


def test_head_and_resize_at_config1_shapes(ops):
    """pred_resize + softmax + CE (129 -> 513, 21 classes, batch 16) and decoder_resize (33 -> 129, 256 ch)"""
    N, h, w, C, H, W = 16, 129, 129, 21, 513, 513
    rng = np.random.default_rng(9)
    z = (rng.standard_normal((N, h, w, 24)) * 2).astype(np.float32)
    z[..., C:] = 0
    labels = rng.integers(0, C, (N, H, W)).astype(np.float32)
    labels[rng.uniform(size=labels.shape) < 0.05] = 255
    out = ops.upsample_softmax_ce(T(z), C, H, W, labels=T(labels), want_logits=True, want_grad=True)
    # reference on two images (the fp64 softmax of 16 x 513 x 513 x 21 is 0.7 GB per temporary)
    for n in (0, 15):
        lg = O.resize_bilinear_fwd(z[n:n + 1, ..., :C].astype(np.float64), H, W)
        assert np.abs(out['logits'][n, ..., :C].cpu().numpy() - lg[0]).max() < 1e-5 * np.abs(lg).max()
        ce, probs, dl = O.sparse_ce_fwd_bwd(lg, labels[n:n + 1], 255)
        got = out['dlogits'][n, ..., :C].cpu().numpy() * N          # the kernel scales by 1 / (N H W)
        assert np.abs(got - dl[0]).max() < 1e-5 * np.abs(dl).max() + 1e-9
    x = rng.standard_normal((N, 33, 33, 256)).astype(np.float32)
    y = ops.resize_bilinear_fwd(T(x), 129, 129)
    y_ref = O.resize_bilinear_fwd(x.astype(np.float64), 129, 129)
    assert rel(y, y_ref) < 1e-5
    gy = rng.standard_normal((N, 129, 129, 256)).astype(np.float32)
    gx = ops.resize_bilinear_bwd(T(gy), 33, 33)
    assert rel(gx, O.resize_bilinear_bwd(gy.astype(np.float64), 33, 33)) < 1e-5


def test_bn_backward_at_config1_shape(ops):
    """the separate reduce / finalize / apply passes on the largest BN of the step (expanded_conv_1_expand_BN,
    16 x 257 x 257 x 96), channels with |mean| >> sigma included"""
    M, C = 16 * 257 * 257, 96
    rng = np.random.default_rng(21)
    z = rng.standard_normal((M, C)).astype(np.float32)
    z[:, :8] = z[:, :8] * 0.01 + 30.0            # post-ReLU6-like channels: mean 30, sigma 0.01
    g = rng.standard_normal((M, C)).astype(np.float32)
    bn = ops.BNState(C, DEV, eps=1e-3)
    part = ops.new_partials(C, DEV)
    # statistics through a producer: identity 1x1 conv would cost a GEMM; use the reduce of (sum, sum^2) kernels
    zt = T(z)
    y, rows = ops.pwconv_fwd(zt, T(np.eye(C, dtype=np.float32)), partials=part)
    ops.bn_finalize(bn, part, rows, float(M))
    z64 = z.astype(np.float64)
    mean, var = z64.mean(0), z64.var(0)
    assert np.abs(bn.mean.cpu().numpy() - mean).max() < 1e-5 * np.abs(mean).max()
    # E[x^2] - E[x]^2 from float32 partial rows: relative error of the variance grows with (mean/sigma)^2
    invstd_ref = 1.0 / np.sqrt(var + 1e-3)
    assert np.abs(bn.invstd.cpu().numpy()[8:] - invstd_ref[8:]).max() < 1e-4 * invstd_ref[8:].max()
    assert np.abs(bn.invstd.cpu().numpy()[:8] - invstd_ref[:8]).max() < 2e-2 * invstd_ref[:8].max()


@pytest.mark.parametrize('model_type', ['mobilenetv2', 'xception'])
def test_every_layer_at_513_matches_float64_on_the_devices_own_inputs(model_type, monkeypatch):
    """the layer-local comparison of tests/test_model_gpu.py at the production shapes and dispatch: every conv layer's forward,
    its data-gradient + BatchNorm-backward segment and its weight gradient against float64 on the device's own inputs"""
    from test_model_gpu import _teacher_forced_step
    monkeypatch.setenv('DL3P_FOLD_APPLY', '0')
    monkeypatch.setenv('DL3P_GRAD_ALIAS', '0')
    if model_type == 'xception':
        # batch 3 (the float64 oracle needs ~50 s per image): image_pooling_BN normalises 3 samples per channel whose pooled
        # features nearly coincide after 130 randomly initialised layers, and amplifies the fp32 rounding of its input by up to
        # 1 / sqrt(eps) = 316; concat_projection reads that branch (measured 3.6e-5 / 4.8e-4 / 6.1e-4; every other layer and the
        # batch-4 runs at 65 x 65 / 97 x 97 sit at the tolerances of the other models)
        _teacher_forced_step(model_type, 513, 513, 16, 3, 1e-4, 2e-3, 2e-3)
    else:
        _teacher_forced_step(model_type, 513, 513, 16, 2, 2e-5, 5e-4, 1e-3)


def test_every_layer_at_513_matches_float64_with_the_production_plan(monkeypatch):
    """the same comparison with NOTHING switched off: BatchNorm-backward applies folded into weight / data
    gradients, aliased Add gradients, the stem fold, the separable head and the fused 257 x 257 block as the bench traces them.  A
    layer whose dz the plan never materialises is held through its weight gradient and its input gradient instead; the bounds are
    those of the folds-off test."""
    from test_model_gpu import _teacher_forced_step
    for k in ('DL3P_FOLD_APPLY', 'DL3P_GRAD_ALIAS', 'DL3P_FOLD_APPLY_STEM', 'DL3P_FUSED_HEAD', 'DL3P_IRB', 'DL3P_IRB_MIN_ROWS', 'DL3P_IRB_DEBUG_Z'):
        monkeypatch.delenv(k, raising=False)
    _teacher_forced_step('mobilenetv2', 513, 513, 16, 2, 2e-5, 5e-4, 1e-3,
                         expect_calls=('dl3p_irb_fwd', 'dl3p_irb_bwd_data', 'dl3p_stem_conv_bwd_weight_slabs_bn', 'dl3p_head_train_rows',
                                       'dl3p_pwconv_bwd_weight_slabs_bn'))


# ------------------------------------------------------------------------------------------- BASELINE configs[3] (VERDICT r03 missing 6)
def test_config3_full_size_properties():
    """BASELINE.json configs[3] at ITS size -- Xception + ASPP (rates 12 / 24 / 36) + decoder, output stride 8, 769 x 769,
    19 Cityscapes classes, per-GPU batch 2 -- where the float64 oracle would need many minutes: the size-independent properties
    configs[1] / [4] get.  Training is bitwise deterministic and hipGraph replay equals eager launches (losses and every weight
    after three steps), the first loss on random weights is close to ln 19, every weight stays finite, predict returns
    probability vectors."""
    pkg = load_pkg()
    N, C, H, W = 2, 19, 769, 769
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
    y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
    y[rng.uniform(size=y.shape) < 0.05] = 255

    def run(use_graphs):
        m = pkg.get_deeplabv3p_model('xception', C, (H, W), 8, training=True)
        m.compile(optimizer=pkg.SGD(0.01, momentum=0.9), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        m.use_graphs = use_graphs
        losses = [m.train_on_batch(x, y) for _ in range(3)]
        w = m.get_weights_by_name()
        del m
        torch.cuda.empty_cache()
        return losses, w
    la, wa = run(False)
    lb, wb = run(True)
    assert la == lb, (la, lb)
    assert all(np.array_equal(wa[k], wb[k]) for k in wa)
    assert abs(la[0] - np.log(C)) < 0.5, la
    assert all(np.isfinite(v).all() for v in wa.values())
    mi = pkg.get_deeplabv3p_model('xception', C, (H, W), 8, training=False)
    mi.set_weights_by_name(wa)
    p = mi.predict(x[:1])
    assert p.shape == (1, H, W, C) and np.abs(p.sum(-1) - 1.0).max() < 1e-5 and p.min() >= 0.0


def test_every_layer_of_config3s_graph_matches_float64_on_the_devices_own_inputs(monkeypatch):
    """The layer-local comparison (tests/test_model_gpu.py::_teacher_forced_step) on configs[3]'s GRAPH -- Xception, output stride 8
    (exit-flow rates 2 / 4, ASPP rates 12 / 24 / 36), 19 classes, production dispatch thresholds -- at 193 x 193, batch 2: the
    float64 oracle needs ~15 min for 769 x 769 (the GPU suite has 20 for everything), so the full size gets the properties above
    and every layer's forward / data-gradient + BatchNorm-backward segment / weight gradient is held against float64 here, on
    25 x 25 maps with the atrous taps of all three regimes (window, 3-class lattice, 2-class lattice: 36 > 25)."""
    from test_model_gpu import _teacher_forced_step
    monkeypatch.setenv('DL3P_FOLD_APPLY', '0')
    monkeypatch.setenv('DL3P_GRAD_ALIAS', '0')
    _teacher_forced_step('xception', 193, 193, 8, 2, 1e-4, 2e-3, 2e-3, C=19)


# ------------------------------------------------------------------------------------------- every conv forward at FULL size (round 6)
def _every_conv_forward_vs_float64_on_device(model_type, H, W, OS, N, C, tol, expect_kernels=()):
    """One eager training step at the configuration's own size, then EVERY pointwise and depthwise conv of the graph recomputed in
    float64 ON THE DEVICE from the device's own input tensor, the BatchNorm coefficients the step used and the weights the step
    started from (the NumPy oracle needs minutes per image at these sizes; torch.float64 on the MI355X needs milliseconds): the
    launch shapes, tiles and fused prologues the bench times, held to the op-level forward bound layer by layer."""
    import torch.nn.functional as F
    pkg = load_pkg()
    ops = load_pkg('ops')
    try:                                            # (production dispatch: the module's autouse fixture)
        torch.manual_seed(0)
        m = pkg.get_deeplabv3p_model(model_type, C, (H, W), OS, training=True)
        m.compile(optimizer=pkg.SGD(0.01, momentum=0.9), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        m.use_graphs = False
        rng = np.random.default_rng(29)
        x = rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
        y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
        w0 = {k: np.array(v) for k, v in m.get_weights_by_name().items()}
        loss = m.train_on_batch(x, y)
        assert np.isfinite(loss)
        ex = m._executor(N, True)
        calls = {ep for plan in (ex.fwd,) for (ep, _) in plan.labels}
        worst, checked, dense = ('', 0.0), 0, 0
        for op in m.graph.ops:
            if op.kind not in ('conv_pw', 'conv_dw', 'conv_dense') or op.out.root.id not in ex.buf or op.x.tensor.root.id not in ex.buf:
                continue            # (a fused inverted-residual block keeps no expand output; its depthwise conv reads no buffer)
            v = op.x
            a = ex.view(v.tensor).double()
            if v.group is not None:
                a = a * ex.gscale[v.group.id][v.goff:v.goff + v.tensor.C].double() + ex.gshift[v.group.id][v.goff:v.goff + v.tensor.C].double()
            if v.act == ops.ACT_RELU:
                a = a.clamp_min(0.0)
            elif v.act == ops.ACT_RELU6:
                a = a.clamp(0.0, 6.0)
            elif v.act == ops.ACT_HSWISH:
                a = a * (a + 3.0).clamp(0.0, 6.0) / 6.0
            elif v.act != ops.ACT_NONE:
                continue
            wk = torch.from_numpy(w0[op.w.name]).to(DEV).double()
            if op.kind == 'conv_dense':
                a = a[..., :op.cin]
                ref = 0
                for ky, kx, s in _taps(a, op.k, op.stride, op.rate, op.pad_t, op.pad_l, op.Ho, op.Wo):
                    ref = ref + s.reshape(-1, op.cin) @ wk[ky, kx]
                if op.b is not None:
                    ref = ref + torch.from_numpy(w0[op.b.name]).to(DEV).double()
                got = ex.view(op.out).double()[..., :wk.shape[-1]]
                dense += 1
            elif op.kind == 'conv_pw':
                real = wk.shape[-1]                  # (the classifier's columns are padded to a multiple of four on the device)
                ref = a.reshape(-1, op.cin)[:, :wk.shape[-2]] @ wk.reshape(-1, real)
                if op.b is not None:
                    ref = ref + torch.from_numpy(w0[op.b.name]).to(DEV).double()
                got = ex.view(op.out).double().reshape(-1, op.out.C)[:, :real]
            else:
                k_eff = op.k + (op.k - 1) * (op.rate - 1)
                xt = op.x.tensor
                pb = max((op.Ho - 1) * op.stride + k_eff - xt.H - op.pad_t, 0)
                pr = max((op.Wo - 1) * op.stride + k_eff - xt.W - op.pad_l, 0)
                ap = F.pad(a.permute(0, 3, 1, 2), (op.pad_l, pr, op.pad_t, pb))
                ref = F.conv2d(ap, wk.reshape(op.k, op.k, op.c).permute(2, 0, 1).unsqueeze(1), stride=op.stride, dilation=op.rate,
                               groups=op.c).permute(0, 2, 3, 1)
                got = ex.view(op.out).double()[..., :op.c]
            r = float((got - ref.reshape(got.shape)).abs().max() / ref.abs().max().clamp_min(1e-30))
            checked += 1
            if r > worst[1]:
                worst = (op.name, r)
            del a, ref, got
        print('%s %dx%d batch %d: %d convs (%d dense) checked, worst %s %.3e' % (model_type, H, W, N, checked, dense, worst[0], worst[1]))
        assert checked >= 20 and dense >= 1, (checked, dense)
        assert worst[1] < tol, worst
        for k in expect_kernels:
            assert k in calls, (k, sorted(calls))
        return checked, worst
    finally:
        torch.cuda.empty_cache()


def test_headline_batch16_every_conv_forward_matches_float64():
    """BASELINE configs[1] AS THE BENCH RUNS IT (MobileNetV2, 513 x 513, batch 16): 266256-row decoder GEMMs on the pinned-schedule
    kernel, fused 257 x 257 / 129 x 129 blocks, lattice ASPP kernels -- every materialised conv output against float64"""
    n, worst = _every_conv_forward_vs_float64_on_device('mobilenetv2', 513, 513, 16, 16, 21, 2e-5, expect_kernels=('dl3p_pwconv_fwd_sb', 'dl3p_irb_fwd'))
    assert n >= 62, n                   # (61 pointwise / depthwise + the stem)


def test_config3_full_size_every_conv_forward_matches_float64():
    """BASELINE configs[3] at ITS size (Xception, 769 x 769, output stride 8, 19 classes, batch 2): VERDICT r05 weak 5 -- the full size
    had property checks only"""
    n, worst = _every_conv_forward_vs_float64_on_device('xception', 769, 769, 8, 2, 19, 1e-4)
    assert n >= 147, n                  # (the entry-flow and stem dense convs included)


def test_config2_full_size_every_conv_forward_matches_float64():
    """BASELINE configs[2] at its per-GPU shape (Xception, 513 x 513, output stride 16, batch 4: the 4356-row layers)"""
    n, worst = _every_conv_forward_vs_float64_on_device('xception', 513, 513, 16, 4, 21, 1e-4)
    assert n >= 147, n
