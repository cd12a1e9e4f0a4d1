"""Every PeleeNet layer at the size it trains at (512 x 512, 21 classes, output stride 16) against float64 on the device.

One eager training step with the production dispatch, SGD(0) (the weights stay the ones the forward used) and every conv-output
gradient materialised (DL3P_FOLD_APPLY=0, DL3P_GRAD_ALIAS=0); then for every pointwise / dense conv, max pooling and local average
pooling: the output recomputed in float64 from the device's own input view (a prefix view of a dense block buffer, activated by its
group's BatchNorm + ReLU), compared with the output slice inside its block buffer; every conv's weight gradient from the device's own
dz; every BatchNorm's batch mean and 1 / sqrt(var + eps) against float64 statistics of the device's own conv output.  The 64 x 64
restatement (tests/test_peleenet_gpu.py) runs other tile counts, no pooling floors and other 1x1 routes."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from layer_walk import _act64, _taps

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def production_dispatch():
    L = load_pkg('_lib').lib()
    L.set_option(b'pw_small_min_rows', -1)        # production threshold (2^17 rows)
    yield
    L.set_option(b'pw_small_min_rows', 64)        # what conftest.py sets for the small-shape tests


def _walk(monkeypatch, mt, narrow, N, bf16=False):
    """-> {(check, kind): (worst layer, worst value)} and the entry points the step launched"""
    monkeypatch.setenv('DL3P_NARROW_CONV', narrow)
    monkeypatch.setenv('DL3P_FOLD_APPLY', '0')
    monkeypatch.setenv('DL3P_GRAD_ALIAS', '0')
    pkg = load_pkg()
    O_ = load_pkg('ops')
    C, H, W = 21, 512, 512
    try:
        if bf16:
            pkg.mixed_precision.set_policy(pkg.mixed_precision.Policy('mixed_bfloat16'))
        try:
            torch.manual_seed(0)
            m = pkg.get_deeplabv3p_model(mt, C, (H, W), 16, training=True)
        finally:
            pkg.mixed_precision.set_policy(pkg.mixed_precision.Policy('float32'))
        m.compile(optimizer=pkg.SGD(0.0), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        m.use_graphs = False
        rng = np.random.default_rng(31)
        x = rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
        y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
        y[rng.uniform(size=y.shape) < 0.05] = 255
        loss = m.train_on_batch(x, y)
        assert np.isfinite(loss)
        ex = m._executor(N, True)
        assert ex.bf16 == bf16
        calls = {ep for plan in (ex.fwd, ex.bwd) for (ep, _) in plan.labels}
        weights = m.get_weights_by_name()
        st = m._store
        bn_by_z = {id(bn.z): bn for bn in m.graph.bns}
        worst = {}
        counts = {}

        def note(key, name, val):
            counts[key] = counts.get(key, 0) + 1
            if val > worst.get(key, ('', -1.0))[1]:
                worst[key] = (name, val)

        for op in m.graph.ops:
            if op.kind not in ('conv_pw', 'conv_dense', 'maxpool', 'avgpool'):
                continue
            if op.out.root.id not in ex.buf or op.x.tensor.root.id not in ex.buf:
                continue
            v = op.x
            cin = op.cin if op.kind.startswith('conv') else op.out.C
            a = ex.view(v.tensor)[..., :cin].double()
            if v.group is not None:
                sc = ex.gscale[v.group.id][v.goff:v.goff + cin].double()
                sh = ex.gshift[v.group.id][v.goff:v.goff + cin].double()
                a = (a * sc + sh).float().double()              # the prologue's single fp32 fma
            if v.group is not None or v.act != O_.ACT_NONE:
                a = _act64(a, v.act)
                if bf16:
                    a = a.float().to(torch.bfloat16).double()
            cout = op.out.C if op.kind in ('maxpool', 'avgpool') else weights[op.w.name].shape[-1]
            got = ex.view(op.out)[..., :cout].double()
            f64 = dict(dtype=torch.float64, device=DEV)
            if op.kind == 'maxpool':
                ref = None
                for _, _, s in _taps(a, op.k, op.stride, 1, op.pad_t, op.pad_l, op.Ho, op.Wo):
                    ref = s.clone() if ref is None else torch.maximum(ref, s)
            elif op.kind == 'avgpool':
                ref = torch.zeros(got.shape, **f64)
                for _, _, s in _taps(a, op.k, op.stride, 1, 0, 0, op.Ho, op.Wo):
                    ref += s
                ref /= op.k * op.k
            else:
                w = torch.from_numpy(weights[op.w.name]).to(DEV).double()
                if bf16:
                    w = w.float().to(torch.bfloat16).double()
                dz = ex.view(op.out, grad=True)[..., :cout].double() if op.w.trainable else None
                if op.kind == 'conv_pw':
                    ref = (a.reshape(-1, cin) @ w.reshape(cin, cout)).reshape(got.shape)
                    gw = (a.reshape(-1, cin).t() @ dz.reshape(-1, cout)).reshape(w.shape) if dz is not None else None
                else:
                    ref = torch.zeros(got.shape, **f64)
                    gw = torch.zeros(w.shape, **f64) if dz is not None else None
                    for ky, kx, s in _taps(a, op.k, op.stride, op.rate, op.pad_t, op.pad_l, op.Ho, op.Wo):
                        ref += (s.reshape(-1, cin) @ w[ky, kx]).reshape(got.shape)
                        if gw is not None:
                            gw[ky, kx] = s.reshape(-1, cin).t() @ dz.reshape(-1, cout)
                if getattr(op, 'b', None) is not None:
                    ref = ref + torch.from_numpy(weights[op.b.name]).to(DEV).double()
                if gw is not None:
                    g = torch.from_numpy(np.ascontiguousarray(st.get(op.w, st.G))).to(DEV).double().reshape(gw.shape)
                    scale = float(gw.abs().max())
                    if scale > 1e-12:
                        note(('wgrad', op.kind), op.name, float((g - gw).abs().max()) / scale)
                # the BatchNorm behind this conv: the batch statistics the step used against float64 ones of its own output
                bn = bn_by_z.get(id(op.out))
                if bn is not None:
                    z = got.reshape(-1, cout)
                    mean = z.mean(0)
                    var = ((z - mean) ** 2).mean(0)
                    aux = ex.bn_aux[bn]
                    std = var.sqrt()
                    note(('bn_mean', op.kind), bn.name, float(((aux['mean'][:cout].double() - mean).abs() / std.clamp_min(1e-30)).max()))
                    inv = 1.0 / (var + bn.eps).sqrt()
                    note(('bn_invstd', op.kind), bn.name, float(((aux['invstd'][:cout].double() - inv).abs() / inv).max()))
                    del z, mean, var
            rmax = float(ref.abs().max())
            if bf16:
                tol = 1.01 * 2.0 ** -8 * ref.abs() + 2e-3 * rmax + 1e-30
                if op.name == 'conv_upsample':
                    tol = torch.full_like(ref, 1e-4 * max(1.0, rmax))
                note(('fwd_miss', op.kind), op.name, float(((got - ref).abs() > tol).double().mean()))
            else:
                note(('fwd', op.kind), op.name, float((got - ref).abs().max()) / max(rmax, 1e-30))
            del a, ref, got
        return worst, counts, calls
    finally:
        torch.cuda.empty_cache()


def _report(tag, worst, counts):
    for k in sorted(worst):
        print('%s %-22s %4d layers, worst %-55s %.3e' % (tag, '%s/%s' % k, counts[k], worst[k][0], worst[k][1]))


# fp32 bounds, about 10x the worst value measured on the MI355X over the three fp32 walks (batch 16, OS 16):
#   forward (relative to the layer's range): dense 9.1e-7 (denselayer5_branch1b, route 1), pointwise 1.24e-6 (concat_projection),
#     local average pooling 1.0e-7, max pooling exact;
#   weight gradient (relative to its scale): dense 1.5e-6 (stem2b), pointwise 4.9e-6 (transition4);
#   batch mean (in standard deviations): dense 8.5e-8, pointwise 4.9e-6 (image_pooling_BN);
#   1 / sqrt(var + eps) (relative): dense 1.2e-7, pointwise 2.8e-4 -- image_pooling_BN, whose 16 rows (one per image) leave the
#     one-pass fp32 variance of a channel with a large mean little to cancel against; every other pointwise BatchNorm is below 5e-6
TOL = {('fwd', 'conv_dense'): 1e-5, ('fwd', 'conv_pw'): 1.5e-5, ('fwd', 'avgpool'): 1e-6, ('fwd', 'maxpool'): 0.0,
       ('wgrad', 'conv_dense'): 1.5e-5, ('wgrad', 'conv_pw'): 5e-5,
       ('bn_mean', 'conv_dense'): 1e-6, ('bn_mean', 'conv_pw'): 5e-5, ('bn_invstd', 'conv_dense'): 1.5e-6, ('bn_invstd', 'conv_pw'): 3e-3}
# bf16 (batch 4): the bounds of the MobileNetV3 bf16 walk for outputs (fraction of elements beyond one bf16 ulp + 2e-3 of the range:
# measured 0) and weight gradients (4e-3 of the scale; measured 3.9e-5, conv_upsample); statistics 10x the measured 1.9e-7
TOL_BF16 = {'fwd_miss': 1e-3, 'wgrad': 4e-3, 'bn_mean': 2e-6, 'bn_invstd': 2e-6}


@pytest.mark.parametrize('mt,narrow', [('peleenet', '1'), ('peleenet', '0'), ('peleenet_lite', '0')])
def test_every_layer_at_512_batch16_matches_float64(monkeypatch, mt, narrow):
    """fp32, batch 16: both routes of the 63 dense-layer 3x3 convs (the narrow direct kernels, the implicit GEMM)"""
    worst, counts, calls = _walk(monkeypatch, mt, narrow, 16)
    _report('%s route %s' % (mt, narrow), worst, counts)
    assert counts[('fwd', 'conv_dense')] >= 65 and counts[('wgrad', 'conv_dense')] >= 65   # 63 dense layers + stem1 + stem2b
    assert counts[('fwd', 'conv_pw')] >= 50 and counts[('fwd', 'maxpool')] == 1 and counts[('fwd', 'avgpool')] == 2
    assert counts[('bn_mean', 'conv_dense')] >= 65
    assert set(worst) == set(TOL), sorted(worst)
    for k, (name, val) in worst.items():
        assert val <= TOL[k], (k, name, val)
    if narrow == '1':
        assert 'dl3p_conv_narrow_fwd' in calls
    else:
        assert 'dl3p_conv_narrow_fwd' not in calls
        assert 'dl3p_conv2d_gemm_fwd' in calls or 'dl3p_conv2d_gemm_fwd_sb' in calls
    assert 'dl3p_avgpool2d_fwd' in calls and 'dl3p_maxpool2d_fwd' in calls


def test_every_layer_at_512_bf16_matches_float64(monkeypatch):
    """mixed_bfloat16, batch 4, the default route: the bf16 im2col GEMMs and the bf16 poolings on prefix views"""
    worst, counts, calls = _walk(monkeypatch, 'peleenet', '0', 4, bf16=True)
    _report('peleenet bf16', worst, counts)
    assert counts[('fwd_miss', 'conv_dense')] >= 65 and counts[('fwd_miss', 'avgpool')] == 2 and counts[('fwd_miss', 'maxpool')] == 1
    for k, (name, val) in worst.items():
        assert val <= TOL_BF16[k[0]], (k, name, val)
    assert any(c.startswith('dl3p_avgpool2d_fwd') for c in calls) and any(c.startswith('dl3p_maxpool2d_fwd') for c in calls)
