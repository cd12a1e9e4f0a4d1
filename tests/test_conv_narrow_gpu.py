"""The narrow-output direct 3x3 convolutions (csrc/conv_narrow.hip, dl3p_conv_narrow_*) against float64 at every dense-layer
shape of a 512 x 512, batch-16 PeleeNet step at output stride 16 and 8: forward with the BatchNorm statistics partial rows,
data gradient (written and accumulated into a channel slice), weight gradient (slabs + the deterministic row reduction).
The other route of these convs (the implicit GEMM, DL3P_NARROW_CONV=0) is covered by the model-level parity tests in
tests/test_peleenet_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (H = W, Cin): branch1b / branch2b take Cin = inter_channel (16, 32, 64 in blocks 1, 2, 3-4), branch2c Cin = 16; Cout = 16
# OS 16: block 1 at 128, block 2 at 64, blocks 3-4 at 32; OS 8: block 1 at 128, blocks 2-4 at 64
SHAPES = sorted({(128, 16), (64, 32), (64, 16), (32, 64), (32, 16), (64, 64)})


def _ref(x64, w64, gy64):
    """float64 conv (torch CPU), its data and weight gradients"""
    x = torch.tensor(x64, requires_grad=True)
    w = torch.tensor(w64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    y.backward(torch.tensor(gy64))
    return y.detach().numpy(), x.grad.numpy(), w.grad.numpy()


def _f(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@pytest.mark.parametrize('H,Cin', SHAPES)
def test_narrow_conv_matches_float64(ops, H, Cin):
    N, W, Cout = 16, H, 16
    rng = np.random.default_rng(H + Cin)
    z = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, Cin).astype(np.float32)
    sh = (rng.standard_normal(Cin) * 0.3).astype(np.float32)
    lim = np.sqrt(6.0 / (9 * Cin + 9 * Cout))
    w = rng.uniform(-lim, lim, (3, 3, Cin, Cout)).astype(np.float32)
    gy = rng.standard_normal((N, H, W, Cout)).astype(np.float32)
    # the prologue as the device forms it (fp32 fma + ReLU), then float64 from there
    zt, sct, sht = _f(z), _f(sc), _f(sh)
    a = torch.relu(torch.addcmul(sht, zt, sct)).double().cpu().numpy()
    y_ref, gx_ref, gw_ref = _ref(a, w.astype(np.float64), gy.astype(np.float64))

    # forward into channels [16, 32) of a 48-channel buffer (a dense-block slice), with the statistics partial rows
    buf = torch.full((N, H, W, 48), 3.0, device=DEV)
    y, part = ops.conv_narrow_fwd(zt, _f(w), sct, sht, ops.ACT_RELU, out=buf[..., 16:32], stats=True)
    yd = y.double().cpu().numpy()
    scale = np.abs(y_ref).max()
    assert np.abs(yd - y_ref).max() < 1e-5 * scale
    assert bool((buf[..., :16] == 3.0).all()) and bool((buf[..., 32:] == 3.0).all())
    p = part.double().cpu().numpy()
    assert 1 <= p.shape[0] <= 1024
    s_ref, q_ref = y_ref.sum((0, 1, 2)), (y_ref ** 2).sum((0, 1, 2))
    M = N * H * W
    # (fp32 partial sums of M terms: bound by the sum of magnitudes, not by the cancelled total)
    assert np.all(np.abs(p[:, 0].sum(0) - s_ref) <= 1e-5 * scale * M ** 0.5 + 1e-6 * np.abs(y_ref).sum((0, 1, 2)))
    assert np.all(np.abs(p[:, 1].sum(0) - q_ref) <= 1e-5 * q_ref)

    # data gradient: written, then accumulated, into a slice
    g = torch.zeros((N, H, W, Cin + 8), device=DEV)
    ops.conv_narrow_bwd_data(_f(gy), _f(w), out=g[..., 4:4 + Cin])
    gd = g[..., 4:4 + Cin].double().cpu().numpy()
    assert np.abs(gd - gx_ref).max() < 1e-5 * np.abs(gx_ref).max()
    assert bool((g[..., :4] == 0).all()) and bool((g[..., 4 + Cin:] == 0).all())
    ops.conv_narrow_bwd_data(_f(gy), _f(w), out=g[..., 4:4 + Cin], accumulate=True)
    assert np.abs(g[..., 4:4 + Cin].double().cpu().numpy() - 2 * gx_ref).max() < 2e-5 * np.abs(gx_ref).max()

    # weight gradient of act(BN(z)) (prologue in the staging pass), deterministic
    gw1 = ops.conv_narrow_bwd_weight(zt, _f(gy), sct, sht, ops.ACT_RELU)
    gw2 = ops.conv_narrow_bwd_weight(zt, _f(gy), sct, sht, ops.ACT_RELU)
    assert torch.equal(gw1, gw2)
    err = np.abs(gw1.double().cpu().numpy() - gw_ref).max()
    assert err < 1e-5 * np.abs(gw_ref).max(), err


def test_narrow_conv_refuses_unsupported_shapes(ops):
    lib = ops.lib()
    assert lib.conv_narrow_supported(16, 16, 3, 1, 1) == 1
    assert lib.conv_narrow_supported(64, 32, 3, 1, 1) == 1
    assert lib.conv_narrow_supported(128, 16, 3, 1, 1) == 0        # Cin <= 64
    assert lib.conv_narrow_supported(16, 64, 3, 1, 1) == 0         # Cout <= 32
    assert lib.conv_narrow_supported(16, 16, 3, 2, 1) == 0         # stride 1 only
    assert lib.conv_narrow_supported(16, 16, 3, 1, 2) == 0         # no dilation
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_fwd(torch.zeros((1, 8, 8, 128), device=DEV), torch.zeros((3, 3, 128, 16), device=DEV))
