"""The narrow-output direct 3x3 convolutions (csrc/conv_narrow.hip, dl3p_conv_narrow_*) against float64 at every dense-layer
shape of a 512 x 512, batch-16 PeleeNet step at output stride 16 and 8: forward with the BatchNorm statistics partial rows,
data gradient (written and accumulated into a channel slice), weight gradient (slabs + the deterministic row reduction).
`test_narrow_conv_contract` then walks the edges of what dl3p_conv_narrow_supported accepts: every Cout, Cin from 4 to 64, ragged
8 x 16 tiles, prefix-view inputs and slice outputs / gradients, each prologue activation and none.
The other route of these convs (the implicit GEMM, DL3P_NARROW_CONV=0) is covered by the model-level parity tests in
tests/test_peleenet_gpu.py and by tests/test_ops_gpu.py::test_conv2d_implicit_gemm_peleenet_geometry."""
import ctypes

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


TH, TW = 8, 16                  # output tile of csrc/conv_narrow.hip


def _act64(a, act, ops):
    if act == ops.ACT_RELU:
        return a.clamp_min(0.0)
    if act == ops.ACT_RELU6:
        return a.clamp(0.0, 6.0)
    if act == ops.ACT_HSWISH:
        return a * (a + 3.0).clamp(0.0, 6.0) / 6.0
    return a


# (N, H, W, Cin, Cout, prologue activation or None): ragged tiles (7 x 9, one past a tile each way at 9 x 17, PeleeNet at 480 on
# 30 x 30, 33 x 65), a single pixel, N = 1, every Cout, Cin from 4 to 64; the last case runs > 1024 forward and > 512 slab tiles
CONTRACT = [(1, 1, 1, 4, 16, 'relu'), (2, 7, 9, 12, 4, 'none'), (2, 9, 17, 16, 8, 'relu6'), (3, 30, 30, 20, 32, 'hswish'),
            (1, 33, 65, 48, 16, None), (2, 9, 17, 64, 32, 'relu'), (1, 7, 9, 32, 8, None), (2, 30, 30, 4, 4, 'relu6'),
            (1, 17, 33, 64, 4, 'hswish'), (16, 128, 128, 16, 16, 'relu')]


@pytest.mark.parametrize('case', CONTRACT, ids=lambda c: '%dx%dx%dx%d_to%d_%s' % (c[:5] + (c[5] or 'bare',)))
def test_narrow_conv_contract(ops, case):
    """forward (+ statistics rows), data gradient (written and accumulated) and weight gradient against float64, with x a prefix
    view [..., :Cin] of a buffer Cin + 32 wide, dy the slice [16, 16 + Cout) of a wider buffer, y and gx written into slices"""
    N, H, W, Cin, Cout, act = case
    acts = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'relu6': ops.ACT_RELU6, 'hswish': ops.ACT_HSWISH}
    actc = acts.get(act, ops.ACT_NONE)
    g = torch.Generator(device=DEV)
    g.manual_seed(N * 1000 + H * 37 + W + Cin + Cout)
    xbuf = torch.randn(N, H, W, Cin + 32, device=DEV, generator=g) * 100.0     # (the channels beside the view: large)
    x = xbuf[..., :Cin]
    x.copy_(torch.randn(N, H, W, Cin, device=DEV, generator=g))
    w = (torch.rand(3, 3, Cin, Cout, device=DEV, generator=g) * 2 - 1) * (6.0 / (9 * Cin + 9 * Cout)) ** 0.5
    dybuf = torch.randn(N, H, W, Cout + 32, device=DEV, generator=g) * 100.0
    dy = dybuf[..., 16:16 + Cout]
    dy.copy_(torch.randn(N, H, W, Cout, device=DEV, generator=g))
    if act is not None:
        sc = torch.rand(Cin, device=DEV, generator=g) + 0.5
        sh = torch.randn(Cin, device=DEV, generator=g) * 0.5 + (2.0 if act == 'relu6' else 0.0)
        pro = (sc, sh, actc)
        a = _act64(torch.addcmul(sh, x, sc).double(), actc, ops)        # the fp32 fma the device forms, then float64
    else:
        pro = (None, None, ops.ACT_NONE)
        a = x.double()
    y_ref, gx_ref, gw_ref = _ref(a.cpu().numpy(), w.double().cpu().numpy(), dy.double().cpu().numpy())

    ybuf = torch.full((N, H, W, Cout + 24), 3.0, device=DEV)
    y, part = ops.conv_narrow_fwd(x, w, *pro, out=ybuf[..., 8:8 + Cout], stats=True)
    yd = y.double().cpu().numpy()
    scale = max(np.abs(y_ref).max(), 1e-30)
    assert np.abs(yd - y_ref).max() < 1e-5 * scale, np.abs(yd - y_ref).max() / scale
    assert bool((ybuf[..., :8] == 3.0).all()) and bool((ybuf[..., 8 + Cout:] == 3.0).all())
    ntiles = N * -(-H // TH) * -(-W // TW)
    p = part.double().cpu().numpy()
    assert p.shape == (min(ntiles, 1024), 2, Cout), (p.shape, ntiles)
    s_ref, q_ref = y_ref.sum((0, 1, 2)), (y_ref ** 2).sum((0, 1, 2))
    M = N * H * W
    assert np.all(np.abs(p[:, 0].sum(0) - s_ref) <= 1e-5 * scale * M ** 0.5 + 1e-6 * np.abs(y_ref).sum((0, 1, 2)))
    assert np.all(np.abs(p[:, 1].sum(0) - q_ref) <= 1e-5 * q_ref + 1e-30)

    gbuf = torch.full((N, H, W, Cin + 12), -5.0, device=DEV)
    gx = gbuf[..., 4:4 + Cin]
    ops.conv_narrow_bwd_data(dy, w, out=gx)
    gscale = max(np.abs(gx_ref).max(), 1e-30)
    assert np.abs(gx.double().cpu().numpy() - gx_ref).max() < 1e-5 * gscale
    assert bool((gbuf[..., :4] == -5.0).all()) and bool((gbuf[..., 4 + Cin:] == -5.0).all())
    ops.conv_narrow_bwd_data(dy, w, out=gx, accumulate=True)
    assert np.abs(gx.double().cpu().numpy() - 2 * gx_ref).max() < 2e-5 * gscale

    gw1 = ops.conv_narrow_bwd_weight(x, dy, *pro)
    gw2 = ops.conv_narrow_bwd_weight(x, dy, *pro)
    assert torch.equal(gw1, gw2)
    err = np.abs(gw1.double().cpu().numpy() - gw_ref).max()
    assert err < 1e-5 * max(np.abs(gw_ref).max(), 1e-30), err


def test_narrow_weight_gradient_slabs_through_the_batched_reduction(ops):
    """the executor's path: dl3p_conv_narrow_bwd_weight_slabs, then dl3p_reduce_rows_batched (every weight gradient of a step in
    two launches), bitwise the one-call dl3p_conv_narrow_bwd_weight"""
    L = ops.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    shapes = [(16, 128, 128, 16, 16), (2, 9, 17, 64, 32), (1, 30, 30, 12, 4)]
    refs, dsts, rec, keep = [], [], [], []
    for N, H, W, Cin, Cout in shapes:
        xbuf = torch.randn(N, H, W, Cin + 32, device=DEV, generator=g)
        dybuf = torch.randn(N, H, W, Cout + 32, device=DEV, generator=g)
        x, dy = xbuf[..., :Cin], dybuf[..., 16:16 + Cout]
        sc = torch.rand(Cin, device=DEV, generator=g) + 0.5
        sh = torch.randn(Cin, device=DEV, generator=g) * 0.3
        refs.append(ops.conv_narrow_bwd_weight(x, dy, sc, sh, ops.ACT_RELU))
        nbytes = L.conv_narrow_bwd_weight_workspace(N, H, W, Cin, Cout)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        rows = ctypes.c_int(0)
        L.conv_narrow_bwd_weight_slabs(x.data_ptr(), Cin + 32, sc.data_ptr(), sh.data_ptr(), ops.ACT_RELU, dy.data_ptr(), Cout + 32,
                                       ws.data_ptr(), nbytes, ctypes.byref(rows), N, H, W, Cin, Cout, st)
        assert rows.value == min(N * -(-H // TH) * -(-W // TW), 512)
        out = torch.full((9 * Cin * Cout,), float('nan'), dtype=torch.float32, device=DEV)
        dsts.append(out)
        keep += [xbuf, dybuf, ws, sc, sh]
        rec.append((ws.data_ptr(), out.data_ptr(), rows.value, 9 * Cin * Cout))
    jobs = np.array(rec, dtype=np.dtype([('src', '<u8'), ('dst', '<u8'), ('rows', '<i4'), ('n', '<i4')]))
    maps = ([], [])
    for j, (_, _, rows, n) in enumerate(rec):
        v = L.reduce_rows_variant(rows, n)
        be = L.reduce_rows_block_elements(v)
        maps[v].extend((j, b) for b in range((n + be - 1) // be))
    jt = torch.from_numpy(jobs.view(np.uint8).copy()).to(DEV)
    m = [torch.tensor(mm if mm else [(0, 0)], dtype=torch.int32, device=DEV) for mm in maps]
    L.reduce_rows_batched(jt.data_ptr(), m[0].data_ptr(), len(maps[0]), m[1].data_ptr(), len(maps[1]), st)
    for out, ref in zip(dsts, refs):
        assert torch.equal(out.reshape(ref.shape), ref)


def test_narrow_conv_refuses_unsupported_shapes(ops):
    lib = ops.lib()
    assert lib.conv_narrow_supported(16, 16, 3, 1, 1) == 1
    assert lib.conv_narrow_supported(64, 32, 3, 1, 1) == 1
    assert lib.conv_narrow_supported(128, 16, 3, 1, 1) == 0        # Cin <= 64
    assert lib.conv_narrow_supported(16, 64, 3, 1, 1) == 0         # Cout <= 32
    assert lib.conv_narrow_supported(16, 16, 3, 2, 1) == 0         # stride 1 only
    assert lib.conv_narrow_supported(16, 16, 3, 1, 2) == 0         # no dilation
    assert lib.conv_narrow_supported(16, 12, 3, 1, 1) == 0         # Cout in {4, 8, 16, 32}
    assert lib.conv_narrow_supported(68, 16, 3, 1, 1) == 0
    assert lib.conv_narrow_supported(6, 16, 3, 1, 1) == 0          # Cin a multiple of 4
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_fwd(torch.zeros((1, 8, 8, 128), device=DEV), torch.zeros((3, 3, 128, 16), device=DEV))
    z = lambda *s: torch.zeros(s, device=DEV)
    for Cin, Cout in ((16, 12), (68, 16), (6, 16)):
        with pytest.raises(ops.Dl3pError):
            ops.conv_narrow_fwd(z(1, 8, 8, Cin), z(3, 3, Cin, Cout))
        with pytest.raises(ops.Dl3pError):
            ops.conv_narrow_bwd_data(z(1, 8, 8, Cout), z(3, 3, Cin, Cout))
        with pytest.raises(ops.Dl3pError):
            ops.conv_narrow_bwd_weight(z(1, 8, 8, Cin), z(1, 8, 8, Cout))
    w = z(3, 3, 16, 16)
    with pytest.raises(ops.Dl3pError):                               # ldx % 4 != 0 (a 16-channel view of an 18-wide buffer)
        ops.conv_narrow_fwd(z(1, 8, 8, 18)[..., :16], w)
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_bwd_data(z(1, 8, 8, 18)[..., :16], w)
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_bwd_weight(z(1, 8, 8, 18)[..., :16], z(1, 8, 8, 16))
    with pytest.raises(ops.Dl3pError):                               # a view 4 bytes into its buffer: not 16-byte aligned
        ops.conv_narrow_fwd(z(1, 8, 8, 20)[..., 1:17], w)
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_fwd(z(1, 8, 8, 16), w, out=z(1, 8, 8, 20)[..., 1:17])
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_bwd_data(z(1, 8, 8, 16), w, out=z(1, 8, 8, 20)[..., 2:18])
    with pytest.raises(ops.Dl3pError):
        ops.conv_narrow_bwd_weight(z(1, 8, 8, 16), z(1, 8, 8, 20)[..., 1:17])
