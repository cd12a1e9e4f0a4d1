"""dl3p_ghost_fwd (csrc/ghost_fwd.hip), the fused ghost-module forward, element by element against float64.

Bounds, of the tests/test_dw_edges_gpu.py kind -- unit roundoff x roundings counted from the kernel's operations x sum of |terms|:
  z1 = a W1: a chain of K / 4 v_mfma_f32_16x16x4_f32, i.e. K products added to one accumulator: any order of a K-term sum of
      products, fused or not, stays within K roundings of S1 = |a| |W1|; the prologue a = act(fmaf(x, scale, shift)) rounds once
      (1 more where there is an affine; ReLU / none are exact on the rounded value); + 1 for second order and the float64
      reference itself:                                                         e1 = (K + 1 + n_pro) u S1
  a1 = act1(fmaf(z1, s1, h1)) from the kernel's own z1: the z1 error passes through s1 (ReLU / none have Lipschitz constant 1), the
      fma rounds once:                                                           ea = |s1| e1 + u (|z1 s1| + |h1|)
  z2 = the nine taps, one multiplication and eight FMAs from it: 9 roundings (+ 1 as above) of S2 = conv(|a1|, |wdw|), and the
      propagated error of the taps:                                             e2 = (9 + 1) u S2 + conv(ea, |wdw|)
A tap outside the image is 0 AFTER BatchNorm and activation; |h1| is of order 1 here, so taking h1 (or act1(h1)) there instead
is an O(1) error.  The operands sit in buffers of their own; x is a channel slice of a wider buffer whose other channels are
NaN, y the middle view of a wider buffer filled with a sentinel that has to survive bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
SENTINEL = -123456.75
KC = [(16, 8), (16, 24), (24, 36), (48, 12), (72, 12)]
WS = (1, 2, 15, 16, 17, 33)
HS = (1, 2, 3, 9)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _conv(a, w):
    """3x3 stride 1 'same' depthwise conv, zero padding; a (N,H,W,C), w (3,3,C), float64"""
    N, H, W, C = a.shape
    p = np.zeros((N, H + 2, W + 2, C))
    p[:, 1:H + 1, 1:W + 1] = a
    out = np.zeros_like(a)
    for ky in range(3):
        for kx in range(3):
            out += p[:, ky:ky + H, kx:kx + W] * w[ky, kx]
    return out


def _operands(N, H, W, K, C, prologue, seed):
    """float32-representable operands as float64 arrays; the two images differ in sign and scale, so that a tap taken from the
    neighbouring image (or a row wrapped into it) is far outside any bound"""
    rng = np.random.default_rng(seed)
    x = _f32(rng.standard_normal((N, H, W, K)))
    x[1:] = _f32(x[1:] * 5.0 + 7.0)
    xs = xh = None
    if prologue:
        xs, xh = _f32(rng.uniform(0.5, 1.5, K)), _f32(rng.standard_normal(K) * 0.3)
    w1 = _f32(rng.standard_normal((K, C)) / np.sqrt(K))
    s1 = _f32(rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C))
    h1 = _f32(rng.uniform(0.7, 1.5, C) * rng.choice([-1.0, 1.0], C))          # |h1| of order 1
    wdw = _f32(rng.standard_normal((3, 3, C)) / 3.0)
    return x, xs, xh, w1, s1, h1, wdw


def _reference(x, xs, xh, w1, s1, h1, act1, wdw):
    """-> z1, e1, z2, e2 (float64)"""
    K = x.shape[-1]
    n_pro = 0
    a = x
    if xs is not None:
        a, n_pro = np.maximum(x * xs + xh, 0.0), 1
    z1 = a @ w1
    e1 = (K + 1 + n_pro) * U * (np.abs(a) @ np.abs(w1))
    u1 = z1 * s1 + h1
    a1 = np.maximum(u1, 0.0) if act1 else u1
    ea = np.abs(s1) * e1 + U * (np.abs(z1 * s1) + np.abs(h1))
    z2 = _conv(a1, wdw)
    e2 = (9 + 1) * U * _conv(np.abs(a1), np.abs(wdw)) + _conv(ea, np.abs(wdw))
    return z1, e1, z2, e2


def _buffers(x, C):
    """x inside NaN channels, y inside sentinel channels: (x wide, x view, y wide, y view)"""
    N, H, W, K = x.shape
    xw = torch.full((N, H, W, K + 8), float('nan'), dtype=torch.float32, device=DEV)
    xw[..., 4:4 + K] = _t(x)
    yw = torch.full((N, H, W, 2 * C + 8), SENTINEL, dtype=torch.float32, device=DEV)
    return xw, xw[..., 4:4 + K], yw, yw[..., 4:4 + 2 * C]


def _sentinel_intact(yw, C):
    rest = torch.cat([yw[..., :4], yw[..., 4 + 2 * C:]], -1)
    return bool((rest == SENTINEL).all())


def _run(ops, N, H, W, K, C, prologue, act1, seed, pair=True):
    x, xs, xh, w1, s1, h1, wdw = _operands(N, H, W, K, C, prologue, seed)
    z1, e1, z2, e2 = _reference(x, xs, xh, w1, s1, h1, act1, wdw)
    xw, xv, yw, yv = _buffers(x, C)
    kw = dict(in_scale=_t(xs), in_shift=_t(xh), in_act=ops.ACT_RELU) if prologue else {}
    a1c = ops.ACT_RELU if act1 else ops.ACT_NONE
    tw1, ts1, th1, twd = _t(w1), _t(s1), _t(h1), _t(wdw)
    assert ops.ghost_fwd_supported((N, H, W, K), C)
    ops.ghost_fwd(xv, tw1, ts1, th1, a1c, twd, out=yv, **kw)
    got = yv.cpu().numpy().astype(np.float64)
    where = 'N=%d H=%d W=%d K=%d C=%d prologue=%s act1=%s' % (N, H, W, K, C, prologue, act1)
    assert np.isfinite(got).all(), where
    d1, d2 = np.abs(got[..., :C] - z1), np.abs(got[..., C:] - z2)
    assert np.all(d1 <= e1 + 1e-38), ('z1', where, float((d1 / (e1 + 1e-38)).max()))
    assert np.all(d2 <= e2 + 1e-38), ('z2', where, float((d2 / (e2 + 1e-38)).max()))
    assert _sentinel_intact(yw, C), where
    assert bool(torch.isnan(xw[..., :4]).all()) and bool(torch.isnan(xw[..., 4 + K:]).all())
    # a second launch: bit for bit the first
    _, _, yw2, yv2 = _buffers(x, C)
    ops.ghost_fwd(xv, tw1, ts1, th1, a1c, twd, out=yv2, **kw)
    assert torch.equal(yw, yw2), where
    if pair:
        # the pair of launches it replaces, on the same inputs: inside the same float64 bound (not compared bit for bit with the
        # fused result: the summation orders differ)
        _, _, yw3, yv3 = _buffers(x, C)
        ops.pwconv_fwd(xv, tw1, out=yv3[..., :C], **kw)
        ops.dwconv2d_fwd(yv3[..., :C], twd, in_scale=ts1, in_shift=th1, in_act=a1c, out=yv3[..., C:])
        pr = yv3.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(pr[..., :C] - z1) <= e1 + 1e-38), ('pair z1', where)
        assert np.all(np.abs(pr[..., C:] - z2) <= e2 + 1e-38), ('pair z2', where)
        assert _sentinel_intact(yw3, C), where


@pytest.mark.parametrize('K,C', KC)
@pytest.mark.parametrize('prologue', [False, True])
@pytest.mark.parametrize('act1', [True, False])
def test_every_edge(ops, K, C, prologue, act1):
    """W = 1, 2 (narrower than the window), 15, 16, 17 (around the 14-column segment and the 16-lane row), 33 (three segments);
    H = 1, 2, 3 (every row at a border) and 9 (three bands of 4, 4, 1 rows)"""
    for H in HS:
        for W in WS:
            _run(ops, 2, H, W, K, C, prologue, act1, seed=H * 100 + W + K + C, pair=(H, W) in ((9, 33), (1, 1), (3, 17)))


def test_many_bands_and_workgroups(ops):
    """2 x 128 x 128, 24 -> 36: ten segments x 32 bands x 2 images = 640 waves in 160 workgroups, three channel tiles per wave
    with the last one a quarter full"""
    _run(ops, 2, 128, 128, 24, 36, True, True, seed=5)


@pytest.mark.parametrize('K,C', [(20, 8), (16, 6), (48, 24), (16, 52)])
def test_unsupported_shapes_are_refused_without_a_launch(ops, K, C):
    N, H, W = 1, 4, 4
    assert not ops.ghost_fwd_supported((N, H, W, K), C)
    Cp = (C + 3) // 4 * 4
    x = torch.zeros((N, H, W, K), dtype=torch.float32, device=DEV)
    yw = torch.full((N, H, W, 2 * Cp + 8), SENTINEL, dtype=torch.float32, device=DEV)
    w1, s1, wdw = torch.zeros((K, C), device=DEV), torch.ones(C, device=DEV), torch.zeros((3, 3, C), device=DEV)
    with pytest.raises(Exception, match='unsupported shape'):
        ops.ghost_fwd(x, w1, s1, s1, ops.ACT_RELU, wdw, out=yw[..., 4:4 + 2 * Cp])
    torch.cuda.synchronize()
    assert bool((yw == SENTINEL).all())


def test_bad_layout_is_refused(ops):
    x = torch.zeros((1, 4, 4, 18), dtype=torch.float32, device=DEV)
    w1, s1, wdw = torch.zeros((16, 8), device=DEV), torch.ones(8, device=DEV), torch.zeros((3, 3, 8), device=DEV)
    with pytest.raises(Exception, match='bad layout'):
        ops.ghost_fwd(x[..., 1:17], w1, s1, s1, ops.ACT_NONE, wdw)                     # ld 18, base off the 16-byte grid
    with pytest.raises(Exception, match='bad layout'):
        ops.ghost_fwd(torch.zeros((1, 4, 4, 16), device=DEV), w1, s1, s1, ops.ACT_NONE, wdw,
                      out=torch.zeros((1, 4, 4, 12), device=DEV))                      # 2C = 16 channels do not fit ld 12
