"""The 2x2 stride-2 transposed convolution (csrc/deconv.hip) against float64 NumPy, role by role.

Bounds are the ones tests/test_ops_gpu.py applies to the pointwise GEMM through its close(): forward and data gradient rtol 2e-4 +
atol 2e-5 of the scale, weight and bias gradient rtol 3e-4.  The shapes are the smallest at which each mechanism can go wrong:
  rows   one 1x1 image (M = 1); M = 63, 64, 65 (one row tile of a wave group, exactly, and one over); N = 2 with an odd width
         (the image boundary in the row decode m -> (n, 2y+dy, 2x+dx)); more 128-row tiles than workgroups (the persistent loop)
  Cin    4, 20 (a partial K step), 32 (exactly one), 36 (one and a remainder)
  Cout   4 (a 64-column tile spans all four quadrants), 20 (quadrants cut off the 16-column boundaries), 64 (a quadrant is a tile),
         72 (a quadrant wider than a tile)
"""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FILLS = (float('nan'), float('inf'), float('-inf'))     # the canaries of tests/test_view_isolation_gpu.py
SENTINEL = 7.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def close(got, want, rtol=2e-4, atol=2e-5, what=''):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = np.abs(got - want).max()
    assert err <= atol * scale + rtol * scale, '%s: max err %g (scale %g)' % (what, err, scale)


def _act(v, act):
    if act == 'relu':
        return np.maximum(v, 0.0)
    if act == 'relu6':
        return np.clip(v, 0.0, 6.0)
    return v


def ref_fwd(a, w, bias):
    """a (N,H,W,Cin) already activated, w (2,2,Cout,Cin) -> (N,2H,2W,Cout), float64"""
    N, H, W, _ = a.shape
    y = np.einsum('nhwi,pqoi->nhpwqo', a, w).reshape(N, 2 * H, 2 * W, w.shape[2])
    return y if bias is None else y + bias


def ref_bwd_data(dy, w):
    N, H2, W2, Cout = dy.shape
    return np.einsum('nhpwqo,pqoi->nhwi', dy.reshape(N, H2 // 2, 2, W2 // 2, 2, Cout), w)


def ref_bwd_weight(a, dy):
    N, H, W, _ = a.shape
    return np.einsum('nhwi,nhpwqo->pqoi', a, dy.reshape(N, H, 2, W, 2, dy.shape[-1])), dy.sum((0, 1, 2))


def _data(N, H, W, Cin, Cout, seed=0):
    r = np.random.RandomState(1000 * seed + 7 * N + 31 * H + 17 * W + Cin + 3 * Cout)
    f = lambda *s: r.standard_normal(s).astype(np.float32).astype(np.float64)     # noqa: E731
    x, dy = f(N, H, W, Cin), f(N, 2 * H, 2 * W, Cout)
    w = f(2, 2, Cout, Cin) / np.sqrt(Cin)
    w = w.astype(np.float32).astype(np.float64)
    bias = f(Cout)
    sc = (r.rand(Cin) + 0.5).astype(np.float32).astype(np.float64)
    sh = (0.3 * r.standard_normal(Cin)).astype(np.float32).astype(np.float64)
    return x, dy, w, bias, sc, sh


def _all_roles(ops, N, H, W, Cin, Cout, act='relu', bias=True, accumulate=False):
    x, dy, w, b, sc, sh = _data(N, H, W, Cin, Cout)
    pro = {'none': (None, None, ops.ACT_NONE), 'relu': (T(sc), T(sh), ops.ACT_RELU), 'relu6': (T(4 * sc), T(sh + 2), ops.ACT_RELU6)}[act]
    a = {'none': x, 'relu': _act(x * sc + sh, 'relu'), 'relu6': _act(x * 4 * sc + (sh + 2), 'relu6')}[act]
    tag = '%dx%dx%d %d->%d %s' % (N, H, W, Cin, Cout, act)
    y = ops.deconv2x2_fwd(T(x), T(w), T(b) if bias else None, *pro)
    close(y, ref_fwd(a, w, b if bias else None), what='fwd ' + tag)
    base = np.random.RandomState(5).standard_normal((N, H, W, Cin)).astype(np.float32).astype(np.float64)
    gx = ops.deconv2x2_bwd_data(T(dy), T(w), out=T(base) if accumulate else None, accumulate=accumulate)
    close(gx, ref_bwd_data(dy, w) + (base if accumulate else 0.0), what='bwd data ' + tag)
    gw, gb = ops.deconv2x2_bwd_weight(T(x), T(dy), *pro, with_bias=True)
    gw_ref, gb_ref = ref_bwd_weight(a, dy)
    close(gw, gw_ref, rtol=3e-4, what='bwd weight ' + tag)
    close(gb, gb_ref, rtol=3e-4, what='bwd bias ' + tag)
    gw2 = ops.deconv2x2_bwd_weight(T(x), T(dy), *pro)         # without the bias gradient
    assert torch.equal(gw, gw2)


# M = 1, 63, 64, 65, and two images of odd width
@pytest.mark.parametrize('N,H,W', [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (2, 3, 5)])
def test_rows(ops, N, H, W):
    _all_roles(ops, N, H, W, 20, 20)


@pytest.mark.parametrize('Cout', [4, 20, 64, 72])
@pytest.mark.parametrize('Cin', [4, 20, 32, 36])
def test_channels(ops, Cin, Cout):
    _all_roles(ops, 2, 3, 5, Cin, Cout)
    _all_roles(ops, 1, 9, 15, Cin, Cout, act='none')       # M = 135: a second row tile, partly filled


@pytest.fixture
def plan():
    L = load_pkg('_lib').lib()
    yield L.deconv2x2_set_plan
    L.deconv2x2_set_plan(0)


def test_more_row_tiles_than_workgroups(ops, plan):
    """N = 2, 96 x 96, Cin 8, Cout 4: 144 row tiles of 128.  The default plan gives each its own workgroup; pinned to 8 workgroups every
    one walks 18 tiles (the persistent loop, its prefetch across tile boundaries and the accumulator reset), and 5 leaves the last
    workgroups one tile short.  All three give the same bits: the tile a row belongs to does not depend on the plan."""
    N, H, W, Cin, Cout = 2, 96, 96, 8, 4
    x, dy, w, b, sc, sh = _data(N, H, W, Cin, Cout)
    a = _act(x * sc + sh, 'relu')
    want_y, want_gx = ref_fwd(a, w, b), ref_bwd_data(dy, w)
    got = []
    for wgs in (0, 8, 5):
        plan(wgs)
        y = ops.deconv2x2_fwd(T(x), T(w), T(b), T(sc), T(sh), ops.ACT_RELU)
        gx = ops.deconv2x2_bwd_data(T(dy), T(w))
        close(y, want_y, what='fwd, %d workgroups' % wgs)
        close(gx, want_gx, what='bwd data, %d workgroups' % wgs)
        got.append((y, gx))
    for y, gx in got[1:]:
        assert torch.equal(y, got[0][0]) and torch.equal(gx, got[0][1])
    gw, gb = ops.deconv2x2_bwd_weight(T(x), T(dy), T(sc), T(sh), ops.ACT_RELU, with_bias=True)     # 72 slices of 256 rows
    gw_ref, gb_ref = ref_bwd_weight(a, dy)
    close(gw, gw_ref, rtol=3e-4, what='bwd weight')
    close(gb, gb_ref, rtol=3e-4, what='bwd bias')


@pytest.mark.parametrize('act', ['none', 'relu', 'relu6'])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('accumulate', [False, True])
def test_prologue_bias_accumulate(ops, act, bias, accumulate):
    _all_roles(ops, 2, 5, 7, 36, 20, act=act, bias=bias, accumulate=accumulate)


def _view(a, lo, hi, fill):
    """a (..., C) inside channels [lo, lo + C) of a buffer filled with `fill`"""
    C = a.shape[-1]
    buf = torch.full(tuple(a.shape[:-1]) + (lo + C + hi,), fill, dtype=torch.float32, device=DEV)
    buf[..., lo:lo + C] = a
    return buf, buf[..., lo:lo + C]


def _outside_is(buf, lo, C, fill):
    ref = torch.full_like(buf, fill)
    m = torch.ones(buf.shape[-1], dtype=torch.bool, device=DEV)
    m[lo:lo + C] = False
    return torch.equal(buf[..., m].contiguous().view(torch.int32), ref[..., m].contiguous().view(torch.int32))


@pytest.mark.parametrize('Cin,Cout', [(20, 20), (36, 72)])
def test_views(ops, Cin, Cout):
    """x, y, dy and gx as channel slices (ld > C, non-zero channel offset) of buffers whose other channels hold NaN / +Inf / -Inf:
    every result is bitwise the contiguous one, every element inside an output slice is written, nothing outside it changes"""
    N, H, W = 2, 5, 7
    x, dy, w, b, sc, sh = _data(N, H, W, Cin, Cout)
    pro = (T(sc), T(sh), ops.ACT_RELU)
    y0 = ops.deconv2x2_fwd(T(x), T(w), T(b), *pro)
    gx0 = ops.deconv2x2_bwd_data(T(dy), T(w))
    gw0, gb0 = ops.deconv2x2_bwd_weight(T(x), T(dy), *pro, with_bias=True)
    for fill in FILLS:
        _, xv = _view(T(x), 8, 12, fill)
        ybuf, yv = _view(torch.full((N, 2 * H, 2 * W, Cout), float('nan'), device=DEV), 16, 4, fill)
        ops.deconv2x2_fwd(xv, T(w), T(b), *pro, out=yv)
        assert torch.equal(yv, y0), 'forward differs with %r beside the views' % fill       # (finite everywhere: all written)
        assert _outside_is(ybuf, 16, Cout, fill)
        _, dv = _view(T(dy), 4, 8, fill)
        gbuf, gv = _view(torch.full((N, H, W, Cin), float('nan'), device=DEV), 12, 20, fill)
        ops.deconv2x2_bwd_data(dv, T(w), out=gv)
        assert torch.equal(gv, gx0), 'data gradient differs with %r beside the views' % fill
        assert _outside_is(gbuf, 12, Cin, fill)
        gw, gb = ops.deconv2x2_bwd_weight(xv, dv, *pro, with_bias=True)
        assert torch.equal(gw, gw0) and torch.equal(gb, gb0), 'weight gradient differs with %r beside the views' % fill
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(gx0).all()) and bool(torch.isfinite(gw0).all())


def test_weight_gradient_is_bitwise_repeatable(ops):
    x, dy, w, b, sc, sh = _data(2, 40, 24, 36, 20)         # M = 1920: eight slices of M
    a = ops.deconv2x2_bwd_weight(T(x), T(dy), T(sc), T(sh), ops.ACT_RELU, with_bias=True)
    c = ops.deconv2x2_bwd_weight(T(x), T(dy), T(sc), T(sh), ops.ACT_RELU, with_bias=True)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize('N,H,W,Cin,Cout', [(2, 3, 5, 36, 20), (1, 9, 15, 32, 64)])
def test_forward_is_the_pointwise_gemm_then_depth_to_space(ops, N, H, W, Cin, Cout):
    """y == depth_to_space(pwconv_fwd(x, w as [Cin][4 Cout])) to 2 ulp of sum |a w| per element (the two kernels may associate the
    sum differently)"""
    x, dy, w, b, sc, sh = _data(N, H, W, Cin, Cout)
    y = ops.deconv2x2_fwd(T(x), T(w), T(b), T(sc), T(sh), ops.ACT_RELU).cpu().numpy()
    wk = np.ascontiguousarray(w.reshape(4 * Cout, Cin).T)
    flat = ops.pwconv_fwd(T(x).reshape(-1, Cin), T(wk), T(np.tile(b, 4)), T(sc), T(sh), ops.ACT_RELU).cpu().numpy()
    d2s = flat.reshape(N, H, W, 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Cout)
    a = _act(x * sc + sh, 'relu')
    mag = ref_fwd(np.abs(a), np.abs(w), np.abs(b))
    bound = 2.0 * np.spacing(mag.astype(np.float32)).astype(np.float64)
    err = np.abs(y.astype(np.float64) - d2s.astype(np.float64))
    print('max err / bound: %.3f' % float((err / bound).max()))
    assert (err <= bound).all()
