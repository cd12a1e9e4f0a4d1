"""No kernel reads the channels beside its view.

A PeleeNet dense block is one NHWC buffer: every Concatenate is a prefix view [0, c) of it and every branch conv writes into a
16-channel slice, so most launches read a view whose row stride is wider than its channel count, and most of the
buffer sits beside the view.  Each case below runs one op wrapper on channel-slice views whose neighbouring channels hold zeros,
then NaN, +Inf and -Inf, and asserts that every output is BITWISE the zero-neighbour one and finite, and that the channels beside
an output slice are untouched.  The kernels are deterministic, so bit equality is the oracle: a K tail zeroed by multiplying with a
zero coefficient (NaN x 0 = NaN), a stride mistaken for the channel count or a vector load that runs past the view fails here even
where finite neighbours would have cancelled."""
import ctypes

import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FILLS = (float('nan'), float('inf'), float('-inf'))
SENTINEL = 7.0


class Bufs:
    """the views of one run: inputs inside buffers whose other channels hold `fill`, outputs inside buffers whose other channels
    hold SENTINEL"""

    def __init__(self, fill):
        self.fill, self.outs = fill, []

    def x(self, a, lo=0, hi=32):
        """a (..., C) in channels [lo, lo + C) of a buffer lo + C + hi wide (lo = 0: the prefix view of a dense block)"""
        C = a.shape[-1]
        buf = torch.full(a.shape[:-1] + (lo + C + hi,), self.fill, dtype=a.dtype, device=DEV)
        buf[..., lo:lo + C] = a
        return buf[..., lo:lo + C]

    def out(self, shape, dtype=torch.float32, lo=16, hi=12, base=None):
        """an output slice [lo, lo + C) of a wider buffer (base: its starting content, for the accumulating forms)"""
        C = shape[-1]
        buf = torch.full(tuple(shape[:-1]) + (lo + C + hi,), SENTINEL, dtype=dtype, device=DEV)
        if base is not None:
            buf[..., lo:lo + C] = base
        self.outs.append((buf, lo, C))
        return buf[..., lo:lo + C]

    def untouched(self):
        for buf, lo, C in self.outs:
            assert bool((buf[..., :lo] == SENTINEL).all()) and bool((buf[..., lo + C:] == SENTINEL).all())


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run(case, ops):
    """the case at fill 0 and at every non-finite fill: outputs bitwise equal and finite, output neighbours untouched"""
    b0 = Bufs(0.0)
    ref = [t.clone() for t in case(ops, b0)]
    b0.untouched()
    for t in ref:
        assert bool(torch.isfinite(t.float()).all())
    for fill in FILLS:
        b = Bufs(fill)
        got = case(ops, b)
        for i, (r, t) in enumerate(zip(ref, got)):
            assert torch.equal(_bits(r), _bits(t)), 'output %d differs with %r beside the views (max |diff| %s)' % (
                i, fill, float((r.float() - t.float()).abs().nan_to_num(float('inf')).max()))
        b.untouched()


def _coef(g, C, dtype=torch.float32):
    sc = torch.rand(C, device=DEV, generator=g) + 0.5
    sh = torch.randn(C, device=DEV, generator=g) * 0.3
    return sc.to(dtype).float(), sh.to(dtype).float()


@pytest.fixture
def option():
    """set_option(name, value) for the test, restored to the value conftest / the production rule uses afterwards"""
    L = load_pkg('_lib').lib()
    restore = []

    def set_(name, value, back):
        L.set_option(name, value)
        restore.append((name, back))
    yield set_
    for name, back in reversed(restore):
        L.set_option(name, back)


# ------------------------------------------------------------------------------------------------------- pointwise GEMMs
# (M, K, N): the few-row kernels (M <= 64), the small-K.N streaming kernels (conftest's pw_small_min_rows = 64), the tiled GEMM
PW_FWD = [(17, 44, 32), (3001, 36, 24), (4099, 100, 96)]


@pytest.mark.parametrize('M,K,N', PW_FWD)
@pytest.mark.parametrize('act', ['none', 'relu'])
def test_pwconv_fwd(ops, M, K, N, act):
    def case(ops, b):
        g = _gen(M + K)
        x = torch.randn(M, K, device=DEV, generator=g)
        w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
        sc, sh = _coef(g, K)
        pro = (sc, sh, ops.ACT_RELU) if act == 'relu' else (sc, sh, ops.ACT_NONE)
        part = ops.new_partials(N, DEV)
        y, rows = ops.pwconv_fwd(b.x(x), w, None, *pro, out=b.out((M, N)), partials=part)
        y2 = ops.pwconv_fwd(b.x(x, lo=4, hi=28), w, out=b.out((M, N)))          # bare operand, a slice at an offset
        return [y, part[:rows * 2 * N], y2]
    _run(case, ops)


@pytest.mark.parametrize('M,K,N', [(4099, 100, 96), (70001, 36, 24)])
def test_pwconv_fwd_tiled(ops, option, M, K, N):
    """the tiled fp32 GEMMs (csrc/pwconv.hip, both kernel layouts) with the streaming kernels kept out.  Their K-tail loads are clamped
    to the view's last quad and then zeroed by a select, so the channels beside a prefix view are never read"""
    option(b'pw_small_min_rows', 1 << 30, 64)

    def case(ops, b):
        g = _gen(M + K + 1)
        x = torch.randn(M, K, device=DEV, generator=g)
        w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
        sc, sh = _coef(g, K)
        part = ops.new_partials(N, DEV)
        y, rows = ops.pwconv_fwd(b.x(x), w, None, sc, sh, ops.ACT_NONE, out=b.out((M, N)), partials=part)
        y2 = ops.pwconv_fwd(b.x(x, lo=4, hi=28), w, out=b.out((M, N)))
        # the transposed-kernel entry point (the executor's): the other tiled kernel, with its own K-tail select
        part2 = ops.new_partials(N, DEV)
        y3, rows3 = ops.pwconv_fwd_wt(b.x(x), w.t().contiguous(), None, sc, sh, ops.ACT_NONE, out=b.out((M, N)), partials=part2)
        return [y, part[:rows * 2 * N], y2, y3, part2[:rows3 * 2 * N]]
    _run(case, ops)


@pytest.mark.parametrize('M,K,N', PW_FWD)
def test_pwconv_bwd(ops, M, K, N):
    def case(ops, b):
        g = _gen(M + 2 * K)
        x = torch.randn(M, K, device=DEV, generator=g)
        dy = torch.randn(M, N, device=DEV, generator=g)
        w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
        sc, sh = _coef(g, K)
        base = torch.randn(M, K, device=DEV, generator=g)
        gx = ops.pwconv_bwd_data(b.x(dy, lo=16, hi=16), w, out=b.out((M, K)))
        acc = ops.pwconv_bwd_data(b.x(dy, lo=16, hi=16), w, out=b.out((M, K), base=base), accumulate=True)
        gw = ops.pwconv_bwd_weight(b.x(x), b.x(dy, lo=16, hi=16), sc, sh, ops.ACT_RELU)
        return [gx, acc, gw]
    _run(case, ops)


@pytest.mark.parametrize('act', ['none', 'relu'])
def test_pwconv_fwd_sb_pinned_schedule(ops, option, act):
    """the pinned-schedule split forward (csrc/pw_split3.hip) with a K tail inside its last K-step (K = 300, pitch 320), a prologue,
    and the operand a prefix view (ldx > K): the tail k = 300 .. 319 of every row reads the neighbouring channels"""
    M, K, N = 65536 + 100, 300, 256
    option(b'pw_small_min_rows', -1, 64)
    option(b'sb3', 1, -1)
    plan = (ctypes.c_int * 6)()
    ops.lib().gemm_plan_query(6, M, K, N, plan)          # (role 6: forward with statistics; wm 4 is the pinned form)
    assert plan[3] == 4, list(plan)

    def case(ops, b):
        g = _gen(K)
        x = torch.randn(M, K, device=DEV, generator=g)
        wsp = ops.split_bf16x3(torch.randn(N, K, device=DEV, generator=g) / K ** 0.5)
        sc, sh = _coef(g, K)
        actc = ops.ACT_RELU if act == 'relu' else ops.ACT_NONE
        part = ops.new_partials(N, DEV)
        y, rows = ops.pwconv_fwd_sb(b.x(x, hi=20), wsp, K, None, sc, sh, actc, out=b.out((M, N)), partials=part)
        return [y, part[:rows * 2 * N]]
    _run(case, ops)


@pytest.mark.parametrize('M,K', [(4099, 100), (70001, 304)])
def test_pwconv_fwd_sb_tiled(ops, option, M, K):
    """the tiled split forward (csrc/pw_split.hip) on a prefix view with a K tail"""
    N = 256 if M > 65536 else 96
    option(b'sb3', 0, -1)

    def case(ops, b):
        g = _gen(M + K)
        x = torch.randn(M, K, device=DEV, generator=g)
        wsp = ops.split_bf16x3(torch.randn(N, K, device=DEV, generator=g) / K ** 0.5)
        sc, sh = _coef(g, K)
        part = ops.new_partials(N, DEV)
        y, rows = ops.pwconv_fwd_sb(b.x(x, hi=20), wsp, K, None, sc, sh, ops.ACT_NONE, out=b.out((M, N)), partials=part)
        return [y, part[:rows * 2 * N]]
    _run(case, ops)


# ------------------------------------------------------------------------------------------------------- dense convs
# (N, H, W, Cin, Cout, k, stride): the dense layers' 3x3 (Cout 16) and the stem2b geometry (stride 2, 16 -> 32); >= 1024 output rows,
# the split kernels' minimum
DENSE = [(4, 18, 26, 32, 16, 3, 1), (4, 34, 40, 16, 32, 3, 2)]


@pytest.mark.parametrize('case_', DENSE)
@pytest.mark.parametrize('split', [False, True])
def test_conv2d_gemm(ops, option, case_, split):
    N, H, W, Cin, Cout, k, s = case_
    if split:
        option(b'conv_sb', 2, -1)
    fwd = ops.conv2d_gemm_fwd_sb if split else ops.conv2d_gemm_fwd
    bwd = ops.conv2d_gemm_bwd_data_sb if split else ops.conv2d_gemm_bwd_data

    def case(ops, b):
        g = _gen(Cin + Cout + s)
        x = torch.randn(N, H, W, Cin, device=DEV, generator=g)
        w = torch.randn(k, k, Cin, Cout, device=DEV, generator=g) / (k * k * Cin) ** 0.5
        sc, sh = _coef(g, Cin)
        part = ops.new_partials(Cout, DEV)
        y, rows = fwd(b.x(x), w, s, 1, 'same', sc, sh, ops.ACT_RELU, partials=part)
        y2 = fwd(b.x(x, lo=8, hi=24), w, s, 1, 'same')
        dy = torch.randn(y.shape, device=DEV, generator=g)
        gx = bwd(b.x(dy, lo=16, hi=16), w, (N, H, W, Cin), s, 1, 'same', out=b.out((N, H, W, Cin)))
        base = torch.randn(N, H, W, Cin, device=DEV, generator=g)
        acc = bwd(b.x(dy, lo=16, hi=16), w, (N, H, W, Cin), s, 1, 'same', out=b.out((N, H, W, Cin), base=base), accumulate=True)
        gw = ops.conv2d_gemm_bwd_weight(b.x(x), b.x(dy, lo=16, hi=16), k, s, 1, 'same', sc, sh, ops.ACT_RELU)
        return [y, part[:rows * 2 * Cout], y2, gx, acc, gw]
    _run(case, ops)


@pytest.mark.parametrize('Cin,Cout', [(32, 16), (12, 8), (64, 32)])
def test_conv_narrow(ops, Cin, Cout):
    N, H, W = 2, 9, 17

    def case(ops, b):
        g = _gen(Cin + Cout)
        x = torch.randn(N, H, W, Cin, device=DEV, generator=g)
        w = torch.randn(3, 3, Cin, Cout, device=DEV, generator=g) / (9 * Cin) ** 0.5
        sc, sh = _coef(g, Cin)
        y, part = ops.conv_narrow_fwd(b.x(x), w, sc, sh, ops.ACT_RELU, out=b.out((N, H, W, Cout)), stats=True)
        y2 = ops.conv_narrow_fwd(b.x(x, lo=4, hi=28), w, out=b.out((N, H, W, Cout)))
        dy = torch.randn(N, H, W, Cout, device=DEV, generator=g)
        gx = ops.conv_narrow_bwd_data(b.x(dy, lo=16, hi=16), w, out=b.out((N, H, W, Cin)))
        base = torch.randn(N, H, W, Cin, device=DEV, generator=g)
        acc = ops.conv_narrow_bwd_data(b.x(dy, lo=16, hi=16), w, out=b.out((N, H, W, Cin), base=base), accumulate=True)
        gw = ops.conv_narrow_bwd_weight(b.x(x), b.x(dy, lo=16, hi=16), sc, sh, ops.ACT_RELU)
        return [y, part, y2, gx, acc, gw]
    _run(case, ops)


# ------------------------------------------------------------------------------------------------------- depthwise
@pytest.mark.parametrize('C,k,stride,rate', [(32, 3, 1, 1), (24, 3, 2, 1), (16, 3, 1, 6), (40, 5, 1, 1)])
def test_dwconv(ops, C, k, stride, rate):
    N, H, W = 2, 19, 23

    def case(ops, b):
        g = _gen(C + k + stride + rate)
        x = torch.randn(N, H, W, C, device=DEV, generator=g)
        w = torch.randn(k, k, C, device=DEV, generator=g) / k
        sc, sh = _coef(g, C)
        part = ops.new_partials(C, DEV)
        y, rows = ops.dwconv2d_fwd(b.x(x), w, stride, rate, 'same', sc, sh, ops.ACT_RELU6, partials=part)
        dy = torch.randn(y.shape, device=DEV, generator=g)
        gx = ops.dwconv2d_bwd_data(b.x(dy, lo=16, hi=16), w, (N, H, W, C), stride, rate, 'same', out=b.out((N, H, W, C)))
        gw = ops.dwconv2d_bwd_weight(b.x(x), b.x(dy, lo=16, hi=16), k, stride, rate, 'same', sc, sh, ops.ACT_RELU6)
        return [y, part[:rows * 2 * C], gx, gw]
    _run(case, ops)


# ------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize('bf16', [False, True])
def test_maxpool(ops, bf16):
    N, H, W, C, k, s, pad = 2, 15, 17, 32, 2, 2, (0, 0, 0, 0)
    dt = torch.bfloat16 if bf16 else torch.float32

    def case(ops, b):
        g = _gen(C + int(bf16))
        x = torch.randn(N, H, W, C, device=DEV, generator=g).to(dt)
        sc, sh = _coef(g, C)
        Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
        am = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8, device=DEV)
        if bf16:
            y = ops.maxpool2d_fwd_bf16(b.x(x), k, s, pad, sc, sh, ops.ACT_RELU, argmax=am)
            dy = torch.randn(y.shape, device=DEV, generator=g).to(dt)
            gx = ops.maxpool2d_bwd_bf16(b.x(dy, lo=16, hi=16), am, (N, H, W, C), k, s, pad, out=b.out((N, H, W, C), dt))
        else:
            y = ops.maxpool2d_fwd(b.x(x), k, s, pad, sc, sh, ops.ACT_RELU, argmax=am)
            dy = torch.randn(y.shape, device=DEV, generator=g)
            gx = ops.maxpool2d_bwd(b.x(x), b.x(dy, lo=16, hi=16), k, s, pad, sc, sh, ops.ACT_RELU, out=b.out((N, H, W, C)))
            gx2 = ops.maxpool2d_bwd(b.x(x), b.x(dy, lo=16, hi=16), k, s, pad, sc, sh, ops.ACT_RELU, out=b.out((N, H, W, C)),
                                    argmax=am)
            return [y, am, gx, gx2]
        return [y, am, gx]
    _run(case, ops)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('k,s', [(2, 2), (3, 2)])
def test_avgpool(ops, bf16, k, s):
    N, H, W, C = 2, 15, 17, 32
    dt = torch.bfloat16 if bf16 else torch.float32
    fwd, bwd = (ops.avgpool2d_fwd_bf16, ops.avgpool2d_bwd_bf16) if bf16 else (ops.avgpool2d_fwd, ops.avgpool2d_bwd)

    def case(ops, b):
        g = _gen(C + k + int(bf16))
        x = torch.randn(N, H, W, C, device=DEV, generator=g).to(dt)
        sc, sh = _coef(g, C)
        Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
        y = fwd(b.x(x), k, s, sc, sh, ops.ACT_RELU, out=b.out((N, Ho, Wo, C), dt))
        dy = torch.randn(N, Ho, Wo, C, device=DEV, generator=g).to(dt)
        gx = bwd(b.x(dy, lo=16, hi=16), (N, H, W, C), k, s, out=b.out((N, H, W, C), dt))
        base = torch.randn(N, H, W, C, device=DEV, generator=g).to(dt)
        acc = bwd(b.x(dy, lo=16, hi=16), (N, H, W, C), k, s, out=b.out((N, H, W, C), dt, base=base), accumulate=True)
        return [y, gx, acc]
    _run(case, ops)


def test_global_avgpool(ops):
    N, H, W, C = 3, 33, 31, 48

    def case(ops, b):
        g = _gen(C)
        x = torch.randn(N, H, W, C, device=DEV, generator=g)
        sc, sh = _coef(g, C)
        y = ops.global_avgpool_fwd(b.x(x), sc, sh, ops.ACT_RELU, out=b.out((N, 1, 1, C)))
        y1 = ops.global_avgpool_fwd(b.x(x, lo=8, hi=24), chunked=False)
        return [y, y1]
    _run(case, ops)


# ------------------------------------------------------------------------------------------------------- elementwise / resize
def test_affine_act(ops):
    N, H, W, C = 2, 13, 11, 36

    def case(ops, b):
        g = _gen(C)
        x = torch.randn(N, H, W, C, device=DEV, generator=g)
        r = torch.randn(N, H, W, C, device=DEV, generator=g)
        sc, sh = _coef(g, C)
        rs, rt = _coef(g, C)
        y = ops.affine_act(b.x(x), sc, sh, ops.ACT_RELU, out=b.out((N, H, W, C)))
        y2 = ops.affine_act(b.x(x), sc, sh, ops.ACT_NONE, residual=b.x(r, lo=4, hi=28), rscale=rs, rshift=rt, ract=ops.ACT_RELU6,
                            out=b.out((N, H, W, C)))
        return [y, y2]
    _run(case, ops)


@pytest.mark.parametrize('h,w,H,W', [(17, 13, 65, 49), (33, 33, 129, 129)])
def test_resize_bilinear(ops, h, w, H, W):
    N, C = 2, 24

    def case(ops, b):
        g = _gen(h + C)
        x = torch.randn(N, h, w, C, device=DEV, generator=g)
        y = ops.resize_bilinear_fwd(b.x(x), H, W, out=b.out((N, H, W, C)))
        dy = torch.randn(N, H, W, C, device=DEV, generator=g)
        gx = ops.resize_bilinear_bwd(b.x(dy, lo=16, hi=16), h, w, out=b.out((N, h, w, C)))
        return [y, gx]
    _run(case, ops)

