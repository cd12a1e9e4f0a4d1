"""The fp32 GEMMs past their last row and at the 4 GiB byte-offset edge.

Every fp32 pointwise / implicit-GEMM kernel addresses its operands with 32-bit byte offsets, and the entry points refuse operands of
4 GiB or more (`M * ld * 4 < 2^32`).  Two things can still go wrong below that guard:
  * the tile loop covers whole tiles: rows past M are computed, and their loads / stores are left to the buffer range check (which
    counts the SGPR offset on gfx950).  The tail canaries below put canary bit patterns (NaN payload, +Inf, -Inf) after the last row
    and beside the output columns of every fp32 entry point that writes rows, at M = 1 and 127 (mod 128).
  * a kernel that computes offsets for rows PAST M (padding rows of the last tile, the prefetch one grid stride ahead) can wrap those
    offsets past 2^32 although every real row is below the guard.  A wrapped offset lands inside the operand, so the range check
    does not drop it.  The pinned-schedule kernels (csrc/pw_split3.hip) are such kernels; their support rules take the leading
    dimensions and refuse launches whose padding or prefetch offsets would wrap.  The edge cases below sit just under the entry
    points' guard, where the pinned forms used to wrap, and check that the launch is correct and writes only its own rows.

Addresses: every wrapped offset is below 2^32 and every access is range-checked against the operand's own extent, so the accesses
of these launches stay inside [base, base + 4 GiB) of each operand; every buffer an operand may wrap in reaches that far.  The float64
references run on the device, in chunks, on sampled rows plus full-length column sums."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GIB4 = 1 << 32
CANARY = (0x7fc0dead, 0x7f800000, 0xff800000 - (1 << 32))      # NaN with a payload, +Inf, -Inf (as int32 bit patterns)
TILE = 128
NUM_CUS = 256


# ------------------------------------------------------------------------------------------------------------------- helpers
def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _pattern(cols):
    return torch.tensor(CANARY, dtype=torch.int32, device=DEV).repeat(cols // 3 + 1)[:cols]


class Canary:
    """a (rows + 128, lo + C + hi) float32 buffer full of the canary pattern; .view is its row-prefix, column-slice [:rows, lo:lo + C]
    (min_bytes: the buffer reaches at least that far from the view's base)"""

    def __init__(self, rows, C, lo=8, hi=24, min_bytes=0):
        self.rows, self.C, self.lo, self.ld = rows, C, lo, lo + C + hi
        total = max(rows + TILE, -(-(min_bytes + lo * 4) // (self.ld * 4)) + 1)
        self.buf = torch.empty(total, self.ld, dtype=torch.float32, device=DEV)
        self.pat = _pattern(self.ld)
        self.buf.view(torch.int32).copy_(self.pat.expand(total, self.ld))
        self.view = self.buf[:rows, lo:lo + C]

    def intact(self, what):
        b = self.buf.view(torch.int32)
        lo, C, M = self.lo, self.C, self.rows
        assert bool((b[M:] == self.pat).all()), '%s: a store landed after the last row' % what
        assert bool((b[:M, :lo] == self.pat[:lo]).all()) and bool((b[:M, lo + C:] == self.pat[lo + C:]).all()), \
            '%s: a store landed beside the output columns' % what


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _act64(u, act, ops):
    if act == ops.ACT_RELU:
        return u.clamp_min(0.0)
    if act == ops.ACT_RELU6:
        return u.clamp(0.0, 6.0)
    return u


def _dact64(u, act, ops):
    if act == ops.ACT_RELU:
        return (u > 0).double()
    if act == ops.ACT_RELU6:
        return ((u > 0) & (u < 6)).double()
    return torch.ones_like(u)


def _stat_sums(part, rows, N):
    return part[:rows * 2 * N].reshape(rows, 2, N).double().sum(0)


def _check_stats(p, s1, s2, M, what):
    assert float((p[0] - s1).abs().max()) < 1e-4 * max(float(s1.abs().max()), float(M) ** 0.5), '%s: statistic sum' % what
    assert float((p[1] - s2).abs().max()) < 1e-4 * float(s2.abs().max()), '%s: statistic sum of squares' % what


def _plan(L, role, M, K, N):
    out = (ctypes.c_int * 6)()
    L.gemm_plan_query(role, M, K, N, out)
    return list(out)


class Opts:
    """dl3p_set_option for the test's duration (restored to the suite's values afterwards)"""
    DEFAULTS = {b'sb3': -1, b'sb_rs': -1, b'pw_small_min_rows': 64}

    def __init__(self, L, **kw):
        self.L, self.kw = L, {k.encode(): v for k, v in kw.items()}

    def __enter__(self):
        for k, v in self.kw.items():
            self.L.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            self.L.set_option(k, self.DEFAULTS[k])


def _free_bytes():
    return torch.cuda.mem_get_info()[0]


# ------------------------------------------------------------------------------------------------------------ a. tail canaries
ROW_COUNTS = [65536 + 1, 65536 + 127]        # M = 1 and 127 (mod 128), from the pinned form's 65536 rows up


def _fwd_case(ops, M, K, N, seed, pro=True, bias=False):
    g = _gen(seed)
    x = torch.randn(M, K, device=DEV, generator=g)
    wt = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    sc = torch.rand(K, device=DEV, generator=g) + 0.5 if pro else None
    sh = torch.randn(K, device=DEV, generator=g) * 0.3 + 0.1 if pro else None
    b = torch.randn(N, device=DEV, generator=g) * 0.1 if bias else None
    act = ops.ACT_RELU if pro else ops.ACT_NONE
    a64 = x.double()
    if pro:
        a64 = _act64(a64 * sc.double() + sh.double(), act, ops)
    y64 = a64 @ wt.double().t()
    if bias:
        y64 = y64 + b.double()
    return x, wt, sc, sh, b, act, y64


# forms of the split-bf16 forward: (name, options, statistics, prologue, bias, K, the wm gemm_plan_query must report)
SB_FWD_FORMS = [
    ('pinned_stats', dict(sb3=1), True, True, False, 304, (4,)),
    ('pinned_bias', dict(sb3=1), False, True, True, 304, (4,)),
    ('pinned_plain', dict(sb3=1), False, False, False, 256, (4,)),
    ('tiled_stats', dict(sb3=0), True, True, False, 304, (1, 2)),
    ('tiled_bias', dict(sb3=0), False, True, True, 256, (1, 2)),
    ('row_stationary_stats', dict(sb_rs=1), True, True, False, 304, (3,)),
]


@pytest.mark.parametrize('M', ROW_COUNTS)
@pytest.mark.parametrize('form', SB_FWD_FORMS, ids=lambda f: f[0])
def test_split_forward_writes_no_row_past_the_last(ops, form, M):
    name, opts, stats, pro, bias, K, wms = form
    N = 256
    L = ops.lib()
    with Opts(L, pw_small_min_rows=-1, **opts):
        plan = _plan(L, 5 + int(stats), M, K, N)
        assert plan[0] == 3 and plan[3] in wms, plan
        x, wt, sc, sh, b, act, y64 = _fwd_case(ops, M, K, N, M + K, pro, bias)
        out = Canary(M, N)
        part = ops.new_partials(N, DEV) if stats else None
        res = ops.pwconv_fwd_sb(x, ops.split_bf16x3(wt), K, b, sc, sh, act, out=out.view, partials=part)
        torch.cuda.synchronize()
        out.intact(name)
        assert _rel(out.view, y64) < 2e-5, (name, _rel(out.view, y64))
        if stats:
            _check_stats(_stat_sums(part, res[1], N), y64.sum(0), (y64 * y64).sum(0), M, name)


def _apply_case(ops, M, seed, act, fact):
    K = N = 256
    g_ = _gen(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g_)
    g = rnd(M, N)
    z_out = rnd(M, N).mul_(1.5).add_(0.3)
    bsc, bsh = torch.rand(N, device=DEV, generator=g_) + 0.5, rnd(N) * 0.5
    mu, istd = rnd(N) * 0.2, torch.rand(N, device=DEV, generator=g_) + 0.5
    coef = torch.stack([torch.rand(N, device=DEV, generator=g_) + 0.5, rnd(N) * 0.1, rnd(N) * 0.1]).contiguous()
    w = (rnd(K, N) / N ** 0.5).contiguous()
    z = rnd(M, K)
    sc, sh = torch.rand(K, device=DEV, generator=g_) + 0.5, rnd(K) * 0.3
    mean, invstd = z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
    return g, z_out, bsc, bsh, mu, istd, coef, w, z, sc, sh, mean, invstd


def _apply_ref(ops, rows, g, z_out, bsc, bsh, act, mu, istd, coef, w):
    """float64 dz and gx of the rows `rows` (a slice or an index tensor)"""
    gg, zz = g[rows].double(), z_out[rows].double()
    m = _dact64(zz * bsc.double() + bsh.double(), act, ops)
    dz64 = coef[0].double() * (gg * m - coef[1].double() - (zz - mu.double()) * istd.double() * coef[2].double())
    return dz64, dz64 @ w.double().t()


@pytest.mark.parametrize('M', ROW_COUNTS)
def test_pinned_apply_writes_no_row_past_the_last(ops, M):
    """dl3p_pwconv_bwd_data_sb_apply on the pinned form: dz and gx inside canary buffers, the BatchNorm-backward sums of the front
    layer against float64"""
    L = ops.lib()
    act, fact = ops.ACT_RELU, ops.ACT_RELU
    with Opts(L, sb3=1):
        g, z_out, bsc, bsh, mu, istd, coef, w, z, sc, sh, mean, invstd = _apply_case(ops, M, M + 5, act, fact)
        dzc, gxc = Canary(M, 256), Canary(M, 256, lo=4, hi=12)
        part = ops.new_partials(256, DEV)
        _, _, rows = ops.pwconv_bwd_data_sb_apply(g, z_out, bsc, bsh, act, mu, istd, coef, ops.split_bf16x3(w), 256, dz=dzc.view,
                                                  out=gxc.view, z=z, scale=sc, shift=sh, act=fact, mean=mean, invstd=invstd, partials=part)
        torch.cuda.synchronize()
        assert rows == min(NUM_CUS, -(-M // TILE)), rows            # (one partial row per workgroup: the pinned form took it)
        dzc.intact('dz')
        gxc.intact('gx')
        dz64, gx64 = _apply_ref(ops, slice(None), g, z_out, bsc, bsh, act, mu, istd, coef, w)
        assert _rel(dzc.view, dz64) < 4e-6, ('dz', _rel(dzc.view, dz64))
        assert _rel(gxc.view, gx64) < 2e-5, ('gx', _rel(gxc.view, gx64))
        d = gx64 * _dact64(z.double() * sc.double() + sh.double(), fact, ops)
        xh = (z.double() - mean.double()) * invstd.double()
        p = _stat_sums(part, rows, 256)
        assert float((p[0] - d.sum(0)).abs().max()) < 2e-4 * float(d.abs().sum(0).max()), 'BN backward sum'
        assert float((p[1] - (d * xh).sum(0)).abs().max()) < 2e-4 * float((d * xh).abs().sum(0).max()), 'BN backward sum * xhat'


def _bwd_bn_ref(ops, gx64, z, sc, sh, act, mean, invstd):
    d = gx64 * _dact64(z.double() * sc.double() + sh.double(), act, ops)
    xh = (z.double() - mean.double()) * invstd.double()
    return d.sum(0), (d * xh).sum(0)


DGRAD_FORMS = ['split_tiled', 'split_tiled_bn', 'fp32', 'fp32_bn']


@pytest.mark.parametrize('M', ROW_COUNTS)
@pytest.mark.parametrize('form', DGRAD_FORMS)
def test_data_gradient_writes_no_row_past_the_last(ops, form, M):
    """gx = dy . W^T (K = 304 output columns over a reduction of N = 256) on the split tiled kernel and the fp32 kernel, plain and
    with the fused BatchNorm-backward sums"""
    K, N = 304, 256
    L = ops.lib()
    g_ = _gen(M + 3 * len(form))
    dy = torch.randn(M, N, device=DEV, generator=g_)
    w = (torch.randn(K, N, device=DEV, generator=g_) / N ** 0.5).contiguous()
    gx64 = dy.double() @ w.double().t()
    bn = form.endswith('_bn')
    if bn:
        z = torch.randn(M, K, device=DEV, generator=g_)
        sc, sh = torch.rand(K, device=DEV, generator=g_) + 0.5, torch.randn(K, device=DEV, generator=g_) * 0.3
        mean, invstd = z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
        part = ops.new_partials(K, DEV)
    out = Canary(M, K)
    with Opts(L, sb3=0, sb_rs=0):
        if form.startswith('split'):
            plan = _plan(L, 7 + int(bn), M, N, K)
            assert plan[0] == 3 and plan[3] in (1, 2), plan
            r = ops.pwconv_bwd_data_sb(dy, ops.split_bf16x3(w), N, out=out.view, **(dict(z=z, scale=sc, shift=sh, act=ops.ACT_RELU,
                                       mean=mean, invstd=invstd, partials=part) if bn else {}))
        elif bn:
            r = ops.pwconv_bwd_data_bn(dy, w, z, sc, sh, ops.ACT_RELU, mean, invstd, part, out=out.view)
        else:
            r = ops.pwconv_bwd_data(dy, w, out=out.view)
        torch.cuda.synchronize()
    out.intact(form)
    assert _rel(out.view, gx64) < 2e-5, (form, _rel(out.view, gx64))
    if bn:
        s1, s2 = _bwd_bn_ref(ops, gx64, z, sc, sh, ops.ACT_RELU, mean, invstd)
        p = _stat_sums(part, r[1], K)
        assert float((p[0] - s1).abs().max()) < 2e-4 * float(s1.abs().max()), 'BN backward sum'
        assert float((p[1] - s2).abs().max()) < 2e-4 * float(s2.abs().max()), 'BN backward sum * xhat'


@pytest.mark.parametrize('M', ROW_COUNTS)
def test_fp32_forward_writes_no_row_past_the_last(ops, M):
    K, N = 304, 256
    x, wt, sc, sh, b, act, y64 = _fwd_case(ops, M, K, N, M + 17, True, False)
    out = Canary(M, N)
    part = ops.new_partials(N, DEV)
    _, rows = ops.pwconv_fwd(x, wt.t().contiguous(), None, sc, sh, act, out=out.view, partials=part)
    torch.cuda.synchronize()
    out.intact('pwconv_fwd')
    assert _rel(out.view, y64) < 2e-5, _rel(out.view, y64)
    _check_stats(_stat_sums(part, rows, N), y64.sum(0), (y64 * y64).sum(0), M, 'pwconv_fwd')


@pytest.mark.parametrize('M', [34 * TILE + 1, 34 * TILE - 1])
def test_split_k_forward_writes_no_row_past_the_last(ops, M):
    K, N = 2048, 256
    L = ops.lib()
    assert L.pwconv_fwd_splitk_plan(M, K, N) > 1
    x, wt, sc, sh, b, act, y64 = _fwd_case(ops, M, K, N, M + 19, True, True)
    out = Canary(M, N)
    part = ops.new_partials(N, DEV)
    _, rows = ops.pwconv_fwd_wt_splitk(x, wt, b, sc, sh, act, out=out.view, partials=part)
    torch.cuda.synchronize()
    out.intact('pwconv_fwd_wt_splitk')
    assert _rel(out.view, y64) < 2e-5, _rel(out.view, y64)
    _check_stats(_stat_sums(part, rows, N), y64.sum(0), (y64 * y64).sum(0), M, 'pwconv_fwd_wt_splitk')


@pytest.mark.parametrize('HW', [(129, 129), (127, 129)], ids=['M1mod128', 'M127mod128'])
@pytest.mark.parametrize('split', [False, True], ids=['fp32', 'split'])
def test_implicit_gemm_writes_no_row_past_the_last(ops, split, HW):
    """conv2d_gemm_fwd(_sb) and conv2d_gemm_bwd_data(_sb), 3x3 stride 1 'same' (output rows = input rows = H W)"""
    import torch.nn.functional as F
    H, W = HW
    Cin, Cout, k = 32, 64, 3
    assert ops.conv2d_gemm_supported(Cin, Cout, k, 1)
    M = H * W
    g_ = _gen(M + int(split))
    x = torch.randn(1, H, W, Cin, device=DEV, generator=g_)
    w = torch.randn(k, k, Cin, Cout, device=DEV, generator=g_) / (k * k * Cin) ** 0.5
    dy = torch.randn(1, H, W, Cout, device=DEV, generator=g_)
    w64 = w.double().permute(3, 2, 0, 1)
    y64 = F.conv2d(x.double().permute(0, 3, 1, 2), w64, padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
    gx64 = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w64, padding=1).permute(0, 2, 3, 1).reshape(M, Cin)
    yc, gc = Canary(M, Cout), Canary(M, Cin)
    fwd = ops.conv2d_gemm_fwd_sb if split else ops.conv2d_gemm_fwd
    bwd = ops.conv2d_gemm_bwd_data_sb if split else ops.conv2d_gemm_bwd_data
    fwd(x, w, out=yc.view.view(1, H, W, Cout))
    bwd(dy, w, x.shape, out=gc.view.view(1, H, W, Cin))
    torch.cuda.synchronize()
    yc.intact('forward')
    gc.intact('data gradient')
    assert _rel(yc.view, y64) < 2e-5, ('forward', _rel(yc.view, y64))
    assert _rel(gc.view, gx64) < 2e-5, ('data gradient', _rel(gc.view, gx64))


# ------------------------------------------------------------------------------------------------- b. the 4 GiB edge of the pinned forms
PREFIX = 65536
CHUNK = 1 << 18


def _pinned_fits(M, lds):
    """the pinned forms' support rule on leading dimensions: no row the kernels address -- the padding rows of the last tile and the
    prefetch one grid stride ahead -- has a byte offset of 2^32 or more"""
    tiles = -(-M // TILE)
    return (tiles + min(tiles, NUM_CUS)) * TILE * max(lds) * 4 <= GIB4


def _sample_rows(M, ld, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    mid = (1 << 31) // (ld * 4)                                          # the row holding the 2 GiB byte mark
    parts = [torch.arange(0, 256), torch.arange(M - 256, M), torch.arange(mid - 128, mid + 128), torch.randint(0, M, (4096,), generator=g)]
    return torch.cat(parts).to(DEV)


def _need(nbytes):
    free = _free_bytes()
    if free < nbytes:
        pytest.skip('needs %.1f GiB of free device memory, %.1f free' % (nbytes / 2 ** 30, free / 2 ** 30))


EDGE_FWD = [
    # (ldx = K, ldy, M): the largest M the entry point's guard admits
    (304, 256, 3532045),          # padding-row reads of x wrap
    (304, 320, 3355443),          # padding-row stores of y wrap (and the reads of the prefetch)
    (256, 256, 4194303),          # control: no padding row wraps, only the prefetch one grid stride past the last tile
]


@pytest.mark.parametrize('case', EDGE_FWD, ids=lambda c: 'ldx%d_ldy%d_M%d' % c)
def test_pinned_forward_at_the_4gib_edge(ops, case):
    """dl3p_pwconv_fwd_sb just under its guard, with statistics and with a bias: the launch writes nothing but its rows, its rows
    0 .. 65535 are the bits of the same launch on the 65536-row prefix (each row's reduction runs in the same order whatever M is, on
    the form the rule picks for the whole launch), sampled rows match float64 and the statistic rows the float64 column sums"""
    K, ldy, M = case
    N = 256
    L = ops.lib()
    _need(2 * GIB4 + (2 << 30))
    assert M * max(K, ldy) * 4 < GIB4 <= (M + 1) * max(K, ldy) * 4          # the largest M the entry point admits
    with Opts(L, pw_small_min_rows=-1):
        assert _plan(L, 6, M, K, N)[3] == 4 and _plan(L, 5, M, K, N)[3] == 4          # (the rule, before the leading dimensions)
    g = _gen(M % 9973)
    xb = torch.empty(max(M, -(-(GIB4 + (1 << 20)) // (K * 4))), K, device=DEV)      # (reaches 4 GiB + 1 MiB from x)
    xb.normal_(generator=g)
    x = xb[:M]
    x[:TILE] *= 1000.0                                                                # a wrapped read of these rows cannot hide
    wt = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    wsp = ops.split_bf16x3(wt)
    sc, sh = torch.rand(K, device=DEV, generator=g) + 0.5, torch.randn(K, device=DEV, generator=g) * 0.3 + 0.1
    bias = torch.randn(N, device=DEV, generator=g)
    rows_s = _sample_rows(M, ldy, M)
    big = rows_s < TILE
    sb3 = int(_pinned_fits(M, (K, ldy)))
    out = Canary(M, N, lo=0, hi=ldy - N, min_bytes=GIB4 + (1 << 20))
    for mode in ('stats', 'bias'):
        b = bias if mode == 'bias' else None
        part = ops.new_partials(N, DEV) if mode == 'stats' else None
        if mode == 'bias':
            out.buf.view(torch.int32).copy_(out.pat.expand_as(out.buf))
        res = ops.pwconv_fwd_sb(x, wsp, K, b, sc, sh, ops.ACT_RELU, out=out.view, partials=part)
        torch.cuda.synchronize()
        out.intact(mode)
        y = out.view
        y64 = _act64(x[rows_s].double() * sc.double() + sh.double(), ops.ACT_RELU, ops) @ wt.double().t()
        if b is not None:
            y64 = y64 + b.double()
        err = (y[rows_s].double() - y64).abs().amax(1)
        for sel, what in ((big, 'the large rows 0 .. 127'), (~big, 'the other sampled rows')):
            bound = 2e-5 * float(y64[sel].abs().max())
            assert float(err[sel].max()) < bound, (mode, what, float(err[sel].max()), bound)
        if part is not None:
            s1 = torch.zeros(N, dtype=torch.float64, device=DEV)
            s2 = torch.zeros_like(s1)
            for r0 in range(0, M, CHUNK):
                yc = _act64(x[r0:r0 + CHUNK].double() * sc.double() + sh.double(), ops.ACT_RELU, ops) @ wt.double().t()
                s1 += yc.sum(0)
                s2 += (yc * yc).sum(0)
                del yc
            _check_stats(_stat_sums(part, res[1], N), s1, s2, M, mode)
        with Opts(L, sb3=sb3):
            yp = ops.pwconv_fwd_sb(x[:PREFIX], wsp, K, b, sc, sh, ops.ACT_RELU, partials=ops.new_partials(N, DEV) if part is not None else None)
        yp = yp[0] if part is not None else yp
        assert torch.equal(y[:PREFIX], yp), (mode, 'rows 0 .. 65535 differ from the prefix launch', float((y[:PREFIX] - yp).abs().max()))


def test_pinned_apply_at_the_4gib_edge(ops):
    """dl3p_pwconv_bwd_data_sb_apply with the pinned form selected (sb3 = 1), dz in a buffer 320 wide at the largest M the guard admits:
    its padding rows and the staging one grid stride past the last tile would wrap.  g, z_out, gx and z are 256 wide (no wrap)"""
    L = ops.lib()
    M, lddz = 3355443, 320
    assert M * lddz * 4 < GIB4 <= (M + 1) * lddz * 4
    _need(4 * M * 256 * 4 + GIB4 + (3 << 30))
    act = fact = ops.ACT_RELU
    g, z_out, bsc, bsh, mu, istd, coef, w, z, sc, sh, mean, invstd = _apply_case(ops, M, 41, act, fact)
    g[:TILE] *= 1000.0
    w_sp = ops.split_bf16x3(w)
    dzc = Canary(M, 256, lo=0, hi=lddz - 256, min_bytes=GIB4 + (1 << 20))
    gxc = Canary(M, 256, lo=0, hi=0)
    sb3 = 1 if _pinned_fits(M, (256, lddz)) else 0
    with Opts(L, sb3=1):
        part = ops.new_partials(256, DEV)
        _, _, rows = ops.pwconv_bwd_data_sb_apply(g, z_out, bsc, bsh, act, mu, istd, coef, w_sp, 256, dz=dzc.view, out=gxc.view,
                                                  z=z, scale=sc, shift=sh, act=fact, mean=mean, invstd=invstd, partials=part)
        torch.cuda.synchronize()
    dzc.intact('dz')
    gxc.intact('gx')
    rows_s = _sample_rows(M, lddz, 7)
    big = rows_s < TILE
    dz64, gx64 = _apply_ref(ops, rows_s, g, z_out, bsc, bsh, act, mu, istd, coef, w)
    for got, ref, tol, what in ((dzc.view[rows_s], dz64, 4e-6, 'dz'), (gxc.view[rows_s], gx64, 2e-5, 'gx')):
        err = (got.double() - ref).abs().amax(1)
        for sel, part_name in ((big, 'rows 0 .. 127'), (~big, 'other rows')):
            bound = tol * float(ref[sel].abs().max())
            assert float(err[sel].max()) < bound, (what, part_name, float(err[sel].max()), bound)
    s1 = torch.zeros(256, dtype=torch.float64, device=DEV)
    s2 = torch.zeros_like(s1)
    a1 = torch.zeros_like(s1)
    a2 = torch.zeros_like(s1)
    for r0 in range(0, M, CHUNK):
        r = slice(r0, r0 + CHUNK)
        _, gxr = _apply_ref(ops, r, g, z_out, bsc, bsh, act, mu, istd, coef, w)
        d = gxr * _dact64(z[r].double() * sc.double() + sh.double(), fact, ops)
        dx = d * (z[r].double() - mean.double()) * invstd.double()
        s1 += d.sum(0); s2 += dx.sum(0); a1 += d.abs().sum(0); a2 += dx.abs().sum(0)
        del gxr, d, dx
    p = _stat_sums(part, rows, 256)
    assert float((p[0] - s1).abs().max()) < 2e-4 * float(a1.max()), 'BN backward sum'
    assert float((p[1] - s2).abs().max()) < 2e-4 * float(a2.max()), 'BN backward sum * xhat'
    # rows 0 .. 131071 against the same launch on the prefix, on the form the rule picks for the whole launch (the row-stationary
    # kernel serves 131072 rows up)
    P = 2 * PREFIX
    with Opts(L, sb3=sb3):
        dzp, gxp = ops.pwconv_bwd_data_sb_apply(g[:P], z_out[:P], bsc, bsh, act, mu, istd, coef, w_sp, 256, dz=torch.empty(P, 256, device=DEV))
    assert torch.equal(dzc.view[:P], dzp), ('dz rows 0 .. %d differ from the prefix launch' % (P - 1))
    assert torch.equal(gxc.view[:P], gxp), ('gx rows 0 .. %d differ from the prefix launch' % (P - 1))


# --------------------------------------------------------------------------------------------------------- c. just over the guards
def _over(ops, fn, outs):
    """fn() must raise Dl3pError and leave every output buffer bitwise untouched"""
    before = [o.view(torch.int32)[:: max(1, o.shape[0] // 4096)].clone() for o in outs]
    heads = [o.view(torch.int32)[:TILE].clone() for o in outs]
    with pytest.raises(ops.Dl3pError, match='4 GiB'):
        fn()
    torch.cuda.synchronize()
    for o, b, h in zip(outs, before, heads):
        assert torch.equal(o.view(torch.int32)[:: max(1, o.shape[0] // 4096)], b) and torch.equal(o.view(torch.int32)[:TILE], h)


@pytest.mark.parametrize('entry', ['pwconv_fwd', 'pwconv_fwd_sb', 'pwconv_bwd_data', 'pwconv_bwd_data_sb', 'sb_apply'])
def test_one_row_over_the_guard_is_refused(ops, entry):
    """M = the smallest row count whose operands reach 4 GiB (256 wide): the entry point refuses it before any launch and the
    output keeps its canary bits.  Every operand is allocated at full length, so even a launch that got through would stay inside
    memory the test owns"""
    K = N = ld = 256
    M = GIB4 // (ld * 4)                        # M * ld * 4 == 2^32
    _need(2 * GIB4 + (1 << 30))
    big = torch.empty(M, ld, device=DEV)
    big.view(torch.int32).copy_(_pattern(ld).expand(M, ld))
    src = torch.zeros(M, ld, device=DEV)
    w = torch.zeros(K, N, device=DEV)
    if entry == 'pwconv_fwd':
        _over(ops, lambda: ops.pwconv_fwd(src, w, out=big), [big])
    elif entry == 'pwconv_fwd_sb':
        _over(ops, lambda: ops.pwconv_fwd_sb(src, ops.split_bf16x3(w), K, out=big), [big])
    elif entry == 'pwconv_bwd_data':
        _over(ops, lambda: ops.pwconv_bwd_data(src, w, out=big), [big])
    elif entry == 'pwconv_bwd_data_sb':
        _over(ops, lambda: ops.pwconv_bwd_data_sb(src, ops.split_bf16x3(w), N, out=big), [big])
    else:
        v = torch.ones(256, device=DEV)
        coef = torch.ones(3, 256, device=DEV)
        _over(ops, lambda: ops.pwconv_bwd_data_sb_apply(src, src, v, v, ops.ACT_RELU, v, v, coef, ops.split_bf16x3(w), N,
                                                        dz=big, out=big), [big])
