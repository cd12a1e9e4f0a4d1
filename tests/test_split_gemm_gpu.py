"""The fp32-accurate GEMMs on the bf16 matrix pipe (csrc/pw_split.hip) at the UNCHANGED tolerances of the
fp32 kernels: forward 2e-5 of the output's scale (tests/test_production_shapes_gpu.py PW_PROD), statistics 1e-4, data
gradient 2e-5, BatchNorm-backward sums 2e-4 -- against float64.  Plus the split itself: exact (a1 + a2 + a3 == a bit for bit),
and the comparison the opt-in is judged by: its error against float64 next to the fp32 MFMA kernel's on the same inputs."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _bf16_planes_to_f32(sp):
    """(3, rows, pitch) int16 -> three float32 arrays"""
    u = sp.cpu().numpy().view(np.uint16).astype(np.uint32) << 16
    return u.view(np.float32)


def test_split_is_exact(ops):
    g = torch.Generator(device=DEV); g.manual_seed(3)
    a = torch.randn(37, 70, device=DEV, generator=g) * torch.exp(torch.randn(37, 70, device=DEV, generator=g) * 4)
    a[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e-39, 6.0, 1e30, -7.5e-20], device=DEV)      # zero, a denormal, large / tiny
    sp = ops.split_bf16x3(a)
    assert sp.shape == (3, 37, 96)
    h, m, l = _bf16_planes_to_f32(sp)
    an = a.cpu().numpy()
    s = (h[:, :70].astype(np.float64) + m[:, :70].astype(np.float64)) + l[:, :70].astype(np.float64)
    # exact: the three pieces carry the 24 significant bits of a float32 (denormals lose what bf16 cannot hold: flushed)
    normal = np.abs(an) > 1e-30
    assert np.array_equal(s[normal], an.astype(np.float64)[normal])
    assert np.all(h[:, 70:] == 0) and np.all(m[:, 70:] == 0) and np.all(l[:, 70:] == 0)
    # magnitudes fall by 2^-8 per level (round to nearest)
    assert np.all(np.abs(m[:, :70][normal]) <= np.abs(h[:, :70][normal]) * 2.0 ** -8 * 1.0001)
    assert np.all(np.abs(l[:, :70][normal]) <= np.abs(h[:, :70][normal]) * 2.0 ** -16 * 1.0001)


SHAPES = [(16 * 129 * 129, 304, 256), (16 * 129 * 129, 256, 256), (16 * 33 * 33, 1280, 256), (16 * 33 * 33, 960, 160),
          (16 * 33 * 33, 160, 960), (4 * 33 * 33, 728, 728), (4 * 33 * 33, 2048, 256), (4 * 33 * 33, 1536, 2048),
          (16 * 65 * 65, 192, 64), (16 * 129 * 129, 256, 24),
          # ragged: M not a multiple of the tile, K not of 32, N not of 16
          (4357, 100, 200), (1089, 36, 24), (9001, 304, 252), (2600, 728, 132), (130, 20, 12)]


@pytest.mark.parametrize('pipe', [1, 0], ids=['producer_consumer', 'symmetric'])
@pytest.mark.parametrize('case', SHAPES)
def test_split_gemm_matches_float64_at_the_fp32_tolerances(ops, case, pipe):
    M, K, N = case
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', -1)
    L.set_option(b'sb_pipe', pipe)
    try:
        g = torch.Generator(device=DEV); g.manual_seed(M % 9973 + 7 * K + 13 * N)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        x = rnd(M, K)
        wt = rnd(N, K) / K ** 0.5
        sc = torch.rand(K, device=DEV, generator=g) + 0.5
        sh = rnd(K) * 0.3
        bias = rnd(N) * 0.1
        a64 = (x.double() * sc.double() + sh.double()).clamp(0.0, 6.0)
        y64 = a64 @ wt.double().t()
        wsp = ops.split_bf16x3(wt)
        part = ops.new_partials(N, DEV)
        y, rows = ops.pwconv_fwd_sb(x, wsp, K, None, sc, sh, ops.ACT_RELU6, partials=part)
        scale = float(y64.abs().max())
        e_sb = float((y.double() - y64).abs().max()) / scale
        assert e_sb < 2e-5, ('forward', e_sb)
        p = part[:rows * 2 * N].reshape(rows, 2, N).double().sum(0)
        s1, s2 = y64.sum(0), (y64 * y64).sum(0)
        assert float((p[0] - s1).abs().max()) < 1e-4 * max(float(s1.abs().max()), float(M) ** 0.5), 'stat sum'
        assert float((p[1] - s2).abs().max()) < 1e-4 * float(s2.abs().max()), 'stat sum of squares'
        # the fp32 MFMA kernel on the same inputs: the split kernel's error is of the same size (recorded, bounded at 3x)
        y32 = ops.pwconv_fwd_wt(x, wt, None, sc, sh, ops.ACT_RELU6)
        e_32 = float((y32.double() - y64).abs().max()) / scale
        assert e_sb < 3 * e_32 + 1e-7, (e_sb, e_32)
        # bias, no statistics, no prologue
        y2 = ops.pwconv_fwd_sb(x, wsp, K, bias)
        assert float((y2.double() - (x.double() @ wt.double().t() + bias.double())).abs().max()) < 2e-5 * float((x.double() @ wt.double().t()).abs().max())
        del y, y2, y32, a64, y64
        # data gradient: dy (M, N) . w (K, N)^T
        dy = rnd(M, N)
        w = wt.t().contiguous()          # (K, N)
        w_sp = ops.split_bf16x3(w)
        gx64 = dy.double() @ w.double().t()
        gx = ops.pwconv_bwd_data_sb(dy, w_sp, N)
        assert float((gx.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max()), 'data gradient'
        base = rnd(M, K)
        gx_acc = ops.pwconv_bwd_data_sb(dy, w_sp, N, out=base.clone(), accumulate=True)
        assert float((gx_acc.double() - (gx64 + base.double())).abs().max()) < 2e-5 * float(gx64.abs().max()), 'accumulate'
        z = rnd(M, K)
        mean = z.mean(0)
        invstd = 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
        part = ops.new_partials(K, DEV)
        gx2, rows = ops.pwconv_bwd_data_sb(dy, w_sp, N, z=z, scale=sc, shift=sh, act=ops.ACT_RELU6, mean=mean, invstd=invstd,
                                           partials=part)
        assert float((gx2.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max()), 'data gradient (+BN sums)'
        u = z.double() * sc.double() + sh.double()
        d = gx64 * ((u > 0) & (u < 6))
        xh = (z.double() - mean.double()) * invstd.double()
        p = part[:rows * 2 * K].reshape(rows, 2, K).double().sum(0)
        assert float((p[0] - d.sum(0)).abs().max()) < 2e-4 * float(d.abs().sum(0).max()), 'BN backward sum'
        assert float((p[1] - (d * xh).sum(0)).abs().max()) < 2e-4 * float((d * xh).abs().sum(0).max()), 'BN backward sum * xhat'
    finally:
        L.set_option(b'pw_small_min_rows', 64)
        L.set_option(b'sb_pipe', 0)


@pytest.mark.parametrize('pipe', [1, 0], ids=['producer_consumer', 'symmetric'])
@pytest.mark.parametrize('mi', [1, 2])
@pytest.mark.parametrize('nt', [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_split_gemm_tile_choice(ops, nt, mi, pipe):
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', 1 << 30)
    L.set_option(b'gemm_nt', nt)
    L.set_option(b'gemm_mi', mi)
    L.set_option(b'sb_pipe', pipe)
    try:
        for case in [(4357, 100, 200), (2600, 728, 132)]:
            _run(ops, case)
    finally:
        L.set_option(b'gemm_nt', 0)
        L.set_option(b'gemm_mi', 0)
        L.set_option(b'sb_pipe', 0)
        L.set_option(b'pw_small_min_rows', 64)


def _run(ops, case):
    L = ops.lib()
    M, K, N = case
    g = torch.Generator(device=DEV); g.manual_seed(M + K + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    wt = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    part = ops.new_partials(N, DEV)
    y, rows = ops.pwconv_fwd_sb(x, ops.split_bf16x3(wt), K, partials=part)
    y64 = x.double() @ wt.double().t()
    assert float((y.double() - y64).abs().max()) < 2e-5 * float(y64.abs().max())
    p = part[:rows * 2 * N].reshape(rows, 2, N).double().sum(0)
    assert float((p[1] - (y64 * y64).sum(0)).abs().max()) < 1e-4 * float((y64 * y64).sum(0).max())
    dy = torch.randn(M, N, device=DEV, generator=g)
    w = wt.t().contiguous()
    z = torch.randn(M, K, device=DEV, generator=g)
    one, zero = torch.ones(K, device=DEV), torch.zeros(K, device=DEV)
    part = ops.new_partials(K, DEV)
    gx, rows = ops.pwconv_bwd_data_sb(dy, ops.split_bf16x3(w), N, z=z, scale=one, shift=zero, act=ops.ACT_RELU, mean=zero, invstd=one,
                                      partials=part)
    gx64 = dy.double() @ w.double().t()
    assert float((gx.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max())
    d = gx64 * (z.double() > 0)
    p = part[:rows * 2 * K].reshape(rows, 2, K).double().sum(0)
    assert float((p[0] - d.sum(0)).abs().max()) < 2e-4 * float(d.abs().sum(0).max())


@pytest.mark.parametrize('nt,mi,wm', [(16, 2, 1), (16, 1, 1), (16, 1, 2), (12, 2, 1), (12, 2, 2), (8, 2, 2)])
def test_every_wide_split_gemm_tile(ops, nt, mi, wm):
    """the one-workgroup-per-CU family (128 / 256 rows x up to 256 columns, 256 or 512 threads)"""
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', 1 << 30)
    L.set_option(b'sb_wm', wm)
    L.set_option(b'sb_nt', nt)
    L.set_option(b'gemm_mi', mi)
    try:
        for case in [(4357, 100, 200), (2600, 728, 252), (70001, 304, 256), (1301, 260, 132)]:
            _run(ops, case)
    finally:
        L.set_option(b'sb_wm', 0)
        L.set_option(b'sb_nt', 0)
        L.set_option(b'gemm_mi', 0)
        L.set_option(b'pw_small_min_rows', 64)


# ---------------------------------------------------------------------------------------------------------------------------
# round 4: operands that are NOT randn: wide per-channel dynamic range, saturated activations, tiny gradients,
# with an ELEMENTWISE bound -- |y - y64| against sum_k |a_mk| |w_nk| of that very element -- instead of one max-abs over the output
def _elementwise_err(y, y64, a64, w64):
    """max over elements of |y - y64| / (|a| @ |w|^T): the condition-aware error of an fp32 inner product (K eps / 2 worst case,
    ~sqrt(K) eps typical); columns or rows 2^20 below the largest count like every other"""
    cond = a64.abs() @ w64.abs().t()
    cond = cond.clamp_min(float(torch.finfo(torch.float64).tiny))
    return float(((y.double() - y64).abs() / cond).max())


WIDE = [(16 * 33 * 33, 320, 256), (9001, 304, 252), (70001, 256, 304)]


@pytest.mark.parametrize('rs', [0, 1], ids=['tiled', 'row_stationary'])
@pytest.mark.parametrize('case', WIDE)
def test_split_gemm_wide_dynamic_range(ops, case, rs):
    """per-column scales spanning 2^+-20 on either operand, a saturated-ReLU6 column block, an all-zero block; the split kernel
    stays within 3x the fp32-input MFMA kernel's own elementwise error and under the fp32 inner-product bound"""
    M, K, N = case
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', -1)
    L.set_option(b'sb_rs', rs)
    try:
        g = torch.Generator(device=DEV); g.manual_seed(11 * M + K + N)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        kscale = torch.exp2(torch.randint(-20, 21, (K,), device=DEV, generator=g).float())     # activation channels over 2^40
        nscale = torch.exp2(torch.randint(-20, 21, (N,), device=DEV, generator=g).float())     # output channels over 2^40
        x = rnd(M, K) * kscale
        wt = rnd(N, K) / K ** 0.5 * nscale[:, None]
        wsp = ops.split_bf16x3(wt)
        # (1) no prologue: the raw dynamic range reaches the split
        y64 = x.double() @ wt.double().t()
        y = ops.pwconv_fwd_sb(x, wsp, K)
        y32 = ops.pwconv_fwd_wt(x, wt)
        e_sb, e_32 = _elementwise_err(y, y64, x.double(), wt.double()), _elementwise_err(y32, y64, x.double(), wt.double())
        assert e_sb < 1e-5 and e_sb < 3 * e_32 + 1e-7, ('forward, raw', e_sb, e_32)
        # every COLUMN on its own scale (what max-abs over the whole output cannot see)
        col = (y.double() - y64).abs().max(0).values / y64.abs().max(0).values
        assert float(col.max()) < 2e-5, ('forward, per column', float(col.max()))
        # (2) BatchNorm + ReLU6 prologue with a saturated block (u >> 6 -> exactly 6), a dead block (u << 0 -> exactly 0) and
        # the rest spanning decades below the clamp
        sc = torch.exp2(torch.randint(-12, 3, (K,), device=DEV, generator=g).float())
        sh = rnd(K) * 0.1
        sh[: K // 8] = 100.0          # saturated at 6
        sh[K // 8: K // 4] = -100.0   # dead
        xs = rnd(M, K)
        a64 = (xs.double() * sc.double() + sh.double()).clamp(0.0, 6.0)
        assert bool((a64[:, : K // 8] == 6.0).all()) and bool((a64[:, K // 8: K // 4] == 0.0).all())
        y64 = a64 @ wt.double().t()
        part = ops.new_partials(N, DEV)
        y, rows = ops.pwconv_fwd_sb(xs, wsp, K, None, sc, sh, ops.ACT_RELU6, partials=part)
        y32 = ops.pwconv_fwd_wt(xs, wt, None, sc, sh, ops.ACT_RELU6)
        e_sb, e_32 = _elementwise_err(y, y64, a64, wt.double()), _elementwise_err(y32, y64, a64, wt.double())
        assert e_sb < 1e-5 and e_sb < 3 * e_32 + 1e-7, ('forward, saturated prologue', e_sb, e_32)
        p = part[:rows * 2 * N].reshape(rows, 2, N).double().sum(0)
        s1, s2 = y64.sum(0), (y64 * y64).sum(0)
        assert float(((p[0] - s1).abs() / y64.abs().sum(0)).max()) < 1e-5, 'statistics, per column'
        assert float(((p[1] - s2).abs() / s2).max()) < 1e-5, 'statistics of squares, per column'
        del y, y32, y64, a64
        # (3) data gradient of a late-training step: dy at 1e-12 with per-channel scales on top
        dy = rnd(M, N) * 1e-12 * nscale
        w = (rnd(K, N) / N ** 0.5).contiguous()
        w_sp = ops.split_bf16x3(w)
        gx64 = dy.double() @ w.double().t()
        gx = ops.pwconv_bwd_data_sb(dy, w_sp, N)
        gx32 = ops.pwconv_bwd_data(dy, w)
        e_sb, e_32 = _elementwise_err(gx, gx64, dy.double(), w.double()), _elementwise_err(gx32, gx64, dy.double(), w.double())
        assert e_sb < 1e-5 and e_sb < 3 * e_32 + 1e-7, ('data gradient at 1e-12', e_sb, e_32)
        assert float(gx.abs().max()) > 0.0
    finally:
        L.set_option(b'pw_small_min_rows', 64)
        L.set_option(b'sb_rs', -1)


def test_split_gemm_domain_edges(ops):
    """What the 3-way split does at the ends of the float32 range, stated at GEMM level (include/dl3p.h):
    * |a| below 2^-110: the third (then the second) piece of a falls under bf16's smallest normal 2^-126; whatever the matrix pipe
      does with such pieces, the product loses at most 2^-126 |w| per term -- an ABSOLUTE error far below any float32-normal
      output scale -- and nothing else;
    * an element that is Inf, NaN, or rounds to bf16 Inf (|a| >= 3.3962e38, half a bf16 step past the largest finite bf16 3.3895e38): the residual a - rn_bf16(a) is NaN, so every output of
      that ROW is non-finite (the fp32-input kernel gives Inf / NaN for Inf / NaN and a finite value for the huge finite one);
      other rows are untouched."""
    M, K, N = 4357, 304, 256
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', -1)
    try:
        g = torch.Generator(device=DEV); g.manual_seed(5)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        wt = rnd(N, K) / K ** 0.5
        wsp = ops.split_bf16x3(wt)
        for lo, hi in ((-112, -106), (-120, -112), (-126, -119)):
            x = rnd(M, K).sign() * torch.exp2(torch.empty(M, K, device=DEV).uniform_(lo, hi, generator=g))
            y64 = x.double() @ wt.double().t()
            y = ops.pwconv_fwd_sb(x, wsp, K)
            bound = 2.0 ** -126 * wt.double().abs().sum(1)[None, :] + 1e-5 * (x.double().abs() @ wt.double().abs().t())
            assert bool(((y.double() - y64).abs() <= bound).all()), ('tiny operands', lo, hi, float(((y.double() - y64).abs() / bound).max()))
        x = rnd(M, K)
        x[7, 3] = float('inf'); x[19, 100] = float('nan'); x[33, 300] = 3.4e38; x[40, 1] = -3.4e38
        y = ops.pwconv_fwd_sb(x, wsp, K)
        y32 = ops.pwconv_fwd_wt(x, wt)
        bad = torch.zeros(M, dtype=torch.bool, device=DEV); bad[[7, 19, 33, 40]] = True
        assert bool((~torch.isfinite(y[bad])).all()), 'a row holding Inf / NaN / |a| > bf16 max must not produce finite values'
        assert bool((~torch.isfinite(y32[[7, 19]])).all()) and bool(torch.isfinite(y32[[33, 40]]).all())       # the fp32 kernel, for the record
        xg = x[~bad]
        y64 = xg.double() @ wt.double().t()
        assert bool(torch.isfinite(y[~bad]).all())
        assert float((y[~bad].double() - y64).abs().max()) < 2e-5 * float(y64.abs().max())
    finally:
        L.set_option(b'pw_small_min_rows', 64)


RS_SHAPES = [(70001, 304, 256), (66564, 256, 256), (9001, 256, 304), (4357, 128, 48), (33289, 192, 48), (2600, 100, 200), (2111, 320, 16)]


@pytest.mark.parametrize('case', RS_SHAPES)
def test_row_stationary_split_gemm(ops, case):
    """csrc/pw_split_rs.hip (dl3p_set_option('sb_rs', 1)): forward + statistics, bias, data gradient (+ accumulate, + fused
    BatchNorm-backward sums) against float64 at the fp32 kernels' tolerances; the planner reports the row-stationary form"""
    import ctypes
    M, K, N = case
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', -1)
    L.set_option(b'sb_rs', 1)
    try:
        out6 = (ctypes.c_int * 6)()
        L.gemm_plan_query(6, M, K, N, out6)
        assert out6[0] == 3 and out6[3] == 3, list(out6)       # role 1 (forward + statistics) on the split path, wm = 3: row-stationary
        g = torch.Generator(device=DEV); g.manual_seed(M % 9973 + 7 * K + 13 * N)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        x = rnd(M, K)
        wt = rnd(N, K) / K ** 0.5
        sc = torch.rand(K, device=DEV, generator=g) + 0.5
        sh = rnd(K) * 0.3
        bias = rnd(N) * 0.1
        a64 = (x.double() * sc.double() + sh.double()).clamp(0.0, 6.0)
        y64 = a64 @ wt.double().t()
        wsp = ops.split_bf16x3(wt)
        part = ops.new_partials(N, DEV)
        y = torch.full((M, N), float('nan'), device=DEV)
        _, rows = ops.pwconv_fwd_sb(x, wsp, K, None, sc, sh, ops.ACT_RELU6, out=y, partials=part)
        assert float((y.double() - y64).abs().max()) < 2e-5 * float(y64.abs().max()), 'forward'
        p = part[:rows * 2 * N].reshape(rows, 2, N).double().sum(0)
        s1, s2 = y64.sum(0), (y64 * y64).sum(0)
        assert float((p[0] - s1).abs().max()) < 1e-4 * max(float(s1.abs().max()), float(M) ** 0.5), 'stat sum'
        assert float((p[1] - s2).abs().max()) < 1e-4 * float(s2.abs().max()), 'stat sum of squares'
        # bit-identical between two launches (fixed summation order everywhere)
        part2 = ops.new_partials(N, DEV)
        y_again, rows2 = ops.pwconv_fwd_sb(x, wsp, K, None, sc, sh, ops.ACT_RELU6, partials=part2)
        assert rows2 == rows and torch.equal(y_again, y) and torch.equal(part2[:rows * 2 * N], part[:rows * 2 * N])
        y2 = ops.pwconv_fwd_sb(x, wsp, K, bias, None, None, ops.ACT_RELU)
        r64 = x.double().clamp_min(0) @ wt.double().t() + bias.double()
        assert float((y2.double() - r64).abs().max()) < 2e-5 * float(r64.abs().max()), 'bias + bare ReLU prologue'
        del y, y2, a64, y64, r64
        dy = rnd(M, N)
        w = wt.t().contiguous()          # (K, N)
        w_sp = ops.split_bf16x3(w)
        L.gemm_plan_query(8, M, N, K, out6)       # the data gradient reduces over N: row-stationary for N in 97..128, 161..192, 225..256, 289..320
        served = out6[0] == 3 and out6[3] == 3
        gx64 = dy.double() @ w.double().t()
        gx = ops.pwconv_bwd_data_sb(dy, w_sp, N)
        assert float((gx.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max()), ('data gradient', served)
        base = rnd(M, K)
        gx_acc = ops.pwconv_bwd_data_sb(dy, w_sp, N, out=base.clone(), accumulate=True)
        assert float((gx_acc.double() - (gx64 + base.double())).abs().max()) < 2e-5 * float(gx64.abs().max()), 'accumulate'
        z = rnd(M, K)
        mean = z.mean(0)
        invstd = 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
        part = ops.new_partials(K, DEV)
        gx2, rows = ops.pwconv_bwd_data_sb(dy, w_sp, N, z=z, scale=sc, shift=sh, act=ops.ACT_RELU6, mean=mean, invstd=invstd,
                                           partials=part)
        assert float((gx2.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max()), 'data gradient (+BN sums)'
        u = z.double() * sc.double() + sh.double()
        d = gx64 * ((u > 0) & (u < 6))
        xh = (z.double() - mean.double()) * invstd.double()
        p = part[:rows * 2 * K].reshape(rows, 2, K).double().sum(0)
        assert float((p[0] - d.sum(0)).abs().max()) < 2e-4 * float(d.abs().sum(0).max()), 'BN backward sum'
        assert float((p[1] - (d * xh).sum(0)).abs().max()) < 2e-4 * float((d * xh).abs().sum(0).max()), 'BN backward sum * xhat'
    finally:
        L.set_option(b'pw_small_min_rows', 64)
        L.set_option(b'sb_rs', -1)


@pytest.mark.parametrize('case', [(131072 + 77, 304, 256), (140000, 256, 256), (133000, 48, 232)])
@pytest.mark.parametrize('act_name', ['relu6', 'relu', 'none'])
def test_data_gradient_with_the_folded_batchnorm_apply(ops, case, act_name):
    """dl3p_pwconv_bwd_data_sb_apply (csrc/pw_split_rs.hip, FOLD): dz = c0 (g act'(z s + t) - c1 - xhat c2) formed while the row
    tile is staged, written once (over g when no other destination is given), multiplied -> gx, with and without the fused
    BatchNorm-backward sums of the layer in front; all of it against float64"""
    M, K, N = case          # K output columns, N the reduction (= channels of the folded BatchNorm)
    act = {'relu6': ops.ACT_RELU6, 'relu': ops.ACT_RELU, 'none': ops.ACT_NONE}[act_name]
    L = ops.lib()
    assert L.pwconv_bwd_data_sb_apply_supported(M, K, N, act, 1) == 1
    assert L.pwconv_bwd_data_sb_apply_supported(M, K, N, ops.ACT_HSWISH, 1) == 0 and L.pwconv_bwd_data_sb_apply_supported(4096, K, N, act, 1) == 0
    g_ = torch.Generator(device=DEV); g_.manual_seed(M + K + N)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g_)
    g = rnd(M, N)
    z_out = rnd(M, N) * 1.5 + 0.3
    bsc, bsh = torch.rand(N, device=DEV, generator=g_) + 0.5, rnd(N) * 0.5 + (1.0 if act == ops.ACT_RELU6 else 0.0)
    mu, istd = rnd(N) * 0.2, torch.rand(N, device=DEV, generator=g_) + 0.5
    coef = torch.stack([torch.rand(N, device=DEV, generator=g_) + 0.5, rnd(N) * 0.1, rnd(N) * 0.1]).contiguous()
    w = (rnd(K, N) / N ** 0.5).contiguous()
    w_sp = ops.split_bf16x3(w)
    u = z_out.double() * bsc.double() + bsh.double()
    if act == ops.ACT_RELU6:
        m = ((u > 0) & (u < 6)).double()
    elif act == ops.ACT_RELU:
        m = (u > 0).double()
    else:
        m = torch.ones_like(u)
    dz64 = coef[0].double() * (g.double() * m - coef[1].double() - (z_out.double() - mu.double()) * istd.double() * coef[2].double())
    gx64 = dz64 @ w.double().t()
    # plain, dz to its own buffer
    dz = torch.full((M, N), float('nan'), device=DEV)
    gx = torch.full((M, K), float('nan'), device=DEV)
    ops.pwconv_bwd_data_sb_apply(g, z_out, bsc, bsh, act, mu, istd, coef, w_sp, N, dz=dz, out=gx)
    assert float((dz.double() - dz64).abs().max()) < 4e-6 * float(dz64.abs().max()), 'dz'
    assert float((gx.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max()), 'gx'
    # with the fused BatchNorm-backward sums of the layer in front, dz IN PLACE of g, accumulate into gx
    z = rnd(M, K)
    sc, sh = torch.rand(K, device=DEV, generator=g_) + 0.5, rnd(K) * 0.3
    mean, invstd = z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
    part = ops.new_partials(K, DEV)
    base = rnd(M, K)
    g2 = g.clone()
    dz2, gx2, rows = ops.pwconv_bwd_data_sb_apply(g2, z_out, bsc, bsh, act, mu, istd, coef, w_sp, N, out=base.clone(), accumulate=True,
                                                  z=z, scale=sc, shift=sh, act=ops.ACT_RELU6, mean=mean, invstd=invstd, partials=part)
    assert dz2.data_ptr() == g2.data_ptr() and torch.equal(dz2, dz), 'in place == separate buffer, bit for bit'
    tot64 = gx64 + base.double()
    assert float((gx2.double() - tot64).abs().max()) < 2e-5 * float(gx64.abs().max()), 'gx (accumulate)'
    uu = z.double() * sc.double() + sh.double()
    d = tot64 * ((uu > 0) & (uu < 6))
    xh = (z.double() - mean.double()) * invstd.double()
    p = part[:rows * 2 * K].reshape(rows, 2, K).double().sum(0)
    assert float((p[0] - d.sum(0)).abs().max()) < 2e-4 * float(d.abs().sum(0).max()), 'BN backward sum'
    assert float((p[1] - (d * xh).sum(0)).abs().max()) < 2e-4 * float((d * xh).abs().sum(0).max()), 'BN backward sum * xhat'


# ---------------------------------------------------------------------------------------------- the accumulate's one-sided bias
# v_mfma_f32_16x16x32_bf16 cuts addends far below the running sum off toward -inf (scripts/micro/mfma_round.hip), so the
# default one-level accumulate of the split GEMMs carries a COLUMN-MEAN bias the per-element bounds above cannot see: measured
# 1.2 .. 1.3e-10 * K of the column's sigma (3.4e-8 at K = 288, 5.8e-7 at K = 4608), linear in the reduction length.  This test pins
# that law with a factor-two margin: a kernel change that doubles the bias fails here.
@pytest.mark.parametrize('K', [256, 304, 728, 1536, 2048, 4608])
def test_split_gemm_column_mean_bias_follows_its_documented_law(ops, K):
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', 1 << 30)
    try:
        M, N = 16 * 33 * 33, 256
        g = torch.Generator(device=DEV); g.manual_seed(K)
        x = torch.randn(M, K, device=DEV, generator=g)
        w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
        sc, sh = torch.rand(K, device=DEV, generator=g) + 0.5, torch.randn(K, device=DEV, generator=g) * 0.3
        a64 = (x.double() * sc.double() + sh.double()).clamp(min=0)
        y64 = a64 @ w.double()
        sig = y64.std(0)
        wt = w.t().contiguous()
        y = ops.pwconv_fwd_sb(x, ops.split_bf16x3(wt), K, None, sc, sh, ops.ACT_RELU)
        e = y.double() - y64
        bias = float((e.mean(0).abs() / sig).max())
        rms = float((e ** 2).mean().sqrt() / (y64 ** 2).mean().sqrt())
        noise = rms / M ** 0.5 * 4                      # what the mean of M unbiased errors of that rms could reach
        assert bias < 2.6e-10 * K + 2e-8 + noise, ('forward', K, bias, rms)
        assert rms < 2.2e-8 * K ** 0.5, rms             # (the unbiased part grows like a random walk over the reduction)
        # data gradient: the reduction runs over the conv's OUTPUT channels (here K of them), result (M, N2)
        N2 = 256
        dy = torch.randn(M, K, device=DEV, generator=g)
        w2 = torch.randn(N2, K, device=DEV, generator=g) / K ** 0.5        # conv kernel (cin = N2, cout = K)
        g64 = dy.double() @ w2.double().t()
        gx = ops.pwconv_bwd_data_sb(dy, ops.split_bf16x3(w2), K)
        e = gx.double() - g64
        bias = float((e.mean(0).abs() / g64.std(0)).max())
        rms = float((e ** 2).mean().sqrt() / (g64 ** 2).mean().sqrt())
        assert bias < 2.6e-10 * K + 2e-8 + rms / M ** 0.5 * 4, ('data gradient', K, bias, rms)
        del x, a64, y64, y, e, dy, g64, gx
        torch.cuda.empty_cache()
    finally:
        L.set_option(b'pw_small_min_rows', 64)


def test_thirty_steps_on_the_split_gemms_stay_with_the_fp32_kernels(monkeypatch):
    """what the bias does to TRAINING: 30 SGD steps of MobileNetV2-DeepLabV3+ at 65 x 65 with every GEMM the tiled kernel serves on the
    split path against the same 30 steps on the fp32-input MFMA kernels -- same weights, batches and dropout stream.  Losses and the
    weight drift are recorded (gpurun_out/split_trajectory.json) and bounded: the two trajectories differ like two orders of
    summation do, not like a biased and an unbiased estimator."""
    import json
    import os
    pkg = load_pkg()
    N, C, H, W = 4, 21, 65, 65
    rng = np.random.default_rng(23)
    xs = [rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32) for _ in range(6)]
    ys = []
    for _ in range(6):
        y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
        y[rng.uniform(size=y.shape) < 0.05] = 255
        ys.append(y)

    def run(split, nudge=1.0):
        monkeypatch.setenv('DL3P_SPLIT_GEMM', '1' if split else '0')
        for k, v in (('DL3P_SPLIT_MIN_K', '32'), ('DL3P_SPLIT_MIN_N', '16'), ('DL3P_SPLIT_MIN_ROWS', '64'), ('DL3P_SPLIT_MIN_ROWS_BN', '64')):
            monkeypatch.setenv(k, v)
        torch.manual_seed(0)
        m = pkg.get_deeplabv3p_model('mobilenetv2', C, (H, W), 16, training=True)
        m.compile(optimizer=pkg.SGD(0.01, momentum=0.9), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        m.use_graphs = False
        start = {k: np.array(v, dtype=np.float64) for k, v in m.get_weights_by_name().items()}
        losses = [m.train_on_batch(xs[i % 6] * np.float32(nudge), ys[i % 6]) for i in range(30)]
        ex = m._executor(N, True)
        took = any('pwconv_fwd_sb' in lab[0] for lab in ex.fwd.labels)
        return losses, m.get_weights_by_name(), took, start

    l1, w1, took1, _ = run(True)
    l0, w0, took0, start = run(False)
    # the control: the fp32-input kernels again on images scaled by 1 + 2.4e-7 (every pixel moves by one or two float32 ulps): what a
    # rounding-sized perturbation alone does to 30 steps
    lc, wc, _, _ = run(False, nudge=1.0 + 2.4e-7)
    assert took1 and not took0
    keys = [k for k in w0 if not k.endswith(('moving_mean', 'moving_variance'))]
    num = sum(float(((w1[k].astype(np.float64) - w0[k]) ** 2).sum()) for k in keys)
    den = sum(float((w0[k].astype(np.float64) ** 2).sum()) for k in keys)
    drift = (num / den) ** 0.5                          # relative l2 distance of the two weight vectors after 30 steps
    moved = (sum(float(((w0[k].astype(np.float64) - start[k]) ** 2).sum()) for k in keys) / den) ** 0.5      # ... of the fp32 run from its start
    control = (sum(float(((wc[k].astype(np.float64) - w0[k]) ** 2).sum()) for k in keys) / den) ** 0.5     # ... of two fp32 runs from each other
    dlc = max(abs(a - b) / abs(b) for a, b in zip(lc, l0))
    dl = max(abs(a - b) / abs(b) for a, b in zip(l1, l0))
    try:
        d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
        os.makedirs(d, exist_ok=True)
        json.dump({'loss_split': l1, 'loss_fp32': l0, 'relative_l2_weight_drift': drift, 'relative_l2_moved_from_start': moved, 'relative_l2_control_drift': control, 'control_loss_difference': dlc, 'worst_relative_loss_difference': dl},
                  open(os.path.join(d, 'split_trajectory.json'), 'w'))
    except OSError:
        pass
    # Two fp32 trajectories that differ in rounding only part ways too: a ReLU6 branch flipped in step 3 is an O(1) change of one
    # activation, and 30 steps of momentum SGD carry it on (the un-injected gradient comparisons of tests/test_product_vs_*_gpu.py
    # sit at 1e-2 for ONE step).  What a biased estimator would add is a DRIFT of the loss curve in one direction; what is measured is
    # a difference that changes sign from step to step (gpurun_out/split_trajectory.json) and a weight distance far below the
    # distance either run has moved from its start.
    assert l1[-1] < l1[0] - 0.05 and l0[-1] < l0[0] - 0.05           # both learn
    assert dl < 2e-2, dl
    signs = [np.sign(a - b) for a, b in zip(l1[5:], l0[5:])]
    assert 0.2 < np.mean(np.array(signs) > 0) < 0.8, signs          # no one-sided offset of the loss curve
    assert abs(float(np.mean(np.array(l1[5:]) - np.array(l0[5:])))) < 5e-3
    assert drift < 2.0 * control + 1e-3, (drift, control, moved)


# ------------------------------------------------------------------------------------------- the pinned-schedule forward (csrc/pw_split3.hip)
def _plan(L, role, M, K, N):
    import ctypes
    out = (ctypes.c_int * 6)()
    L.gemm_plan_query(role, M, K, N, out)
    return list(out)


SB3_CASES = [
    # (M, K, N, act, prologue, statistics, bias, input pitch, output pitch)
    (16 * 129 * 129, 304, 256, 'relu', True, True, False, 304, 256),       # decoder_conv0_pointwise at BASELINE configs[1]
    (16 * 129 * 129, 256, 256, 'relu', True, True, False, 256, 256),       # decoder_conv1_pointwise
    (70001, 304, 256, 'relu6', True, True, False, 320, 272),               # ragged rows (last tile: 113 rows), operands inside wider buffers
    (66000, 256, 256, 'none', False, False, True, 256, 256),               # no prologue, bias, no statistics
    (65536 + 129, 500, 256, 'none', True, True, False, 500, 256),          # K tail inside the last K-step (pitch 512), one row in the last tile
    (300, 256, 256, 'relu', True, True, False, 256, 256),                  # fewer tiles than CUs (forced)
    (128 * 256 * 2 + 64, 384, 256, 'relu', True, False, True, 384, 300),   # two full rounds + a half tile; prologue and bias, no statistics
]


@pytest.mark.parametrize('case', SB3_CASES, ids=lambda c: '%dx%d_%s%s%s' % (c[0], c[1], c[3], '_stats' if c[5] else '', '_bias' if c[6] else ''))
def test_pinned_schedule_forward_matches_float64(ops, case):
    """dl3p_pwconv_fwd_sb on pw_gemm_sb3_kernel (one workgroup per CU, the staging pinned into the MFMA gaps, the output tile leaving
    in slices under the next tile): the forward tolerances of the tiled split kernels, ragged M / K tails, slices of wider buffers"""
    M, K, N, act, pro, stats, has_bias, ldx, ldy = case
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', -1)
    L.set_option(b'sb3', 1)
    try:
        assert _plan(L, 5 + int(stats), M, K, N)[3] == 4, _plan(L, 5 + int(stats), M, K, N)
        g = torch.Generator(device=DEV); g.manual_seed(M % 9973 + 7 * K + 3)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        # the operand sits in a wider buffer whose other columns hold large values (a K tail must not leak them in)
        xbuf = rnd(M, ldx) * 50.0
        x = xbuf[:, :K]
        x.copy_(rnd(M, K))
        wt = rnd(N, K) / K ** 0.5
        sc = (torch.rand(K, device=DEV, generator=g) + 0.5) if pro else None
        sh = (rnd(K) * 0.3 + 0.2) if pro else None
        bias = rnd(N) * 0.1 if has_bias else None
        actc = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'relu6': ops.ACT_RELU6}[act]
        a64 = x.double()
        if pro:
            a64 = a64 * sc.double() + sh.double()
        if act != 'none':
            a64 = a64.clamp(0.0, 6.0 if act == 'relu6' else float('inf'))
        y64 = a64 @ wt.double().t()
        if has_bias:
            y64 = y64 + bias.double()
        wsp = ops.split_bf16x3(wt)
        ybuf = torch.full((M, ldy), 7.0, device=DEV)
        y = ybuf[:, :N]
        part = ops.new_partials(N, DEV) if stats else None
        res = ops.pwconv_fwd_sb(x, wsp, K, bias, sc, sh, actc, out=y, partials=part)
        scale = float(y64.abs().max())
        e = float((y.double() - y64).abs().max()) / scale
        assert e < 2e-5, ('forward', e)
        if ldy > N:
            assert float((ybuf[:, N:] - 7.0).abs().max()) == 0.0, 'columns beside the output were written'
        if stats:
            rows = res[1]
            assert rows == min(256, -(-M // 128)), rows
            p = part[:rows * 2 * N].reshape(rows, 2, N).double().sum(0)
            s1, s2 = y64.sum(0), (y64 * y64).sum(0)
            assert float((p[0] - s1).abs().max()) < 1e-4 * max(float(s1.abs().max()), float(M) ** 0.5), 'stat sum'
            assert float((p[1] - s2).abs().max()) < 1e-4 * float(s2.abs().max()), 'stat sum of squares'
        # the tiled kernel on the same launch: both within the bound, and of each other
        L.set_option(b'sb3', 0)
        y_old = ops.pwconv_fwd_sb(x, wsp, K, bias, sc, sh, actc)
        assert float((y_old.double() - y.double()).abs().max()) / scale < 2e-5
    finally:
        L.set_option(b'pw_small_min_rows', 64)
        L.set_option(b'sb3', -1)


def test_pinned_schedule_forward_is_the_default_on_the_long_decoder_layers_only(ops):
    L = ops.lib()
    L.set_option(b'pw_small_min_rows', -1)
    try:
        assert _plan(L, 6, 16 * 129 * 129, 304, 256)[3] == 4 and _plan(L, 6, 16 * 129 * 129, 256, 256)[3] == 4
        assert _plan(L, 5, 2 * 385 * 385, 256, 256)[3] == 4                       # BASELINE configs[3], batch 2
        assert _plan(L, 6, 16 * 33 * 33, 1280, 256)[3] != 4                       # too few rows
        assert _plan(L, 6, 16 * 129 * 129, 288, 256)[3] != 4                      # nine K-steps: the loop runs them in pairs
        assert _plan(L, 6, 16 * 129 * 129, 304, 304)[3] != 4
        # an activation the kernel does not carry falls back inside the call
        g = torch.Generator(device=DEV); g.manual_seed(5)
        x = torch.randn(66000, 256, device=DEV, generator=g)
        wt = torch.randn(256, 256, device=DEV, generator=g) / 16
        sc = torch.rand(256, device=DEV, generator=g) + 0.5
        sh = torch.randn(256, device=DEV, generator=g) * 0.3
        y = ops.pwconv_fwd_sb(x, ops.split_bf16x3(wt), 256, None, sc, sh, ops.ACT_HSWISH)
        u = x.double() * sc.double() + sh.double()
        y64 = (u * (u + 3).clamp(0, 6) / 6) @ wt.double().t()
        assert float((y.double() - y64).abs().max()) < 2e-5 * float(y64.abs().max())
    finally:
        L.set_option(b'pw_small_min_rows', 64)


def test_a_launch_the_pinned_schedule_form_does_not_serve_takes_the_tiled_plan(ops):
    """sb3 = 1 pins the pinned-schedule form wherever the SHAPE is served (the plan query reports it); the planner refuses it for a
    launch whose input activation it has no instantiation for (hard-swish) or that wants statistics and a bias together, and
    plans such a launch as if sb3 were 0.  Both runs then take the same tiled kernel, which is deterministic: output,
    statistic partials and their row count are bit-identical, no tolerance"""
    M, K, N = 300, 256, 256
    L = ops.lib()
    g = torch.Generator(device=DEV); g.manual_seed(31)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x, wt = rnd(M, K), rnd(N, K) / K ** 0.5
    sc, sh, bias = torch.rand(K, device=DEV, generator=g) + 0.5, rnd(K) * 0.3 + 0.2, rnd(N) * 0.1
    wsp = ops.split_bf16x3(wt)
    launches = {'hswish': (None, ops.ACT_HSWISH, False), 'stats_and_bias': (bias, ops.ACT_RELU, True)}

    def run(sb3):
        L.set_option(b'sb3', sb3)
        out = {}
        for name, (b, act, stats) in launches.items():
            part = torch.zeros(ops.MAX_STAT_ROWS * 2 * N, device=DEV) if stats else None
            res = ops.pwconv_fwd_sb(x, wsp, K, b, sc, sh, act, partials=part)
            out[name] = (res[0], res[1], part) if stats else (res, None, None)
        torch.cuda.synchronize()
        return out
    L.set_option(b'pw_small_min_rows', -1)
    try:
        L.set_option(b'sb3', 1)
        assert _plan(L, 5, M, K, N)[3] == 4 and _plan(L, 6, M, K, N)[3] == 4       # the shape-level route: pinned
        pinned, tiled = run(1), run(0)
        assert _plan(L, 5, M, K, N)[3] != 4
        for name in launches:
            (y1, rows1, p1), (y0, rows0, p0) = pinned[name], tiled[name]
            assert torch.equal(y1, y0), name
            assert rows1 == rows0, (name, rows1, rows0)
            if p1 is not None:
                assert rows1 > 0 and torch.equal(p1, p0), name
    finally:
        L.set_option(b'pw_small_min_rows', 64)
        L.set_option(b'sb3', -1)


@pytest.mark.parametrize('act_name,front_act', [('relu', 'relu'), ('relu6', 'relu6'), ('none', 'relu')])
@pytest.mark.parametrize('M', [16 * 129 * 129, 70001, 300])
def test_pinned_schedule_data_gradient_with_the_folded_apply(ops, M, act_name, front_act):
    """dl3p_pwconv_bwd_data_sb_apply on pw_gemm_sb3d_kernel (256 output columns over a reduction of 256, no accumulation): dz, gx and the
    fused BatchNorm-backward sums of the layer in front against float64 at the row-stationary kernel's tolerances, dz in place of g
    and in its own buffer bit for bit, operands inside wider buffers, rows past M untouched -- and dz equal to the row-stationary
    kernel's bit for bit (the same arithmetic)"""
    K = N = 256
    A = {'relu6': ops.ACT_RELU6, 'relu': ops.ACT_RELU, 'none': ops.ACT_NONE}
    act, fact = A[act_name], A[front_act]
    L = ops.lib()
    L.set_option(b'sb3', 1)
    try:
        g_ = torch.Generator(device=DEV); g_.manual_seed(M + 11)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g_)
        gbuf = rnd(M, N + 16); g = gbuf[:, :N]                  # operands with their own pitches
        zbuf = rnd(M, N + 32) * 1.5 + 0.3; z_out = zbuf[:, 8:8 + N]
        bsc, bsh = torch.rand(N, device=DEV, generator=g_) + 0.5, rnd(N) * 0.5 + (1.0 if act == ops.ACT_RELU6 else 0.0)
        mu, istd = rnd(N) * 0.2, torch.rand(N, device=DEV, generator=g_) + 0.5
        coef = torch.stack([torch.rand(N, device=DEV, generator=g_) + 0.5, rnd(N) * 0.1, rnd(N) * 0.1]).contiguous()
        w = (rnd(K, N) / N ** 0.5).contiguous()
        w_sp = ops.split_bf16x3(w)
        u = z_out.double() * bsc.double() + bsh.double()
        m = {'relu6': ((u > 0) & (u < 6)).double(), 'relu': (u > 0).double(), 'none': torch.ones_like(u)}[act_name]
        dz64 = coef[0].double() * (g.double() * m - coef[1].double() - (z_out.double() - mu.double()) * istd.double() * coef[2].double())
        gx64 = dz64 @ w.double().t()
        z = rnd(M, K)
        sc, sh = torch.rand(K, device=DEV, generator=g_) + 0.5, rnd(K) * 0.3 + (1.0 if fact == ops.ACT_RELU6 else 0.0)
        mean, invstd = z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
        # separate dz buffer, with the sums
        dzb = torch.full((M + 3, N + 8), 5.0, device=DEV)
        gxb = torch.full((M + 3, K + 4), 7.0, device=DEV)
        part = ops.new_partials(K, DEV)
        dz, gx, rows = ops.pwconv_bwd_data_sb_apply(g, z_out, bsc, bsh, act, mu, istd, coef, w_sp, N, dz=dzb[:M, :N], out=gxb[:M, :K],
                                                    z=z, scale=sc, shift=sh, act=fact, mean=mean, invstd=invstd, partials=part)
        assert rows == min(256, -(-M // 128)), rows            # (one partial row per workgroup: the pinned form took the launch)
        assert float((dz.double() - dz64).abs().max()) < 4e-6 * float(dz64.abs().max()), 'dz'
        assert float((gx.double() - gx64).abs().max()) < 2e-5 * float(gx64.abs().max()), 'gx'
        assert float((dzb[M:] - 5.0).abs().max()) == 0 and float((dzb[:, N:] - 5.0).abs().max()) == 0, 'dz wrote outside its rows / columns'
        assert float((gxb[M:] - 7.0).abs().max()) == 0 and float((gxb[:, K:] - 7.0).abs().max()) == 0, 'gx wrote outside its rows / columns'
        uu = z.double() * sc.double() + sh.double()
        fm = {'relu6': ((uu > 0) & (uu < 6)).double(), 'relu': (uu > 0).double(), 'none': torch.ones_like(uu)}[front_act]
        d = gx64 * fm
        xh = (z.double() - mean.double()) * invstd.double()
        p = part[:rows * 2 * K].reshape(rows, 2, K).double().sum(0)
        assert float((p[0] - d.sum(0)).abs().max()) < 2e-4 * float(d.abs().sum(0).max()), 'BN backward sum'
        assert float((p[1] - (d * xh).sum(0)).abs().max()) < 2e-4 * float((d * xh).abs().sum(0).max()), 'BN backward sum * xhat'
        # in place of g, no sums: the same bits
        g2 = gbuf.clone()
        dz2, gx2 = ops.pwconv_bwd_data_sb_apply(g2[:, :N], z_out, bsc, bsh, act, mu, istd, coef, w_sp, N)
        assert dz2.data_ptr() == g2.data_ptr() and torch.equal(dz2, dz) and torch.equal(gx2, gx)
        assert torch.equal(g2[:, N:], gbuf[:, N:])
        # the row-stationary kernel on the same launch (where it serves it): dz bit for bit, gx to rounding
        if L.pwconv_bwd_data_sb_apply_supported(M, K, N, act, 0):
            L.set_option(b'sb3', 0)
            dz3, gx3 = ops.pwconv_bwd_data_sb_apply(g, z_out, bsc, bsh, act, mu, istd, coef, w_sp, N, dz=torch.empty(M, N, device=DEV))
            assert torch.equal(dz3, dz)
            assert float((gx3.double() - gx.double()).abs().max()) < 2e-5 * float(gx64.abs().max())
    finally:
        L.set_option(b'sb3', -1)
