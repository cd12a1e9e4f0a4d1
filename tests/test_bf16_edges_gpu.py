"""The bf16 kernels at their lane-plan, view and last-row edges, against float64.

bf16_ew.hip picks 8-channel lanes (C % 8 == 0, every row stride % 8 == 0, every base 16-byte aligned) or 4-channel lanes, and
lane_split / pool_plan_b then cut the channels into slabs.  Every case here runs an entry point through ops.lib() on operands that
sit inside buffers of their own: canary bit patterns (NaN with a payload, +Inf, -Inf) fill the rows past the last row and, for the
'ld4' (row stride C + 4) and 'off4' (base 8 but not 16-byte aligned) layouts, the channels beside the view.  The canaries of every
output must come back bit-identical, and a canary read from an input shows up as a non-finite value in the float64 comparison.

References are float64 on the device.  The consumer-side prologue Q(act(z*scale+shift)) is formed the way DESIGN 4b specifies it
(one fp32 fma, the fp32 activation, one bf16 rounding), so that a bf16 rounding boundary cannot fall between the reference and the
device; everything after it is compared with float64 under a PER-ELEMENT bound: one bf16 ulp of the reference plus a few fp32
roundings of the magnitudes of the terms that formed that element (for the cancelling forms, d - c1 - xhat*c2, the residual add and
the resize lerps, of every term, not of the result), and for reductions the number of fp32 terms times the sum of |terms|.  There
is no tensor-scale term: a dropped shift or a wrong lane fails at any magnitude."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
U = 2.0 ** -24                      # one fp32 rounding, relative
NONE, RELU, RELU6, HSWISH, HSIGMOID = 0, 1, 2, 3, 4
SIXTH = float(np.float32(1.0) / np.float32(6.0))
# canary bf16 bit patterns: a NaN with a payload, +Inf, -Inf
CANARY = (0x7FA5, 0x7F80, -0x80)
LAYOUTS = ('contig', 'ld4', 'off4')
# cv = C/4 < 8, no divisor of cv in [8, cv), primes below and above 256 (1028 = 4 * 257, 2056 = 8 * 257) and production widths
CS = (4, 12, 20, 36, 72, 268, 960, 1028, 1280, 2056)
RATE, SEED = 0.3, 0x5EED


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _s():
    return torch.cuda.current_stream().cuda_stream


class Plane:
    """a (rows, C) bf16 operand inside its own buffer: `after` canary rows past its last row and, for 'ld4' / 'off4', canary
    channels beside it.  Nothing outside the buffer is ever addressed."""

    def __init__(self, rows, C, layout='contig', after=3, ld=None, lo=0):
        lo, w = {'contig': (lo, C), 'ld4': (0, C + 4), 'off4': (4, C + 8)}[layout]
        if ld is not None:
            w = ld
        n = (rows + after) * w
        pat = torch.tensor(CANARY, dtype=torch.int16, device=DEV)
        self.bits = pat.repeat((n + 2) // 3)[:n].reshape(rows + after, w).contiguous()
        self.t = self.bits.view(BF)[:rows, lo:lo + C]
        self.ld, self.rows, self.C, self.lo = w, rows, C, lo

    def set(self, v):
        self.t.copy_(v.reshape(self.rows, self.C).to(BF))
        self.keep = self.bits.clone()
        return self

    @property
    def p(self):
        return self.t.data_ptr()

    def intact(self, what):
        mask = torch.ones_like(self.bits, dtype=torch.bool)
        mask[:self.rows, self.lo:self.lo + self.C] = False
        bad = int((self.bits[mask] != self.keep[mask]).sum())
        assert bad == 0, '%s: %d canary elements beside / past the output changed' % (what, bad)


def plane(v, layout='contig', after=3):
    """an input plane holding v (rows, C)"""
    return Plane(v.shape[0], v.shape[1], layout, after).set(v)


def out_plane(rows, C, layout='contig', base=None):
    """an output plane: canaries everywhere, the view set to `base` (accumulating forms) or left as canaries"""
    o = Plane(rows, C, layout)
    if base is not None:
        o.set(base)
    else:
        o.keep = o.bits.clone()
    return o


def ulp(ref):
    """one bf16 ulp at |ref| (float64)"""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def close(got, ref, terms, what, k=4.0):
    """|got - ref| <= ulp_bf16(ref) + k * U * terms, per element (NaN / Inf in got fails)"""
    got = got.double()
    err = (got - ref).abs()
    bound = ulp(ref) + k * U * terms
    ok = err <= bound
    if not bool(ok.all()):
        i = int((~ok).reshape(-1).nonzero()[0])
        raise AssertionError('%s: %d of %d elements out of bound; first at flat %d: got %r want %r (bound %.3g)' % (
            what, int((~ok).sum()), ok.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
            float(bound.reshape(-1)[i])))


def bits(t):
    return t.contiguous().view(torch.int16)


def _rows_sum(part, rows, C, pairs, n, what):
    """partial rows [rows][len(pairs)][C] of fp32 sums: their float64 total within (n + rows) fp32 roundings of the sum of |terms|"""
    assert 0 < rows <= 2048, what
    tot = part[:rows * len(pairs) * C].double().reshape(rows, len(pairs), C).sum(0)
    for i, (want, terms) in enumerate(pairs):
        err = (tot[i] - want).abs()
        ok = err <= (n + rows + 4) * U * terms
        assert bool(ok.all()), '%s [%d]: worst %.3g (bound %.3g)' % (what, i, float(err.max()), float(((n + rows + 4) * U * terms).max()))


# ---- the fp32 prologue of DESIGN 4b, formed exactly: fmaf(z, scale, shift) (z*scale is exact in float64, one rounding to fp32;
# float64 -> fp32 double rounding is harmless here), the fp32 activation, one bf16 rounding
def fma32(z, sc, sh):
    if sc is None:
        return z.float()
    return (z.double() * sc.double() + sh.double()).float()


def act32(v, act):
    if act == NONE:
        return v
    if act == RELU:
        return v.clamp_min(0)
    if act == RELU6:
        return v.clamp(0, 6)
    t = (v + 3).clamp(0, 6) * SIXTH
    return v * t if act == HSWISH else t


def pro(z, sc, sh, act):
    """Q(act(z*scale + shift)) as bf16"""
    return act32(fma32(z, sc, sh), act).to(BF)


def grad64(u, act):
    """act'(u) of the fp32 pre-activation u (kinks decided on the fp32 values, like the device), in float64"""
    if act == NONE:
        return torch.ones_like(u, dtype=torch.float64)
    if act == RELU:
        return (u > 0).double()
    if act == RELU6:
        return ((u > 0) & (u < 6)).double()
    t = u + 3
    inside = ((t > 0) & (t < 6)).double() * SIXTH
    hs = t.clamp(0, 6).double() * SIXTH
    return hs + u.double() * inside if act == HSWISH else inside


def coefs(g, C):
    sc = (torch.rand(C, device=DEV, generator=g) + 0.5)
    sh = torch.randn(C, device=DEV, generator=g) * 0.5
    return sc.contiguous(), sh.contiguous()


def keep_scale(rate):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))


def drop_mask(ops, rate, step, M, C):
    m = torch.empty((M, C), dtype=torch.float32, device=DEV)
    ops.lib().dropout_mask(float(rate), SEED, step.data_ptr(), m.data_ptr(), M, C, _s())
    return m


def bnd(g, C):
    """BatchNorm-backward operands: scale, shift, mean, invstd, coef (3, C)"""
    sc, sh = coefs(g, C)
    mu = torch.randn(C, device=DEV, generator=g) * 0.3
    inv = torch.rand(C, device=DEV, generator=g) + 0.5
    coef = torch.randn(3, C, device=DEV, generator=g).contiguous()
    coef[0] = coef[0].abs() + 0.5
    return sc, sh, mu, inv, coef


def ws_nan(ops, N, HW, C):
    """the pooling workspace, NaN-filled: every float a launch reads must have been written by it"""
    n = ops.lib().pool_workspace_bf16(N, HW, C) // 4
    return torch.full((n,), float('nan'), dtype=torch.float32, device=DEV), n * 4


# ----------------------------------------------------------------------------------------- 3. lane plans against float64
def _per_element(ops, C, layout, N=3, H=7, W=19):
    """every per-element bf16_ew entry point at one (C, layout); returns {name: output} for the cross-layout bit check"""
    L, s = ops.lib(), _s()
    HW = H * W
    M = N * HW
    g = _gen(C * 7 + 1)
    rn = lambda *sh: torch.randn(*sh, device=DEV, generator=g)  # noqa: E731
    x, r, gy, z, old = (rn(M, C).mul(2).to(BF) for _ in range(5))
    sc, sh = coefs(g, C)
    rsc, rsh = coefs(g, C)
    step = torch.tensor([5], dtype=torch.int64, device=DEV)
    ks = keep_scale(RATE)
    keep = drop_mask(ops, RATE, step, M, C).double()
    out = {}
    X, R, GY, Z = plane(x, layout), plane(r, layout), plane(gy, layout), plane(z, layout)

    # affine_act: dropout(act(x*sc+sh)) + ract(r*rsc+rsh)
    a = pro(x, sc, sh, HSWISH).double()
    b = pro(r, rsc, rsh, RELU6).double()
    Y = out_plane(M, C, layout)
    L.affine_act_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, R.p, R.ld, rsc.data_ptr(), rsh.data_ptr(), RELU6,
                      RATE, SEED, step.data_ptr(), Y.p, Y.ld, M, C, s)
    close(Y.t, a * ks * keep + b, (a * ks).abs() + b.abs(), 'affine_act + dropout + residual', 3)
    Y.intact('affine_act')
    out['affine_act'] = Y.t

    # dropout alone: exactly the mask's zeros, kept values Q(v * keep_scale), bitwise
    Y2 = out_plane(M, C, layout)
    L.affine_act_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), RELU, None, 0, None, None, NONE,
                      RATE, SEED, step.data_ptr(), Y2.p, Y2.ld, M, C, s)
    want = torch.where(keep > 0, (pro(x, sc, sh, RELU).float() * ks).to(BF), torch.zeros((), dtype=BF, device=DEV))
    assert torch.equal(bits(Y2.t), bits(want)), 'affine_act dropout: not the mask of dl3p_dropout_mask / not Q(v * keep_scale)'
    Y2.intact('affine_act dropout')
    out['affine_act dropout'] = Y2.t

    # scale_mask_bwd: the forward's mask, plain (bitwise) and accumulating
    G = out_plane(M, C, layout)
    L.scale_mask_bwd_bf16(GY.p, GY.ld, RATE, SEED, step.data_ptr(), G.p, G.ld, 0, M, C, s)
    want = torch.where(keep > 0, (gy.float() * ks).to(BF), torch.zeros((), dtype=BF, device=DEV))
    assert torch.equal(bits(G.t), bits(want)), 'scale_mask_bwd: not the forward mask / not Q(g * keep_scale)'
    G.intact('scale_mask_bwd')
    G2 = out_plane(M, C, layout, base=old)
    L.scale_mask_bwd_bf16(GY.p, GY.ld, RATE, SEED, step.data_ptr(), G2.p, G2.ld, 1, M, C, s)
    gk = gy.double() * ks * keep
    close(G2.t, gk + old.double(), gk.abs() + old.double().abs(), 'scale_mask_bwd accumulate', 3)
    G2.intact('scale_mask_bwd accumulate')
    out['scale_mask_bwd'], out['scale_mask_bwd acc'] = G.t, G2.t

    # bn_bwd_apply: c0 * (g * act'(z*sc+sh) - c1 - (z - mean) * invstd * c2), plain and accumulating
    bsc, bsh, mu, inv, coef = bnd(g, C)
    u = fma32(z, bsc, bsh)
    d = gy.double() * grad64(u, HSWISH)
    zd = z.double()
    want = coef[0].double() * (d - coef[1].double() - (zd - mu.double()) * inv.double() * coef[2].double())
    terms = coef[0].double().abs() * (d.abs() + coef[1].double().abs() +
                                      (zd.abs() + mu.double().abs()) * inv.double() * coef[2].double().abs())
    for acc in (0, 1):
        D = out_plane(M, C, layout, base=old if acc else None)
        L.bn_bwd_apply_bf16(GY.p, GY.ld, Z.p, Z.ld, bsc.data_ptr(), bsh.data_ptr(), HSWISH, mu.data_ptr(), inv.data_ptr(),
                            coef.data_ptr(), D.p, D.ld, acc, M, C, s)
        if acc:
            close(D.t, want + old.double(), terms + old.double().abs(), 'bn_bwd_apply accumulate', 10)
        else:
            close(D.t, want, terms, 'bn_bwd_apply', 10)
        D.intact('bn_bwd_apply')
        out['bn_bwd_apply %d' % acc] = D.t

    # global_avgpool_bwd: gx[n, i, c] (+)= gy[n, c] / HW
    gp = rn(N, C).mul(8).to(BF)
    GP = plane(gp, layout)
    want = (gp.double() / HW).repeat_interleave(HW, 0)
    for acc in (0, 1):
        D = out_plane(M, C, layout, base=old if acc else None)
        L.global_avgpool_bwd_bf16(GP.p, GP.ld, D.p, D.ld, acc, N, HW, C, s)
        if acc:
            close(D.t, want + old.double(), want.abs() + old.double().abs(), 'global_avgpool_bwd accumulate', 3)
        else:
            close(D.t, want, want.abs(), 'global_avgpool_bwd', 2)
        D.intact('global_avgpool_bwd')
        out['gap_bwd %d' % acc] = D.t

    # scale_bcast_fwd: Q(act(x*sc+sh)) * Q(hsigmoid(s[n])) -- a product of two bf16 values, exact in fp32: one rounding
    sv = rn(N, C).mul(3).to(BF)
    SV = plane(sv, layout)
    Y3 = out_plane(M, C, layout)
    L.scale_bcast_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, SV.p, SV.ld, HSIGMOID, Y3.p, Y3.ld, N, HW, C, s)
    sq = act32(sv.float(), HSIGMOID).to(BF).double().repeat_interleave(HW, 0)
    close(Y3.t, a * sq, (a * sq).abs(), 'scale_bcast_fwd', 1)
    Y3.intact('scale_bcast_fwd')
    out['scale_bcast_fwd'] = Y3.t

    # ---- reductions: bounded by the number of fp32 terms times the sum of |terms|
    # bn_bwd_reduce partial rows
    part = torch.full((ops.MAX_STAT_ROWS * 2 * C,), float('nan'), dtype=torch.float32, device=DEV)
    rows = ctypes.c_int(0)
    L.bn_bwd_reduce_bf16(GY.p, GY.ld, Z.p, Z.ld, bsc.data_ptr(), bsh.data_ptr(), HSWISH, mu.data_ptr(), inv.data_ptr(),
                         part.data_ptr(), ctypes.byref(rows), M, C, s)
    pr = part[:rows.value * 2 * C].double().reshape(rows.value, 2, C).sum(0)
    xh = (zd - mu.double()) * inv.double()
    n = M + rows.value + 4
    for i, (w, t) in enumerate(((d.sum(0), d.abs().sum(0)),
                                ((d * xh).sum(0), (d.abs() * (zd.abs() + mu.double().abs()) * inv.double()).sum(0)))):
        err = (pr[i] - w).abs()
        assert bool((err <= n * U * t + 1e-30).all()), 'bn_bwd_reduce partial %d: worst %.3g (bound %.3g)' % (
            i, float(err.max()), float((n * U * t).max()))

    # global_avgpool_fwd with the prologue and an out_scale
    ws, wsb = ws_nan(ops, N, HW, C)
    P = out_plane(N, C, layout)
    L.global_avgpool_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, P.p, P.ld, 0.75, N, HW, C, ws.data_ptr(), wsb, s)
    a3 = a.reshape(N, HW, C)
    close(P.t, a3.sum(1) * 0.75 / HW, a3.abs().sum(1) * 0.75 / HW, 'global_avgpool_fwd (C=%d)' % C, HW + 40)
    P.intact('global_avgpool_fwd')

    # scale_bcast_bwd: gx (+)= gy * Q(hsigmoid(s)) per element, gs = sum over the image of gy * Q(act(x))
    ws, wsb = ws_nan(ops, N, HW, C)
    for acc in (0, 1):
        GX = out_plane(M, C, layout, base=old if acc else None)
        GS = out_plane(N, C, layout)
        L.scale_bcast_bwd_bf16(GY.p, GY.ld, X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, SV.p, SV.ld, HSIGMOID,
                               GX.p, GX.ld, acc, GS.p, GS.ld, N, HW, C, ws.data_ptr(), wsb, s)
        ga = gy.double() * sq
        if acc:
            close(GX.t, ga + old.double(), ga.abs() + old.double().abs(), 'scale_bcast_bwd gx accumulate', 3)
        else:
            close(GX.t, ga, ga.abs(), 'scale_bcast_bwd gx', 1)
            out['scale_bcast_bwd gx'] = GX.t
        ta = (gy.double() * a).reshape(N, HW, C)
        close(GS.t, ta.sum(1), ta.abs().sum(1), 'scale_bcast_bwd gs (C=%d)' % C, HW + 40)
        GX.intact('scale_bcast_bwd gx')
        GS.intact('scale_bcast_bwd gs')
    return out


# (N, H, W): M = N H W = 399 (15 mod 128), 127, 129 (1 mod 128), 64 and 65
EW_SHAPES = [(3, 7, 19), (1, 1, 127), (1, 3, 43), (1, 8, 8), (1, 5, 13)]


@pytest.mark.parametrize('NHW', EW_SHAPES)
@pytest.mark.parametrize('C', CS)
def test_ew_lane_plans(ops, C, NHW):
    """every per-element entry point on the 8-lane plan (where C allows it) and the 4-lane plans of the strided and the 8-byte
    aligned views: float64 per element, canaries intact, and the launches of one input bitwise equal across the plans"""
    runs = {lay: _per_element(ops, C, lay, *NHW) for lay in LAYOUTS}
    for name, t in runs['contig'].items():
        for lay in LAYOUTS[1:]:
            assert torch.equal(bits(t), bits(runs[lay][name])), '%s: the %s launch differs from the contiguous one (C=%d)' % (
                name, lay, C)


def _resize_ref(x, H, W):
    """float64 bilinear resize (half-pixel centres, edge clamp) of x (N, h, w, C) and the sum of |corner| per output"""
    N, h, w, C = x.shape

    def axis(o, n_in, n_out):
        src = (torch.arange(o, device=DEV, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5
        fl = torch.floor(src)
        lo = fl.clamp_min(0).long()
        hi = torch.ceil(src).clamp_max(n_in - 1).long()
        return lo, hi, src - fl
    ylo, yhi, ty = axis(H, h, H)
    xlo, xhi, tx = axis(W, w, W)
    xd = x.double()
    tl, tr = xd[:, ylo][:, :, xlo], xd[:, ylo][:, :, xhi]
    bl, br = xd[:, yhi][:, :, xlo], xd[:, yhi][:, :, xhi]
    tx4, ty4 = tx.view(1, 1, W, 1), ty.view(1, H, 1, 1)
    top = tl + (tr - tl) * tx4
    bot = bl + (br - bl) * tx4
    return top + (bot - top) * ty4, tl.abs() + tr.abs() + bl.abs() + br.abs()


@pytest.mark.parametrize('C', CS)
def test_resize_lane_plans(ops, C):
    """dl3p_resize_bilinear_{fwd,bwd}_bf16 on every lane plan: per-element float64 (the lerps bounded by their corners), canaries
    intact, the plans bitwise equal; the backward is the float64 transpose of the forward, accumulating"""
    L, s = ops.lib(), _s()
    N, h, w, H, W = 2, 5, 7, 9, 13
    g = _gen(C + 11)
    x = torch.randn(N, h, w, C, device=DEV, generator=g).to(BF)
    gy = torch.randn(N, H, W, C, device=DEV, generator=g).to(BF)
    old = torch.randn(N * h * w, C, device=DEV, generator=g).to(BF)
    want, corners = _resize_ref(x, H, W)
    # the transpose: d out / d in of the float64 forward, applied to gy (exact linear map: forward of unit vectors)
    eye = torch.eye(h * w, dtype=torch.float64, device=DEV).reshape(h * w, h, w, 1)
    Mf, _ = _resize_ref(eye, H, W)                       # (h w, H, W, 1): weight of input pixel p in every output pixel
    Mf = Mf.reshape(h * w, H * W)
    gyd = gy.double().reshape(N, H * W, C)
    gx_want = torch.einsum('po,noc->npc', Mf, gyd).reshape(N * h * w, C)
    gx_terms = torch.einsum('po,noc->npc', Mf.abs() + (Mf != 0), gyd.abs()).reshape(N * h * w, C)
    res = {}
    for lay in LAYOUTS:
        X = plane(x.reshape(-1, C), lay)
        Y = out_plane(N * H * W, C, lay)
        L.resize_bilinear_fwd_bf16(X.p, X.ld, Y.p, Y.ld, N, h, w, C, H, W, s)
        close(Y.t, want.reshape(-1, C), corners.reshape(-1, C), 'resize fwd (%s)' % lay, 8 + 2 * max(h, w))
        Y.intact('resize fwd')
        GY = plane(gy.reshape(-1, C), lay)
        G = out_plane(N * h * w, C, lay, base=old)
        L.resize_bilinear_bwd_bf16(GY.p, GY.ld, G.p, G.ld, 1, N, h, w, C, H, W, s)
        close(G.t, gx_want + old.double(), gx_terms + old.double().abs(), 'resize bwd accumulate (%s)' % lay, 24 + 2 * max(H, W))
        G.intact('resize bwd')
        res[lay] = (Y.t, G.t)
    for lay in LAYOUTS[1:]:
        for i in range(2):
            assert torch.equal(bits(res['contig'][i]), bits(res[lay][i])), 'resize %d: %s differs from contiguous' % (i, lay)


# (N, HW, C): the chunk count at its cap of 32 (one image, 512 x 1024, 16 channels), one chunk per image (8 small images), HW below
# 4 pixel lanes (px = 64 at C = 16), and the widths whose pool plans have no channel slab of 8..256 lanes
POOL_SHAPES = [(1, 512 * 1024, 16), (8, 48, 64), (8, 100, 16), (2, 33, 1028), (3, 17, 2056), (2, 40, 268)]


@pytest.mark.parametrize('N,HW,C', POOL_SHAPES)
def test_pool_reductions(ops, N, HW, C):
    """dl3p_global_avgpool_fwd_bf16 and dl3p_scale_bcast_bwd_bf16's scale gradient at the edges of pool_plan_b, against float64:
    every channel, with a NaN-filled workspace (a slab that is never reduced reads NaN).  Before the plan tiled every channel,
    C = 1028 and 2056 left channels 1024.. unreduced"""
    L, s = ops.lib(), _s()
    M = N * HW
    g = _gen(N * HW + C)
    x = torch.randn(M, C, device=DEV, generator=g).to(BF)
    gy = torch.randn(M, C, device=DEV, generator=g).to(BF)
    sv = torch.randn(N, C, device=DEV, generator=g).to(BF)
    sc, sh = coefs(g, C)
    a = pro(x, sc, sh, RELU6).double().reshape(N, HW, C)
    X, GY, SV = plane(x), plane(gy), plane(sv)
    ws, wsb = ws_nan(ops, N, HW, C)
    P = out_plane(N, C)
    L.global_avgpool_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), RELU6, P.p, P.ld, 1.0, N, HW, C, ws.data_ptr(), wsb, s)
    close(P.t, a.sum(1) / HW, a.abs().sum(1) / HW, 'global_avgpool_fwd', HW + 40)
    P.intact('global_avgpool_fwd')
    ws, wsb = ws_nan(ops, N, HW, C)
    GX, GS = out_plane(M, C), out_plane(N, C)
    L.scale_bcast_bwd_bf16(GY.p, GY.ld, X.p, X.ld, sc.data_ptr(), sh.data_ptr(), RELU6, SV.p, SV.ld, HSIGMOID, GX.p, GX.ld, 0,
                           GS.p, GS.ld, N, HW, C, ws.data_ptr(), wsb, s)
    sq = act32(sv.float(), HSIGMOID).to(BF).double()
    ga = gy.double().reshape(N, HW, C) * sq[:, None]
    assert torch.equal(bits(GX.t), bits(ga.reshape(M, C).to(BF))), 'scale_bcast_bwd gx: not Q(gy * Q(s))'
    ta = gy.double().reshape(N, HW, C) * a
    close(GS.t, ta.sum(1), ta.abs().sum(1), 'scale_bcast_bwd gs', HW + 40)
    GX.intact('scale_bcast_bwd gx')
    GS.intact('scale_bcast_bwd gs')
    # the BatchNorm-backward partial rows at the same shape
    bsc, bsh, mu, inv, _ = bnd(g, C)
    part = torch.full((ops.MAX_STAT_ROWS * 2 * C,), float('nan'), dtype=torch.float32, device=DEV)
    rows = ctypes.c_int(0)
    L.bn_bwd_reduce_bf16(GY.p, GY.ld, X.p, X.ld, bsc.data_ptr(), bsh.data_ptr(), RELU6, mu.data_ptr(), inv.data_ptr(),
                         part.data_ptr(), ctypes.byref(rows), M, C, s)
    pr = part[:rows.value * 2 * C].double().reshape(rows.value, 2, C).sum(0)
    d = gy.double() * grad64(fma32(x, bsc, bsh), RELU6)
    xd = x.double()
    xh = (xd - mu.double()) * inv.double()
    n = M + rows.value + 4
    err0, t0 = (pr[0] - d.sum(0)).abs(), d.abs().sum(0)
    err1, t1 = (pr[1] - (d * xh).sum(0)).abs(), (d.abs() * (xd.abs() + mu.double().abs()) * inv.double()).sum(0)
    assert bool((err0 <= n * U * t0).all()) and bool((err1 <= n * U * t1).all()), 'bn_bwd_reduce partials'


# -------------------------------------------------------------------------------------------------------- avgpool2d
@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('st', [1, 2, 3])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_avgpool_bf16(ops, k, st, layout):
    """dl3p_avgpool2d_{fwd,bwd}_bf16 (fixed 4-channel lanes) at every k, s <= 3, with H and W that leave the last rows and columns
    in no window when s > 1: float64 per element, the backward accumulating, canaries intact"""
    L, s = ops.lib(), _s()
    N, C = 2, 20
    H, W = 3 * st + k + (st > 1), 4 * st + k + (st > 1)
    Ho, Wo = (H - k) // st + 1, (W - k) // st + 1
    g = _gen(k * 10 + st)
    x = torch.randn(N * H * W, C, device=DEV, generator=g).to(BF)
    dy = torch.randn(N * Ho * Wo, C, device=DEV, generator=g).to(BF)
    old = torch.randn(N * H * W, C, device=DEV, generator=g).to(BF)
    sc, sh = coefs(g, C)
    a = pro(x, sc, sh, RELU6).double().reshape(N, H, W, C)
    want = torch.zeros(N, Ho, Wo, C, dtype=torch.float64, device=DEV)
    absw = torch.zeros_like(want)
    for ky in range(k):
        for kx in range(k):
            tap = a[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st]
            want += tap
            absw += tap.abs()
    X = plane(x, layout)
    Y = out_plane(N * Ho * Wo, C, layout)
    L.avgpool2d_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), RELU6, Y.p, Y.ld, N, H, W, C, k, st, Ho, Wo, s)
    close(Y.t, (want / (k * k)).reshape(-1, C), (absw / (k * k)).reshape(-1, C), 'avgpool fwd', k * k + 2)
    Y.intact('avgpool fwd')
    gx = torch.zeros(N, H, W, C, dtype=torch.float64, device=DEV)
    gabs = torch.zeros_like(gx)
    dyd = dy.double().reshape(N, Ho, Wo, C) / (k * k)
    for ky in range(k):
        for kx in range(k):
            gx[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st] += dyd
            gabs[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st] += dyd.abs()
    DY = plane(dy, layout)
    G = out_plane(N * H * W, C, layout, base=old)
    L.avgpool2d_bwd_bf16(DY.p, DY.ld, G.p, G.ld, 1, N, H, W, C, k, st, Ho, Wo, s)
    close(G.t, gx.reshape(-1, C) + old.double(), gabs.reshape(-1, C) + old.double().abs(), 'avgpool bwd accumulate', k * k + 3)
    G.intact('avgpool bwd')


# ------------------------------------------------------------------------------------------------ 4. conversions
def test_f32_to_bf16(ops):
    """dl3p_f32_to_bf16: round-to-nearest-even ties, NaN stays NaN, +-Inf, overflow past bf16's largest finite value, subnormals,
    at lengths n % 4 = 0..3 (the tail is one thread's): every non-NaN result bitwise torch's rounding"""
    L, s = ops.lib(), _s()
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.3895314e38, 3.39e38, -3.4e38, 3.3961776e38,
                        1e-40, -1e-40, 1.4e-45, 2.0 ** -126, 2.0 ** -133, 1.0, -1.0], dtype=np.float32)
    # exact ties: bf16 value + half its ulp (even and odd mantissas), and one float32 step either side
    base = np.array([1.0, 1.0078125, 1.015625, 3.0, -5.5, 1e-3, 2.0 ** -127], dtype=np.float32)
    tb = base.view(np.uint32) & np.uint32(0xFFFF0000)
    ties = np.concatenate([(tb + 0x8000).view(np.float32), (tb + 0x7FFF).view(np.float32), (tb + 0x8001).view(np.float32)])
    rng = np.random.default_rng(0)
    rnd = (rng.standard_normal(4096) * 10.0 ** rng.integers(-30, 30, 4096)).astype(np.float32)
    allv = np.concatenate([special, ties, rnd]).astype(np.float32)
    for n in (1, 2, 3, 4, 5, 6, 7, len(allv) - 3, len(allv) - 2, len(allv) - 1, len(allv)):
        src = torch.from_numpy(allv[:n].copy()).to(DEV)
        dst = torch.full((n + 5,), -0x80, dtype=torch.int16, device=DEV)
        L.f32_to_bf16(src.data_ptr(), dst.data_ptr(), n, s)
        got = dst[:n].view(BF).cpu()
        want = torch.from_numpy(allv[:n].copy()).to(BF)
        nan = torch.isnan(want)
        assert bool(torch.isnan(got[nan]).all()), 'f32_to_bf16: a NaN came back as a number (n=%d)' % n
        assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), 'f32_to_bf16 (n=%d): %s' % (
            n, (got[~nan].view(torch.int16) != want[~nan].view(torch.int16)).nonzero()[:4].flatten().tolist())
        assert bool((dst[n:] == -0x80).all()), 'f32_to_bf16 wrote past n'
    # the scalar tail (one thread, n % 4 elements): every special value and tie once at the end of a 5..7-element launch
    edge = np.concatenate([special, ties]).astype(np.float32)
    for i in range(0, len(edge), 3):
        for t in range(1, min(3, len(edge) - i) + 1):
            v = np.concatenate([rnd[:4], edge[i:i + t]]).astype(np.float32)
            src = torch.from_numpy(v).to(DEV)
            dst = torch.full((len(v) + 3,), -0x80, dtype=torch.int16, device=DEV)
            L.f32_to_bf16(src.data_ptr(), dst.data_ptr(), len(v), s)
            got, want = dst[:len(v)].view(BF).cpu(), torch.from_numpy(v).to(BF)
            nan = torch.isnan(want)
            assert bool(torch.isnan(got[nan]).all()) and torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), (
                'f32_to_bf16 tail: %r' % (edge[i:i + t].tolist(),))
            assert bool((dst[len(v):] == -0x80).all()), 'f32_to_bf16 wrote past n'


@pytest.mark.parametrize('div,sub', [(127.5, 1.0), (1.0, 0.0), (255.0, 0.5)])
def test_u8_to_bf16(ops, div, sub):
    """dl3p_u8_to_bf16 over every byte value at ragged lengths, against Q(float32(b) / div - sub)"""
    L, s = ops.lib(), _s()
    for n in (256, 257, 258, 259, 1 + 4 * 300, 3):
        b = (torch.arange(n, dtype=torch.int64, device=DEV) * 7 % 256).to(torch.uint8)
        dst = torch.full((n + 5,), -0x80, dtype=torch.int16, device=DEV)
        L.u8_to_bf16(b.data_ptr(), dst.data_ptr(), n, float(div), float(sub), s)
        bd = b.double()
        close(dst[:n].view(BF), bd / div - sub, bd / div + sub, 'u8_to_bf16 n=%d' % n, 2)
        assert bool((dst[n:] == -0x80).all()), 'u8_to_bf16 wrote past n'


def test_transpose_batch_bf16(ops):
    """dl3p_transpose_batch_bf16 over a table of matrices with K and N off the 32 tile, some below 32: bitwise torch's transpose
    and rounding, the gaps between the matrices untouched"""
    L, s = ops.lib(), _s()
    shapes = [(33, 70), (7, 100), (96, 5), (31, 31), (65, 129), (1, 40)]
    offs, o = [], 0
    for K, N in shapes:
        offs.append(o)
        o += K * N + 9                                   # a gap after each matrix
    src = torch.randn(o, device=DEV, generator=_gen(3)) * 5
    table = torch.tensor([[off, K, N, 0] for off, (K, N) in zip(offs, shapes)], dtype=torch.int32, device=DEV)
    dst = torch.full((o,), 0x7FA5, dtype=torch.int16, device=DEV)
    L.transpose_batch_bf16(src.data_ptr(), dst.data_ptr(), table.data_ptr(), len(shapes), s)
    touched = torch.zeros(o, dtype=torch.bool, device=DEV)
    for off, (K, N) in zip(offs, shapes):
        want = src[off:off + K * N].reshape(K, N).t().contiguous().to(BF)
        assert torch.equal(dst[off:off + K * N].reshape(N, K), want.view(torch.int16)), 'transpose %dx%d' % (K, N)
        touched[off:off + K * N] = True
    assert bool((dst[~touched] == 0x7FA5).all()), 'transpose_batch_bf16 wrote between the matrices'


# -------------------------------------------------------------------------------- 2. the pointwise GEMM past its last row
def _pw_ref(x, sc, sh, act, w, bias):
    """float64 y = Q(act(x*sc+sh)) @ Q(w) (+ bias) and the sum of |terms| per output"""
    a = pro(x, sc, sh, act).double() if sc is not None else x.double()
    wq = w.to(BF).double()
    y = a @ wq
    if bias is not None:
        y = y + bias.double()
    t = a.abs() @ wq.abs() + (bias.double().abs() if bias is not None else 0)
    return y, t


ROWS = [1, 64, 65, 127, 129, 255, 1 + (1 << 16), 127 + (1 << 16)]
# (M, kg): every row count on the rule's kernel (kg 0), the tiled kernel's row counts also with its K groups pinned to 1, 2 and 4
PW_CASES = [(M, 0) for M in ROWS] + [(M, kg) for M in (65, 129, 255) for kg in (1, 2, 4)]


@pytest.mark.parametrize('M,kg', PW_CASES)
@pytest.mark.parametrize('K,N', [(40, 32), (104, 72)])
def test_pwconv_bf16_rows(ops, M, kg, K, N):
    """dl3p_pwconv_fwd_bf16 and dl3p_pwconv_bwd_data_bf16 at the row counts where their kernels change (the few-row kernel to
    M = 64, the tiled kernel, the streaming kernel from 2^16 rows in 32-row tiles), on prefix views (lo = 0) beside canaries, K off
    the 32-step: the canary rows after M and the channels beside the output slice bit-identical, every row against float64.  The
    forward with and without the prologue and the bias, to a bf16 and to an fp32 output; the data gradient plain, accumulating
    and from an fp32 gradient"""
    L, s = ops.lib(), _s()
    if kg:
        L.set_option(b'bf16_kg', kg)
    try:
        g = _gen(M + K + N)
        x = torch.randn(M, K, device=DEV, generator=g).to(BF)
        w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
        bias = torch.randn(N, device=DEV, generator=g)
        sc, sh = coefs(g, K)
        wt = w.t().contiguous().to(BF)
        X = Plane(M, K, ld=K + 16, after=5).set(x)              # the prefix view [0, K) of a K + 16 wide buffer
        for pro_on, with_bias, f32 in ((False, False, False), (True, True, False), (True, False, True)):
            if f32 and kg > 1:
                continue                    # (gemm_b never takes K groups with an fp32 operand: that is the kg = 1 case again)
            stats = pro_on and not f32
            want, terms = _pw_ref(x, sc if pro_on else None, sh, HSWISH, w, bias if with_bias else None)
            what = 'pwconv_fwd_bf16 M=%d kg=%d pro=%d bias=%d f32=%d' % (M, kg, pro_on, with_bias, f32)
            if f32:
                lo, ld = 8, N + 16
                buf = torch.full((M + 4, ld), float('nan'), dtype=torch.float32, device=DEV)
                keep = buf.clone()
                y = buf[:M, lo:lo + N]
            else:
                Y = Plane(M, N, ld=N + 16, after=4, lo=8)
                Y.keep = Y.bits.clone()
                y = Y.t
            part = torch.full((ops.MAX_STAT_ROWS * 2 * N,), float('nan'), dtype=torch.float32, device=DEV)
            rows = ctypes.c_int(0)
            L.pwconv_fwd_bf16(X.p, X.ld, 0, sc.data_ptr() if pro_on else None, sh.data_ptr() if pro_on else None,
                              HSWISH if pro_on else NONE, wt.data_ptr(), bias.data_ptr() if with_bias else None,
                              y.data_ptr(), y.stride(0), int(f32), part.data_ptr() if stats else None,
                              ctypes.byref(rows) if stats else None, M, K, N, s)
            if stats:                       # (sum, sum of squares) of the STORED values
                yq = y.double()
                _rows_sum(part, rows.value, N, [(yq.sum(0), yq.abs().sum(0)), ((yq * yq).sum(0), (yq * yq).sum(0))],
                          M, what + ' statistics')
            if f32:
                err = (y.double() - want).abs()
                assert bool((err <= (K + 4) * U * terms).all()), what
                mask = torch.ones_like(buf, dtype=torch.bool)
                mask[:M, lo:lo + N] = False
                assert torch.equal(buf[mask].view(torch.int32), keep[mask].view(torch.int32)), what + ': canaries'
            else:
                close(y, want, terms, what, K + 4)
                Y.intact(what)
        # the data gradient gx (+)= dy @ Q(w)^T
        dy = torch.randn(M, N, device=DEV, generator=g)
        old = torch.randn(M, K, device=DEV, generator=g).to(BF)
        wb = w.to(BF).contiguous()
        wq = wb.double()
        for acc, dy_f32 in ((0, 0), (1, 0), (0, 1)):
            what = 'pwconv_bwd_data_bf16 M=%d kg=%d acc=%d dy_f32=%d' % (M, kg, acc, dy_f32)
            dq = dy if dy_f32 else dy.to(BF)
            if dy_f32:
                dbuf = torch.full((M + 3, N + 8), float('nan'), dtype=torch.float32, device=DEV)
                dbuf[:M, :N] = dq
                dp, ldd = dbuf.data_ptr(), N + 8
            else:
                DY = Plane(M, N, ld=N + 8).set(dq)
                dp, ldd = DY.p, DY.ld
            G = Plane(M, K, ld=K + 24, after=4, lo=8)
            if acc:
                G.set(old)
            else:
                G.keep = G.bits.clone()
            L.pwconv_bwd_data_bf16(dp, ldd, dy_f32, wb.data_ptr(), G.p, G.ld, acc, M, K, N, s)
            dd = dq.to(BF).double()                 # (an fp32 gradient enters the bf16 matrix pipe rounded to bf16)
            want = dd @ wq.t() + (old.double() if acc else 0)
            terms = dd.abs() @ wq.abs().t() + (old.double().abs() if acc else 0)
            close(G.t, want, terms, what, N + 4)
            G.intact(what)
        if M > 64:
            # the data gradient with the BatchNorm-backward sums of the BatchNorm behind it, over the STORED gradient
            z = (torch.randn(M, K, device=DEV, generator=g) * 2).to(BF)
            bsc, bsh, mu, inv, _ = bnd(g, K)
            Z, DY = Plane(M, K, ld=K + 8).set(z), Plane(M, N, ld=N + 8).set(dy.to(BF))
            for acc in (0, 1):
                what = 'pwconv_bwd_data_bn_bf16 M=%d kg=%d acc=%d' % (M, kg, acc)
                G = Plane(M, K, ld=K + 24, after=4, lo=8)
                if acc:
                    G.set(old)
                else:
                    G.keep = G.bits.clone()
                part = torch.full((ops.MAX_STAT_ROWS * 2 * K,), float('nan'), dtype=torch.float32, device=DEV)
                rows = ctypes.c_int(0)
                L.pwconv_bwd_data_bn_bf16(DY.p, DY.ld, wb.data_ptr(), G.p, G.ld, acc, M, K, N, Z.p, Z.ld, bsc.data_ptr(),
                                          bsh.data_ptr(), RELU6, mu.data_ptr(), inv.data_ptr(), part.data_ptr(),
                                          ctypes.byref(rows), s)
                dd = dy.to(BF).double()
                want = dd @ wq.t() + (old.double() if acc else 0)
                terms = dd.abs() @ wq.abs().t() + (old.double().abs() if acc else 0)
                close(G.t, want, terms, what, N + 4)
                G.intact(what)
                d = G.t.double() * grad64(fma32(z, bsc, bsh), RELU6)
                zd = z.double()
                xh = (zd - mu.double()) * inv.double()
                _rows_sum(part, rows.value, K, [(d.sum(0), d.abs().sum(0)),
                                                ((d * xh).sum(0), (d.abs() * (zd.abs() + mu.double().abs()) * inv.double()).sum(0))],
                          M, what + ' BatchNorm sums')
        # the weight gradient gw = Q(act(x*sc+sh))^T dy (+ the bias gradient), and its slab form
        DY = Plane(M, N, ld=N + 8).set(dy.to(BF))
        a = pro(x, sc, sh, HSWISH).double()
        dd = dy.to(BF).double()
        need = L.pwconv_bwd_weight_workspace_bf16(M, K, N) // 4
        ws = torch.full((need + 4,), float('nan'), dtype=torch.float32, device=DEV)
        gw = torch.full((K, N), float('nan'), dtype=torch.float32, device=DEV)
        gb = torch.full((N,), float('nan'), dtype=torch.float32, device=DEV)
        L.pwconv_bwd_weight_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, DY.p, DY.ld, 0, gw.data_ptr(), gb.data_ptr(),
                                 ws.data_ptr(), ws.numel() * 4, M, K, N, s)
        n = M + 2 * ops.MAX_STAT_ROWS
        gw_want, gw_terms = a.t() @ dd, a.abs().t() @ dd.abs()
        what = 'pwconv_bwd_weight_bf16 M=%d kg=%d' % (M, kg)
        assert bool(((gw.double() - gw_want).abs() <= n * U * gw_terms).all()), what
        assert bool(((gb.double() - dd.sum(0)).abs() <= n * U * dd.abs().sum(0)).all()), what + ' bias'
        if M > 64:
            ws.fill_(float('nan'))
            rows = ctypes.c_int(0)
            L.pwconv_bwd_weight_slabs_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, DY.p, DY.ld, 0, ws.data_ptr(),
                                           ws.numel() * 4, ctypes.byref(rows), M, K, N, s)
            slab = ws[:rows.value * K * N].double().reshape(rows.value, K, N).sum(0)
            assert bool(((slab - gw_want).abs() <= n * U * gw_terms).all()), what + ' slabs'
    finally:
        if kg:
            L.set_option(b'bf16_kg', -1)


# ------------------------------------------------------------------------------- 5. configs[4] non-conv ops at production shape
@pytest.mark.parametrize('N,H,W,C', [(1, 512, 1024, 16), (1, 256, 512, 72), (1, 64, 128, 960)])
def test_production_bn_backward(ops, N, H, W, C):
    """the BatchNorm backward of MobileNetV3-Large 1024 x 2048 (reduce, finalize, apply) on every element against float64"""
    L, s = ops.lib(), _s()
    M = N * H * W
    g = _gen(C)
    gy = torch.randn(M, C, device=DEV, generator=g).to(BF)
    z = (torch.randn(M, C, device=DEV, generator=g) * 2 + 0.3).to(BF)
    bsc, bsh, mu, inv, coef = bnd(g, C)
    GY, Z = plane(gy), plane(z)
    part = torch.full((ops.MAX_STAT_ROWS * 2 * C,), float('nan'), dtype=torch.float32, device=DEV)
    rows = ctypes.c_int(0)
    L.bn_bwd_reduce_bf16(GY.p, GY.ld, Z.p, Z.ld, bsc.data_ptr(), bsh.data_ptr(), HSWISH, mu.data_ptr(), inv.data_ptr(),
                         part.data_ptr(), ctypes.byref(rows), M, C, s)
    pr = part[:rows.value * 2 * C].double().reshape(rows.value, 2, C).sum(0)
    d = gy.double() * grad64(fma32(z, bsc, bsh), HSWISH)
    zd = z.double()
    xh = (zd - mu.double()) * inv.double()
    n = M // max(rows.value, 1) + rows.value + 8           # a thread's serial chain plus the row sums
    t0, t1 = d.abs().sum(0), (d.abs() * (zd.abs() + mu.double().abs()) * inv.double()).sum(0)
    assert bool(((pr[0] - d.sum(0)).abs() <= (n + 256) * U * t0).all()), 'bn_bwd_reduce sum d'
    assert bool(((pr[1] - (d * xh).sum(0)).abs() <= (n + 256) * U * t1).all()), 'bn_bwd_reduce sum d xhat'
    D = out_plane(M, C)
    L.bn_bwd_apply_bf16(GY.p, GY.ld, Z.p, Z.ld, bsc.data_ptr(), bsh.data_ptr(), HSWISH, mu.data_ptr(), inv.data_ptr(),
                        coef.data_ptr(), D.p, D.ld, 0, M, C, s)
    c0, c1, c2 = (coef[i].double() for i in range(3))
    want = c0 * (d - c1 - xh * c2)
    terms = c0.abs() * (d.abs() + c1.abs() + (zd.abs() + mu.double().abs()) * inv.double() * c2.abs())
    close(D.t, want, terms, 'bn_bwd_apply at %s' % ((N, H, W, C),), 10)
    D.intact('bn_bwd_apply')


def test_production_se_and_resize(ops):
    """the (1, 64, 128, 960) squeeze-excite of configs[4]: its global pool, multiply and both gradients, and the decoder's 4x
    bilinear resize (256 channels, 64 x 128 -> 256 x 512) forward and backward, on every element against float64"""
    L, s = ops.lib(), _s()
    N, H, W, C = 1, 64, 128, 960
    HW, M = H * W, H * W
    g = _gen(960)
    x = torch.randn(M, C, device=DEV, generator=g).to(BF)
    gy = torch.randn(M, C, device=DEV, generator=g).to(BF)
    sv = torch.randn(N, C, device=DEV, generator=g).to(BF)
    sc, sh = coefs(g, C)
    X, GY, SV = plane(x), plane(gy), plane(sv)
    a = pro(x, sc, sh, HSWISH).double()
    ws, wsb = ws_nan(ops, N, HW, C)
    P = out_plane(N, C)
    L.global_avgpool_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, P.p, P.ld, 1.0, N, HW, C, ws.data_ptr(), wsb, s)
    close(P.t, a.sum(0, keepdim=True) / HW, a.abs().sum(0, keepdim=True) / HW, 'SE pool', HW + 40)
    sq = act32(sv.float(), HSIGMOID).to(BF).double()
    Y = out_plane(M, C)
    L.scale_bcast_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, SV.p, SV.ld, HSIGMOID, Y.p, Y.ld, N, HW, C, s)
    close(Y.t, a * sq, (a * sq).abs(), 'SE multiply', 1)
    ws, wsb = ws_nan(ops, N, HW, C)
    GX, GS = out_plane(M, C), out_plane(N, C)
    L.scale_bcast_bwd_bf16(GY.p, GY.ld, X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, SV.p, SV.ld, HSIGMOID, GX.p, GX.ld, 0,
                           GS.p, GS.ld, N, HW, C, ws.data_ptr(), wsb, s)
    close(GX.t, gy.double() * sq, (gy.double() * sq).abs(), 'SE multiply gx', 1)
    ta = gy.double() * a
    close(GS.t, ta.sum(0, keepdim=True), ta.abs().sum(0, keepdim=True), 'SE multiply gs', HW + 40)
    for o in (P, Y, GX, GS):
        o.intact('SE')
    # decoder resize
    h, w, Cr, Hr, Wr = 64, 128, 256, 256, 512
    xr = torch.randn(h * w, Cr, device=DEV, generator=g).to(BF)
    want, corners = _resize_ref(xr.reshape(1, h, w, Cr), Hr, Wr)
    XR = plane(xr)
    YR = out_plane(Hr * Wr, Cr)
    L.resize_bilinear_fwd_bf16(XR.p, XR.ld, YR.p, YR.ld, 1, h, w, Cr, Hr, Wr, s)
    close(YR.t, want.reshape(-1, Cr), corners.reshape(-1, Cr), 'decoder resize', 8 + 2 * w)
    YR.intact('decoder resize')
    gyr = torch.randn(Hr * Wr, Cr, device=DEV, generator=g).to(BF)
    # the transpose, separable: gx = Ry^T gy Rx with the 1-D float64 interpolation matrices
    def mat(n_in, n_out):
        eye = torch.eye(n_in, dtype=torch.float64, device=DEV)
        m, _ = _resize_ref(eye.reshape(1, n_in, 1, n_in).expand(1, n_in, 1, n_in).contiguous(), n_out, 1)
        return m.reshape(n_out, n_in)
    Ry, Rx = mat(h, Hr), mat(w, Wr)
    Ay, Ax = Ry.abs() + (Ry != 0), Rx.abs() + (Rx != 0)        # (a weight fp32 rounding can move counts with |g|)
    gg = gyr.double().reshape(Hr, Wr, Cr)
    gx_want = torch.einsum('Xx,yXc->yxc', Rx, torch.einsum('Yy,YXc->yXc', Ry, gg)).reshape(-1, Cr)
    gx_terms = torch.einsum('Xx,yXc->yxc', Ax, torch.einsum('Yy,YXc->yXc', Ay, gg.abs())).reshape(-1, Cr)
    GYR = plane(gyr)
    GR = out_plane(h * w, Cr)
    L.resize_bilinear_bwd_bf16(GYR.p, GYR.ld, GR.p, GR.ld, 0, 1, h, w, Cr, Hr, Wr, s)
    close(GR.t, gx_want, gx_terms, 'decoder resize backward', 24 + 2 * Wr)
    GR.intact('decoder resize backward')


@pytest.mark.parametrize('H,W,C,ldo', [(128, 128, 128, 256), (64, 64, 256, 512)])
def test_production_peleenet_avgpool(ops, H, W, C, ldo):
    """the two bf16 transition pools of PeleeNet at 512 x 512 (batch 2): AveragePooling2D(2, 2) with the producer's prologue into
    the prefix [0, C) of the next dense block's buffer, and the accumulating backward, on every element against float64"""
    L, s = ops.lib(), _s()
    N, k, st = 2, 2, 2
    Ho, Wo = (H - k) // st + 1, (W - k) // st + 1
    g = _gen(C + H)
    x = torch.randn(N * H * W, C, device=DEV, generator=g).to(BF)
    dy = torch.randn(N * Ho * Wo, C, device=DEV, generator=g).to(BF)
    old = torch.randn(N * H * W, C, device=DEV, generator=g).to(BF)
    sc, sh = coefs(g, C)
    a = pro(x, sc, sh, RELU).double().reshape(N, H, W, C)
    taps = [(ky, kx) for ky in range(k) for kx in range(k)]
    win = lambda t, ky, kx: t[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st]  # noqa: E731
    want = sum(win(a, ky, kx) for ky, kx in taps) / (k * k)
    absw = sum(win(a, ky, kx).abs() for ky, kx in taps) / (k * k)
    X = plane(x)
    Y = Plane(N * Ho * Wo, C, ld=ldo)
    Y.keep = Y.bits.clone()
    L.avgpool2d_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), RELU, Y.p, Y.ld, N, H, W, C, k, st, Ho, Wo, s)
    close(Y.t, want.reshape(-1, C), absw.reshape(-1, C), 'avgpool fwd', k * k + 2)
    Y.intact('avgpool fwd')
    gx = torch.zeros(N, H, W, C, dtype=torch.float64, device=DEV)
    gabs = torch.zeros_like(gx)
    dyd = dy.double().reshape(N, Ho, Wo, C) / (k * k)
    for ky, kx in taps:
        win(gx, ky, kx).add_(dyd)
        win(gabs, ky, kx).add_(dyd.abs())
    DY = plane(dy)
    G = out_plane(N * H * W, C, base=old)
    L.avgpool2d_bwd_bf16(DY.p, DY.ld, G.p, G.ld, 1, N, H, W, C, k, st, Ho, Wo, s)
    close(G.t, gx.reshape(-1, C) + old.double(), gabs.reshape(-1, C) + old.double().abs(), 'avgpool bwd', k * k + 3)
    G.intact('avgpool bwd')


# ------------------------------------------------------------------------------------------ depthwise and dense-conv gathers
def _pad_for(H, W, k, st, r, pt, pl, Ho, Wo):
    keff = (k - 1) * r + 1
    return pl, max(0, (Wo - 1) * st + keff - W - pl), pt, max(0, (Ho - 1) * st + keff - H - pt)


def _dw64(a, w, st, r, pt, pl, Ho, Wo):
    """float64 depthwise conv of a (N, H, W, C) with w (k, k, C), 'same' geometry (pt, pl) -> (N, Ho, Wo, C)"""
    import torch.nn.functional as F
    N, H, W, C = a.shape
    k = w.shape[0]
    ap = F.pad(a.permute(0, 3, 1, 2), _pad_for(H, W, k, st, r, pt, pl, Ho, Wo))
    y = F.conv2d(ap, w.permute(2, 0, 1).unsqueeze(1), stride=st, dilation=r, groups=C)[:, :, :Ho, :Wo]
    return y.permute(0, 2, 3, 1)


def _dw_grads(a, w, dy, st, r, pt, pl, Ho, Wo):
    """float64 (gx, gw) of the depthwise conv: the transposes, by autograd of _dw64"""
    a = a.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    _dw64(a, w, st, r, pt, pl, Ho, Wo).backward(dy)
    return a.grad, w.grad


# (N, H, W, C, k, stride, rate): the 3x3 window kernels (the weight-gradient window from 16384 output pixels), rate 2, the 5x5 strip
# kernels, rates 6 and 18, stride 2 at 3x3 and 5x5
DW_CASES = [(1, 129, 129, 24, 3, 1, 1), (2, 33, 35, 20, 3, 1, 2), (2, 31, 29, 24, 5, 1, 1), (1, 40, 45, 12, 5, 1, 6),
            (1, 45, 50, 16, 3, 1, 18), (2, 33, 31, 20, 3, 2, 1), (1, 34, 36, 8, 5, 2, 1)]


@pytest.mark.parametrize('layout', ['ld4', 'off4'])
@pytest.mark.parametrize('N,H,W,C,k,st,r', DW_CASES)
def test_dwconv_bf16_edges(ops, N, H, W, C, k, st, r, layout):
    """dl3p_dwconv2d_{fwd,bwd_data,bwd_weight}_bf16 and the slab form of the weight gradient on views beside canaries (NaN / +-Inf
    in the channels beside every view and in the rows after the last one): output canaries bit-identical, every element against
    float64 -- the forward with its statistics rows, the data gradient plain and accumulating, the weight gradient reduced and as
    slabs (NaN-filled workspace)"""
    L, s = ops.lib(), _s()
    Ho, Wo, pt, pl = ops.conv_geometry(H, W, k, st, r, 'same')
    g = _gen(H * W + C + k + r)
    x = torch.randn(N * H * W, C, device=DEV, generator=g).to(BF)
    w = (torch.randn(k, k, C, device=DEV, generator=g) / k).to(BF).contiguous()
    dy = torch.randn(N * Ho * Wo, C, device=DEV, generator=g).to(BF)
    old = torch.randn(N * H * W, C, device=DEV, generator=g).to(BF)
    sc, sh = coefs(g, C)
    a = pro(x, sc, sh, HSWISH).double().reshape(N, H, W, C)
    wd = w.double()
    geo = (st, r, pt, pl, Ho, Wo)
    X, DY = plane(x, layout), plane(dy, layout)
    # forward + statistics of the stored values
    want = _dw64(a, wd, *geo).reshape(-1, C)
    terms = _dw64(a.abs(), wd.abs(), *geo).reshape(-1, C)
    Y = out_plane(N * Ho * Wo, C, layout)
    part = torch.full((ops.MAX_STAT_ROWS * 2 * C,), float('nan'), dtype=torch.float32, device=DEV)
    rows = ctypes.c_int(0)
    L.dwconv2d_fwd_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, w.data_ptr(), Y.p, Y.ld, part.data_ptr(),
                        ctypes.byref(rows), N, H, W, C, k, st, r, pt, pl, Ho, Wo, s)
    close(Y.t, want, terms, 'dwconv fwd', k * k + 2)
    Y.intact('dwconv fwd')
    yq = Y.t.double()
    _rows_sum(part, rows.value, C, [(yq.sum(0), yq.abs().sum(0)), ((yq * yq).sum(0), (yq * yq).sum(0))], yq.shape[0],
              'dwconv fwd statistics')
    # data gradient, plain and accumulating
    dyd = dy.double().reshape(N, Ho, Wo, C)
    gx_want, gw_want = _dw_grads(a, wd, dyd, *geo)
    gx_terms, gw_terms = _dw_grads(a.abs(), wd.abs(), dyd.abs(), *geo)
    gx_want, gx_terms = gx_want.reshape(-1, C), gx_terms.reshape(-1, C)
    for acc in (0, 1):
        G = out_plane(N * H * W, C, layout, base=old if acc else None)
        L.dwconv2d_bwd_data_bf16(DY.p, DY.ld, w.data_ptr(), G.p, G.ld, acc, N, H, W, C, k, st, r, pt, pl, Ho, Wo, s)
        if acc:
            close(G.t, gx_want + old.double(), gx_terms + old.double().abs(), 'dwconv bwd_data accumulate', k * k + 3)
        else:
            close(G.t, gx_want, gx_terms, 'dwconv bwd_data', k * k + 2)
        G.intact('dwconv bwd_data')
    # weight gradient: reduced, and as slab rows
    need = L.dwconv2d_bwd_weight_workspace_bf16(N, Ho, Wo, C, k) // 4
    ws = torch.full((need,), float('nan'), dtype=torch.float32, device=DEV)
    gw = torch.full((k, k, C), float('nan'), dtype=torch.float32, device=DEV)
    L.dwconv2d_bwd_weight_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, DY.p, DY.ld, gw.data_ptr(), ws.data_ptr(),
                               need * 4, N, H, W, C, k, st, r, pt, pl, Ho, Wo, s)
    n = N * Ho * Wo + 2 * ops.MAX_STAT_ROWS
    assert bool(((gw.double() - gw_want).abs() <= n * U * gw_terms).all()), 'dwconv bwd_weight: worst %.3g' % float(
        (gw.double() - gw_want).abs().max())
    ws.fill_(float('nan'))
    rows = ctypes.c_int(0)
    L.dwconv2d_bwd_weight_slabs_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), HSWISH, DY.p, DY.ld, ws.data_ptr(), need * 4,
                                     ctypes.byref(rows), N, H, W, C, k, st, r, pt, pl, Ho, Wo, s)
    assert 0 < rows.value and rows.value * k * k * C <= need
    slab = ws[:rows.value * k * k * C].double().reshape(rows.value, k, k, C).sum(0)
    assert bool(((slab - gw_want).abs() <= n * U * gw_terms).all()), 'dwconv bwd_weight slabs'


def _im2col64(a, k, st, r, pt, pl, Ho, Wo):
    """float64 im2col of a (N, H, W, Cin) -> (N Ho Wo, k k Cin) in (ky, kx, ci) order, zero padding"""
    import torch.nn.functional as F
    N, H, W, Cin = a.shape
    ap = F.pad(a.permute(0, 3, 1, 2), _pad_for(H, W, k, st, r, pt, pl, Ho, Wo))
    Hp, Wp = ap.shape[2], ap.shape[3]
    keff = (k - 1) * r + 1
    col = F.unfold(ap, k, dilation=r, stride=st)
    col = col.reshape(N, Cin, k, k, (Hp - keff) // st + 1, (Wp - keff) // st + 1)[..., :Ho, :Wo]
    return col.permute(0, 4, 5, 2, 3, 1).reshape(N * Ho * Wo, k * k * Cin)


# (N, H, W, Cin, k, stride, rate): the RGB stem (Cin = 3), a strided 3x3, a dilated 3x3, a 7x7
IM2COL_CASES = [(2, 33, 31, 3, 3, 2, 1), (1, 20, 23, 12, 3, 1, 2), (2, 17, 19, 16, 3, 2, 1), (1, 12, 30, 4, 7, 2, 1)]


@pytest.mark.parametrize('N,H,W,Cin,k,st,r', IM2COL_CASES)
def test_im2col_col2im_bf16(ops, N, H, W, Cin, k, st, r):
    """dl3p_im2col_bf16 from a view beside canaries: bitwise Q(act(x*sc+sh)) or the padding zero in every column up to ld_col, the
    rows after the last one untouched; dl3p_col2im_bf16 (its transpose) into a view beside canaries, plain and accumulating, against
    float64"""
    L, s = ops.lib(), _s()
    Ho, Wo, pt, pl = ops.conv_geometry(H, W, k, st, r, 'same')
    M, kk = N * Ho * Wo, k * k * Cin
    ldc = (kk + 7) // 8 * 8 + 8
    g = _gen(H * W + Cin + k)
    x = torch.randn(N * H * W, Cin, device=DEV, generator=g).to(BF)
    sc, sh = coefs(g, Cin)
    X = Plane(N * H * W, Cin, ld=Cin + 5 if Cin % 4 else Cin + 4).set(x)
    COL = Plane(M, ldc, after=3)
    COL.keep = COL.bits.clone()
    L.im2col_bf16(X.p, X.ld, sc.data_ptr(), sh.data_ptr(), RELU6, COL.p, ldc, N, H, W, Cin, k, st, r, pt, pl, Ho, Wo, s)
    a = pro(x, sc, sh, RELU6).double().reshape(N, H, W, Cin)
    want = torch.zeros(M, ldc, dtype=torch.float64, device=DEV)
    want[:, :kk] = _im2col64(a, k, st, r, pt, pl, Ho, Wo)
    assert torch.equal(bits(COL.t), bits(want.to(BF))), 'im2col_bf16'
    COL.intact('im2col_bf16')
    if Cin % 4:
        return                                             # (col2im needs Cin % 4 == 0)
    gcol = torch.randn(M, ldc, device=DEV, generator=g).to(BF)
    GC = plane(gcol)
    old = torch.randn(N * H * W, Cin, device=DEV, generator=g).to(BF)
    ad = torch.zeros(N, H, W, Cin, dtype=torch.float64, device=DEV, requires_grad=True)
    _im2col64(ad, k, st, r, pt, pl, Ho, Wo).backward(gcol.double()[:, :kk])
    gx_want = ad.grad.reshape(-1, Cin)
    ad.grad = None
    _im2col64(ad, k, st, r, pt, pl, Ho, Wo).backward(gcol.double()[:, :kk].abs())
    gx_terms = ad.grad.reshape(-1, Cin)
    for acc in (0, 1):
        G = out_plane(N * H * W, Cin, 'ld4', base=old if acc else None)
        L.col2im_bf16(GC.p, ldc, G.p, G.ld, acc, N, H, W, Cin, k, st, r, pt, pl, Ho, Wo, s)
        if acc:
            close(G.t, gx_want + old.double(), gx_terms + old.double().abs(), 'col2im accumulate', k * k + 3)
        else:
            close(G.t, gx_want, gx_terms, 'col2im', k * k + 2)
        G.intact('col2im_bf16')
