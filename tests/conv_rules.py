"""The dense-conv kernels (csrc/pw_gemm_kernels.h GA, pw_wgrad_kernels.h GX, pw_split.hip GA / GX, stem.hip, conv.hip) in float64 with
per-element bounds, the host rules that route a launch restated in Python, the kernels' index arithmetic in numpy integers / float32,
and the case tables of tests/test_conv_rules_cpu.py and tests/test_conv_edges_gpu.py.

Reference.  a = act(x * scale + shift) in float64, padding applied to a (a tap outside the source contributes nothing, whatever
act(shift) is); forward y[m][co] = sum over taps inside and channels of a * w, weight gradient gw[k][co] = sum over rows whose tap
is inside of a * dy, data gradient gx[pixel][ci] = sum over the (tap, output pixel) pairs that reach the pixel and co of dy * w.
Every reference returns the value, the SUM OF THE MAGNITUDES OF ITS TERMS and the term count n per element.

Bounds.  No max|want| anywhere.
 * fp32 routes: |got - ref| <= (n + r + 1) U sum|terms|, U = 2^-24.  n products / adds in any order (MFMA chains, slabs, the slab
   reduction: a sum of n terms takes at most n roundings per term whatever its tree); r = the operand's own roundings on the way
   in: 1 for the prologue's fma, ACT_K[act] for the activation (ew_rules); + 1 for the bias add / the accumulate / second order.
   The magnitude of an operand element is |a| for none / ReLU / ReLU6 (the fma rounds ONCE relative to u, and a clamp is exact) and
   ew_rules.act_mag(|x scale| + |shift|) for the hard activations (their roundings are relative to the pieces of v * clamp(v + 3),
   not to the product).  A bias or an accumulate base is one more term of its own magnitude.
 * kinks: an element whose prologue argument lies within 2 U (|x scale| + |shift|) of a kink could take either branch.  inputs()
   asserts that their share is under KINK_SHARE_MAX and then moves those elements off the kink, so that no case has one.
 * split-bf16 routes: worst |got - ref| / sum|terms| below 1e-5 and below 3 x (the fp32 route's worst on the same launch) + 1e-7
   (tests/test_split_gemm_gpu.py::_elementwise_err).
 * statistic rows / bias gradients: (rows + n + 4) U sum|y| per column, from the device's own y."""
import collections
import zlib

import numpy as np
import torch

from ew_rules import (U, F, NONE, RELU, RELU6, HSWISH, HSIGMOID, KINKS, KINK_SHARE_MAX, ACT_K, act64, act32, act_mag, pro64,  # noqa: F401
                      fma32, D, Check, Plane, plane, out_plane, Vec, vec, ptr)

SB_ABS, SB_REL, SB_FLOOR = 1e-5, 3.0, 1e-7


# ------------------------------------------------------------------------------------------------ host rules (pwconv.hip, ops.py)
def cdiv(a, b):
    return -(-a // b)


def machine():
    """(DL3P_NUM_CUS, DL3P_MAX_STAT_ROWS) from where the library exposes them: dl3p_device_cus() and ops.MAX_STAT_ROWS"""
    from conftest import load_pkg
    return load_pkg('_lib').lib().device_cus(), load_pkg('ops').MAX_STAT_ROWS


def same_pad(n, k, s, r):
    ke = k + (k - 1) * (r - 1)
    out = cdiv(n, s)
    return out, max((out - 1) * s + ke - n, 0) // 2


def conv_geometry(H, W, k, s, r, pad):
    """ops.conv_geometry restated: 'same' | 'valid' | (pt, pb, pl, pr) -> Ho, Wo, pad_t, pad_l"""
    if pad == 'same':
        (Ho, pt), (Wo, pl) = same_pad(H, k, s, r), same_pad(W, k, s, r)
        return Ho, Wo, pt, pl
    pt, pb, pl, pr = (0, 0, 0, 0) if pad == 'valid' else pad
    ke = k + (k - 1) * (r - 1)
    return (H + pt + pb - ke) // s + 1, (W + pl + pr - ke) // s + 1, pt, pl


def pick_nt(N, M, cus):
    """pwconv.hip pick_nt (float32 costs, first strict minimum in the order 8 .. 1)"""
    ntiles, mt64 = cdiv(N, 16), cdiv(M, 64)
    small = mt64 * cdiv(ntiles, 8) <= 6 * cus
    best, best_cost = 1, F(1e30)
    for c in (8, 7, 6, 5, 4, 3, 2, 1):
        if c == 7 and not small:
            continue
        if small:
            cost = F(cdiv(mt64 * cdiv(ntiles, c), cus)) * (F(2) + F(c))
        else:
            cost = F(cdiv(ntiles, c) * c) * (F(1) + F(1.5) / F(c))
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def gemm_grid(nt, M, N, cus, max_rows, force_mi=0, force_pc=0):
    """pwconv.hip gemm_grid without the fused BatchNorm sums -> dict(nt, mi, gx, gy, m_tiles)"""
    nb = cdiv(N, 16 * nt)
    mi = 1 if cdiv(M, 128) * nb < 4 * cus else 2
    if M >= 60000 and nt >= 2:
        mi = 1
    per_cu = 6 if nt <= 1 else 5 if nt == 2 else 3 if nt <= 4 else 2
    if mi == 1:
        per_cu = max(per_cu, 3)
    if force_mi:
        mi = force_mi
        if mi == 1:
            per_cu = max(per_cu, 3)
    if force_pc:
        per_cu = force_pc
    mt = cdiv(M, 64 * mi)
    gx_max = min(max(cus * per_cu // nb, 8), max_rows)
    g = mt if mt <= gx_max else cdiv(mt, cdiv(mt, gx_max))
    return dict(nt=nt, mi=mi, gx=g, gy=nb, m_tiles=mt)


def plan_conv_gemm(M, N, cus, max_rows):
    """the fp32 implicit GEMMs: the heuristics only (no table, no pins)"""
    return gemm_grid(pick_nt(N, M, cus), M, N, cus, max_rows)


def plan_gemm_sb_ga(M, N, cus, max_rows, pin_nt=0, pin_mi=0, pin_pc=0):
    nt = min(pick_nt(N, M, cus), 8)
    if pin_nt:
        nt = min(pin_nt, 8)
    return gemm_grid(nt, M, N, cus, max_rows, pin_mi if pin_mi else (2 if M >= 4096 and nt < 6 else 1), pin_pc)


def conv_sb_supported(role, M, K, N, conv_sb=2, split_wgrad=1):
    if role not in (0, 1, 2, 4) or conv_sb == 0:
        return False
    if M < 1024 or K < 32 or N < 16 or K % 4 or N % 4 or K >= 65536:
        return False
    return (split_wgrad > 0 and N >= 32) if role == 4 else True


def trips(pl):
    """M tiles the busiest workgroup of a plan walks (the persistent loop's trip count)"""
    return cdiv(pl['m_tiles'], pl['gx'])


WGRAD_TILES = ((1, 4), (2, 4), (1, 8), (2, 8))                      # fp32 "wgrad_tile" 0 .. 3: (64 kw) x (16 nw)
SB_WGRAD_TILES = ((2, 8), (1, 8), (2, 4), (1, 4), (2, 16))          # "split_wgrad_tile" 0 .. 4: (64 kf) x (16 nw)


def _tile_cost(K, N, kw, nw):
    tk, tn = 64 * kw, 16 * nw
    area = F(cdiv(K, tk) * tk) * F(cdiv(N, tn) * tn)
    return area * (F(1) + F(0.5) * (F(64) / F(tk) + F(64) / F(tn)))


def wgrad_tiled_plan(M, K, N, cus, max_rows, tile=-1, per_cu=4):
    """pwconv.hip wgrad_tiled_plan for a shape the measured table does not know -> dict(tile, tiles, slabs, mchunk)"""
    pick = 0
    if tile >= 0 or M >= 65536:
        best = F(1e30)
        for i, (kw, nw) in enumerate(WGRAD_TILES):
            if tile >= 0 and i != tile:
                continue
            c = _tile_cost(K, N, kw, nw)
            if c < best:
                best, pick = c, i
    kw, nw = WGRAD_TILES[pick]
    tiles = cdiv(K, 64 * kw) * cdiv(N, 16 * nw)
    s = min(max(cus * per_cu // tiles, 1), cdiv(M, 256), max_rows)
    chunk = cdiv(cdiv(M, s), 32) * 32
    return dict(form=0, tile=pick, tiles=tiles, slabs=cdiv(M, chunk), mchunk=chunk)


def wgrad_sb_plan(M, K, N, cus, max_slabs, tile=-1, per_cu=0):
    """pw_split.hip dl3p_wgrad_sb_plan -> dict or None (shape not served)"""
    if M < 1024 or K < 32 or N < 32 or K % 4 or N % 4 or max_slabs < 1:
        return None
    best, pick = F(1e30), 3
    for i, (kf, nw) in enumerate(SB_WGRAD_TILES[:5 if tile == 4 else 4]):
        c = _tile_cost(K, N, kf, nw)
        if (tile < 0 and c < best) or tile == i:
            best, pick = c, i
    kf, nw = SB_WGRAD_TILES[pick]
    tiles = cdiv(K, 64 * kf) * cdiv(N, 16 * nw)
    if per_cu <= 0:
        per_cu = 2 if (kf, nw) == (2, 8) else 4
    s = min(max(cus * per_cu // tiles, 1), cdiv(M, 256), max_slabs)
    chunk = cdiv(cdiv(M, s), 32) * 32
    return dict(form=4, tile=pick, tiles=tiles, slabs=cdiv(M, chunk), mchunk=chunk)


def plan_conv_wgrad(M, K, N, cus, max_rows, conv_sb=1, tile=-1, sb_tile=-1):
    """dl3p_conv2d_gemm_bwd_weight with the workspace dl3p_conv2d_gemm_bwd_weight_workspace asks for: the workspace is sized from a
    first plan with room for DL3P_MAX_STAT_ROWS slabs, the launch plans again with what that workspace holds"""
    def pays():
        if not conv_sb_supported(4, M, K, N, conv_sb):
            return False
        return conv_sb == 2 or (M >= 4096 and M >= 8192 and K >= 128)

    def plan(max_slabs):
        t = wgrad_tiled_plan(M, K, N, cus, max_rows, tile)
        sb = wgrad_sb_plan(M, K, N, cus, min(max_slabs, max_rows), 0 if sb_tile == 4 else sb_tile) if pays() else None
        return t, sb
    t, sb = plan(max_rows)
    floats = max(max(t['slabs'], sb['slabs'] if sb else 0) * K * N, 512 * N)
    t, sb = plan(floats // (K * N))
    return sb if sb else t


# ---- stem.hip
STEM_TP = 64


def stem_segments(Wo):
    return cdiv(Wo, STEM_TP)


def stem_interior(H, W, pad_t, pad_l, oy, ox0):
    """the wave-uniform fast path: all three rows and all 129 columns of the tile inside the image (taken only with ldx == 3)"""
    ix0, iy0 = 2 * ox0 - pad_l, 2 * oy - pad_t
    return ix0 >= 0 and ix0 + 2 * STEM_TP < W and iy0 >= 0 and iy0 + 2 < H


def stem_interior_tiles(H, W, pad_t, pad_l, Ho, Wo):
    return sum(stem_interior(H, W, pad_t, pad_l, oy, 64 * sg) for oy in range(Ho) for sg in range(stem_segments(Wo)))


def stem_grid(tiles, per_cu, cus, max_rows, xcds=8):
    g = min(cdiv(cdiv(tiles, xcds), 4) * xcds, cus * per_cu)
    if g > max_rows:
        g = max_rows // xcds * xcds
    return max(g, xcds)


# ---- conv.hip
WCHUNK = 32


def wchunks(K):
    """the weight-gradient launches of the direct kernel: (first flat (tap, ci), how many)"""
    return [(e0, min(WCHUNK, K - e0)) for e0 in range(0, K, WCHUNK)]


def ld_col(K):
    return (K + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ index arithmetic (numpy)
def cmagic(C):
    return ((1 << 32) // C + 1) & 0xFFFFFFFF


def tap_of(kidx, C):
    """__umulhi(k, g_cmagic): claimed k // C for k < 2^16"""
    return ((np.asarray(kidx, np.uint64) * np.uint64(cmagic(C))) >> np.uint64(32)).astype(np.int64)


def kwmagic(k):
    return 65536 // k + 1


def ky_of(tap, k, magic=None):
    """(tap * g_kwmagic) >> 16: claimed tap // k for tap < 64"""
    return (np.asarray(tap, np.int32) * np.int32(kwmagic(k) if magic is None else magic)) >> 16


def parity_tap(ty, tx, shift, SH, SW):
    """the stride-2 data gradient's tap test on int32: -> (ok, sy, sx)"""
    ty, tx = np.asarray(ty, np.int32), np.asarray(tx, np.int32)
    par = np.int32((1 << shift) - 1)
    sy, sx = ty >> shift, tx >> shift
    return (ty >= 0) & (tx >= 0) & (((ty | tx) & par) == 0) & (sy < SH) & (sx < SW), sy, sx


def divmod_small(a, d, correct=True):
    """pw_wgrad_kernels.h divmod_small / pw_split.hip sb_divmod: one multiply by the float32 reciprocal, one correction step"""
    a = np.asarray(a, np.int32)
    inv = F(1) / F(d)
    q = (a.astype(F) * inv).astype(np.int32)
    rem = a - q * np.int32(d)
    if correct:
        lo = rem < 0
        q, rem = np.where(lo, q - 1, q), np.where(lo, rem + d, rem)
        hi = rem >= d
        q, rem = np.where(hi, q + 1, q), np.where(hi, rem - d, rem)
    return q, rem


# ------------------------------------------------------------------------------------------------ float64 references (torch)
Geo = collections.namedtuple('Geo', 'N H W k s r pt pl Ho Wo')


def geo_of(c):
    Ho, Wo, pt, pl = conv_geometry(c.H, c.W, c.k, c.s, c.r, c.pad)
    return Geo(c.N, c.H, c.W, c.k, c.s, c.r, pt, pl, Ho, Wo)


def tap_index(g, dev='cpu'):
    """-> pix (Ho*Wo, k*k) the source pixel of every (output pixel, tap), clamped into the image, and ok: the tap is inside"""
    ar = lambda n: torch.arange(n, device=dev)
    iy = ar(g.Ho)[:, None] * g.s - g.pt + ar(g.k)[None, :] * g.r
    ix = ar(g.Wo)[:, None] * g.s - g.pl + ar(g.k)[None, :] * g.r
    oky, okx = (iy >= 0) & (iy < g.H), (ix >= 0) & (ix < g.W)
    pix = iy.clamp(0, g.H - 1)[:, None, :, None] * g.W + ix.clamp(0, g.W - 1)[None, :, None, :]
    ok = oky[:, None, :, None] & okx[None, :, None, :]
    return pix.reshape(g.Ho * g.Wo, g.k * g.k), ok.reshape(g.Ho * g.Wo, g.k * g.k)


def patches(a, g):
    """a (N*H*W, C) -> (N*Ho*Wo, k*k, C), zero where the tap is outside"""
    pix, ok = tap_index(g, a.device)
    P = a.reshape(g.N, g.H * g.W, -1)[:, pix]                       # (N, Ho*Wo, kk, C)
    return torch.where(ok[None, :, :, None], P, torch.zeros((), dtype=a.dtype, device=a.device)).reshape(g.N * g.Ho * g.Wo, g.k * g.k, -1)


def prologue64(x, sc, sh, act):
    """-> a = act(x sc + sh), the magnitude A of an operand element (module docstring), r = its roundings, u and T for the kinks"""
    u, T, r = pro64(x, sc, sh)
    a = act64(u, act)
    A = a.abs() if act in (NONE, RELU, RELU6) else act_mag(T, act)
    return a, A, r + ACT_K[act], u, T


def fwd_ref(x, w, g, sc=None, sh=None, act=NONE, bias=None):
    """x (N*H*W, Cin), w (k*k*Cin, Cout) float64 -> Check over (N*Ho*Wo, Cout), worst-case |err| / sum|terms| helper fields"""
    a, A, r, _, _ = prologue64(x, sc, sh, act)
    K = w.shape[0]
    P, PA = patches(a, g).reshape(-1, K), patches(A, g).reshape(-1, K)
    y, mag = P @ w, PA @ w.abs()
    n = tap_index(g, x.device)[1].sum(1).repeat(g.N)[:, None].double() * x.shape[1]
    if bias is not None:
        y, mag, n = y + bias, mag + bias.abs(), n + 1
    return Bounded(y, mag, n, r)


def wgrad_ref(x, dy, g, sc=None, sh=None, act=NONE):
    """-> Check over (k*k*Cin, Cout)"""
    a, A, r, _, _ = prologue64(x, sc, sh, act)
    C = x.shape[1]
    P, PA = patches(a, g).reshape(-1, g.k * g.k * C), patches(A, g).reshape(-1, g.k * g.k * C)
    gw, mag = P.t() @ dy, PA.t() @ dy.abs()
    n = (tap_index(g, x.device)[1].sum(0) * g.N).repeat_interleave(C)[:, None].double()
    return Bounded(gw, mag, n, r)


def dgrad_ref(dy, w, g, Cin, base=None):
    """dy (N*Ho*Wo, Cout), w (k*k*Cin, Cout) -> Check over (N*H*W, Cin) and `reached` (N*H*W,): some tap reaches the input pixel"""
    pix, ok = tap_index(g, dy.device)
    kk, Cout = g.k * g.k, dy.shape[1]
    w3 = w.reshape(kk, Cin, Cout)
    G = torch.einsum('mo,tco->mtc', dy, w3)                          # (M, kk, Cin)
    GA = torch.einsum('mo,tco->mtc', dy.abs(), w3.abs())
    dst = (torch.arange(g.N, device=dy.device)[:, None, None] * (g.H * g.W) + pix[None]).reshape(-1)
    okf = ok[None].expand(g.N, -1, -1).reshape(-1)
    gx = torch.zeros(g.N * g.H * g.W, Cin, dtype=torch.float64, device=dy.device)
    mag, cnt = torch.zeros_like(gx), torch.zeros(g.N * g.H * g.W, dtype=torch.float64, device=dy.device)
    gx.index_add_(0, dst[okf], G.reshape(-1, Cin)[okf])
    mag.index_add_(0, dst[okf], GA.reshape(-1, Cin)[okf])
    cnt.index_add_(0, dst[okf], torch.ones_like(dst[okf], dtype=torch.float64))
    n = cnt[:, None] * Cout
    if base is not None:
        gx, mag, n = gx + base, mag + base.abs(), n + 1
    b = Bounded(gx, mag, n, 0)
    b.reached = cnt > 0
    return b


class Bounded(Check):
    """a float64 reference with sum|terms|, the term count and the fp32 bound (n + r + 1) U sum|terms| per element"""

    def __init__(self, ref, mag, n, r):
        super().__init__(ref, (n + r + 1) * U * mag)
        self.mag, self.n, self.r = mag, n, r

    def rel(self, got):
        """worst |got - ref| / sum|terms| (the split routes' figure); an element without terms must be exactly zero"""
        err = (got.double().reshape(self.ref.shape) - self.ref).abs()
        return float(torch.where(self.mag > 0, err / self.mag.clamp_min(1e-300), torch.where(err == 0, err, err + float('inf'))).max())


def stat_check(y, rows):
    """the statistic rows (sum y, sum y^2) of a device output y (M, C): Checks with (rows + M + 4) U sum|y| per column"""
    y = y.double()
    k = (rows + y.shape[0] + 4) * U
    return Check(y.sum(0), k * y.abs().sum(0)), Check((y * y).sum(0), k * (y * y).sum(0))


def colsum_check(dy, rows=512):
    """the bias gradient: column sums of dy through at most `rows` partial rows"""
    dy = dy.double()
    return Check(dy.sum(0), (rows + dy.shape[0] + 4) * U * dy.abs().sum(0))


# ------------------------------------------------------------------------------------------------ inputs
def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def signed(r, shape, lo=0.25, hi=1.0):
    """|v| in [lo, hi) with a random sign: no term of a sum is small against the others, so one dropped or doubled tap moves an
    element by ~1 / n of its sum|terms| -- thousands of times its bound"""
    return (r.uniform(lo, hi, shape) * r.choice([-1.0, 1.0], shape)).astype(F)


PRO = {                      # prologues by name: (act, scale range, shift range); act(shift) != 0 on every channel for the 'pos' ones
    'none': None,
    'relu_pos': (RELU, (0.5, 1.5), (0.25, 0.75)),
    'relu6_pos': (RELU6, (2.0, 5.0), (0.5, 1.5)),
    'hswish': (HSWISH, (1.0, 3.0), (0.5, 1.5)),
    'affine': (NONE, (0.5, 1.5), (-0.5, 0.5)),
}


def prologue_of(name, C, r):
    if PRO[name] is None:
        return None, None, NONE
    act, (s0, s1), (h0, h1) = PRO[name]
    return r.uniform(s0, s1, C).astype(F), r.uniform(h0, h1, C).astype(F), act


def off_kinks(x, sc, sh, act):
    """assert the share of elements within 2 U T of a kink, then move them away -> x with none"""
    if sc is None or not KINKS[act]:
        return x
    for it in range(4):
        u = x.astype(np.float64) * sc + sh
        T = np.abs(x.astype(np.float64) * sc) + np.abs(sh.astype(np.float64))
        near = np.zeros(x.shape, bool)
        for kink in KINKS[act]:
            near |= np.abs(u - kink) <= 2 * U * T
        if it == 0:
            assert near.mean() <= KINK_SHARE_MAX, near.mean()
        if not near.any():
            return x
        x = np.where(near, x + F(0.0625), x).astype(F)
    raise AssertionError('elements stay on a kink')


def conv_inputs(c):
    """float32 operands of a GEMM-family case (numpy): x (N*H*W, Cin), w (k*k*Cin, Cout), dy (N*Ho*Wo, Cout), sc / sh, bias, the base"""
    r, g = rng_of(c.name), geo_of(c)
    sc, sh, act = prologue_of(c.pro, c.Cin, r)
    x = off_kinks(signed(r, (c.N * c.H * c.W, c.Cin), 0.25, 2.0), sc, sh, act)
    return dict(x=x, w=signed(r, (c.k * c.k * c.Cin, c.Cout)), dy=signed(r, (c.N * g.Ho * g.Wo, c.Cout)), sc=sc, sh=sh, act=act,
                bias=signed(r, (c.Cout,)),
                xbase=signed(r, (c.N * c.H * c.W, c.Cin), 64.0, 256.0))


# ------------------------------------------------------------------------------------------------ fp32 emulation (numpy)
def pro32(x, sc, sh, act):
    return act32(x if sc is None else fma32(x, sc, sh), act)


def patches32(a, g):
    pix, ok = (t.numpy() for t in tap_index(g))
    P = a.reshape(g.N, g.H * g.W, -1)[:, pix]
    return np.where(ok[None, :, :, None], P, F(0)).reshape(g.N * g.Ho * g.Wo, -1)


def sum32(terms, order):
    """fp32 sum over axis 0 of float32 terms: order 0 strictly sequential (cumsum), order 1 numpy's pairwise sum of the reversed list"""
    if order == 0:
        return np.cumsum(terms, axis=0, dtype=F)[-1]
    return terms[::-1].sum(axis=0, dtype=F)


def matmul32(A, B, order, cols=None):
    """A (M, K) x B (K, N) with every product rounded to float32 and the sum in float32 in `order`"""
    B = B if cols is None else B[:, cols]
    out = np.empty((A.shape[0], B.shape[1]), F)
    step = max(1, (1 << 24) // max(1, A.shape[1] * B.shape[1]))
    for m0 in range(0, A.shape[0], step):
        t = A[m0:m0 + step, :, None] * B[None, :, :]                 # float32 products
        out[m0:m0 + step] = sum32(np.moveaxis(t, 1, 0), order)
    return out


# ------------------------------------------------------------------------------------------------ the case tables
# GEMM family (forward and data gradient of dl3p_conv2d_gemm_*).  pad: 'same' | 'valid' | (pt, pb, pl, pr).  pro: a key of PRO.
# want: what dl3p_conv2d_gemm_plan_query must report for the forward GEMM (M = N Ho Wo, N = Cout) under `f` and for the data
# gradient (M = N H W, N = Cin) under `d`, as (nt, mi, trips); None: not asserted.  The split twins run wherever
# conv_sb_supported admits the GEMM with conv_sb = 2 (split_cases below).
G = collections.namedtuple('G', 'name N H W Cin Cout k s r pad pro edge f d')


def _g(name, N, H, W, Cin, Cout, k, s=1, r=1, pad='same', pro='none', edge='', f=None, d=None):
    return G(name, N, H, W, Cin, Cout, k, s, r, pad, pro, edge, f, d)


GEMM = [
    # ---- row decode: two integer divisions per M tile, rows past M, tiles that span images
    _g('m1', 1, 1, 1, 4, 4, 3, edge='M = 1: one live row in the tile, only the centre tap inside', f=(1, 1, 1), d=(1, 1, 1)),
    _g('map_2x3', 3, 2, 3, 4, 12, 3, edge='Ho, Wo = 2, 3: every pixel on a border', f=(1, 1, 1), d=(1, 1, 1)),
    _g('map_5x7_span', 3, 5, 7, 12, 4, 3, pro='relu_pos', edge='35 pixels per image: the first 64-row tile spans two images',
       f=(1, 1, 1), d=(1, 1, 1)),
    _g('m63', 1, 7, 9, 4, 20, 3, edge='M % 64 = 63', f=(1, 1, 1), d=(1, 1, 1)),
    _g('m64', 1, 8, 8, 4, 4, 3, edge='M % 64 = 0: no row past M', f=(1, 1, 1), d=(1, 1, 1)),
    _g('m65', 1, 5, 13, 4, 4, 3, edge='M % 64 = 1: a second tile with one live row', f=(1, 1, 1), d=(1, 1, 1)),
    _g('sb_m1024', 1, 32, 32, 36, 36, 1, pro='relu6_pos', edge='split: the smallest M served, M % 64 = 0, K = 36 (K % 8 = 4)',
       f=(1, 1, 1), d=(1, 1, 1)),
    _g('sb_m1025', 1, 25, 41, 20, 16, 3, edge='split: M % 64 = 1, K = 180 (K % 8 = 4) forward', f=(1, 1, 1), d=(1, 1, 1)),
    _g('sb_m1087', 1, 1, 1087, 16, 20, 3, pro='relu_pos', edge='split: M % 64 = 63, a one-row map (top and bottom taps outside); data gradient K % 8 = 4',
       f=(1, 1, 1), d=(1, 1, 1)),
    # ---- persistent loop and tile height
    _g('trips_fwd', 1, 56, 56, 4, 2048, 1, edge='forward: 26 column blocks, gx_max = 29 < 49 M tiles: a second trip (default plan)',
       f=(5, 1, 2), d=(1, 1, 1)),
    _g('trips_dgrad', 1, 56, 56, 2048, 4, 1, edge='data gradient: the same second trip over input pixels', f=(1, 1, 1), d=(5, 1, 2)),
    _g('trips_3x3', 3, 33, 33, 4, 2048, 3, pro='relu_pos', edge='second trip with a 3 x 3 gather: the row decode runs again',
       f=(7, 1, 2), d=(1, 1, 1)),
    _g('mi2', 2, 256, 256, 4, 4, 3, edge='131072 rows at one column block: the smallest M with 128-row tiles (MI = 2)',
       f=(1, 2, 1), d=(1, 2, 1)),
    _g('mi2_trips', 1, 82, 100, 4, 2048, 1, edge='MI = 2 and three trips: 65 tiles of 128 rows over 16 column blocks',
       f=(8, 2, 3), d=(1, 1, 1)),
    # ---- K decode: umulhi by g_cmagic, (tap * g_kwmagic) >> 16, the K tail of the last 32-wide step
    _g('k4', 2, 5, 5, 4, 12, 1, edge='K = 4: the clamp min(k, K - 4) is 0', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k2_c4', 2, 6, 5, 4, 8, 2, edge='k = 2 (even kernel under same), K = 16', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k4_c4', 2, 7, 6, 4, 8, 4, pro='relu_pos', edge='k = 4 (even kernel under same), K % 32 = 0', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k3_c12', 2, 5, 6, 12, 8, 3, edge='Cin = 12: K = 108, K % 32 = 12', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k3_c20', 2, 5, 6, 20, 8, 3, pro='hswish', edge='Cin = 20: K = 180', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k3_c28', 2, 5, 6, 28, 8, 3, edge='K = 252, K % 32 = 28', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k3_c36', 2, 5, 6, 36, 8, 3, edge='Cin = 36: K = 324, K % 32 = 4', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k5_c4', 2, 7, 7, 4, 8, 5, pro='relu6_pos', edge='k = 5: taps up to 24, K = 100', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k7_c4', 2, 9, 8, 4, 8, 7, edge='k = 7: taps up to 48 (the (tap * magic) >> 16 rule at its largest)', f=(1, 1, 1), d=(1, 1, 1)),
    _g('k7_c1336', 2, 3, 3, 1336, 16, 7, edge='K = 65464, the largest admitted: k indices up to 2^16', f=(1, 1, 1), d=(1, 1, 1)),
    _g('sb_k3_c20', 2, 23, 23, 20, 36, 3, pro='relu_pos', edge='split: K = 180, K % 8 = 4; data gradient K = 324, K % 8 = 4', f=(1, 1, 1),
       d=(1, 1, 1)),
    # ---- padding
    _g('rate_ge_h', 2, 3, 3, 4, 8, 3, r=3, pro='relu_pos', edge='rate >= H: only the centre tap is inside', f=(1, 1, 1), d=(1, 1, 1)),
    _g('rate2_ge_h', 2, 5, 4, 4, 8, 3, r=3, pro='hswish', edge='2 rate >= H: no pixel sees both outer taps', f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_0101_even', 2, 8, 6, 4, 8, 3, s=2, pad=(0, 1, 0, 1), pro='relu6_pos', edge='(0,1,0,1) at stride 2, even size',
       f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_0101_odd', 2, 7, 9, 4, 8, 3, s=2, pad=(0, 1, 0, 1), edge='(0,1,0,1) at stride 2, odd size; ty < 0 at the top-left corner',
       f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_1111_even', 2, 8, 6, 4, 8, 3, s=2, pad=(1, 1, 1, 1), pro='relu_pos', edge='(1,1,1,1) at stride 2, even size',
       f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_1111_odd', 2, 7, 9, 4, 8, 3, s=2, pad=(1, 1, 1, 1), edge='(1,1,1,1) at stride 2, odd size', f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_same_even', 2, 8, 8, 4, 8, 3, s=2, edge='same at stride 2, even size: pad_t = 0', f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_same_odd', 2, 9, 7, 4, 8, 3, s=2, pro='hswish', edge='same at stride 2, odd size: pad_t = 1', f=(1, 1, 1), d=(1, 1, 1)),
    # ---- stride-2 data gradient: the parity mask and ty >> 1
    _g('s2_k1', 2, 7, 6, 4, 8, 1, s=2, edge='stride 2, k = 1: three input pixels in four have no tap', f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_k2', 2, 8, 6, 4, 8, 2, s=2, edge='stride 2, k = 2: exactly one tap per input pixel', f=(1, 1, 1), d=(1, 1, 1)),
    _g('s2_r2', 2, 9, 10, 4, 8, 3, s=2, r=2, edge='stride 2 with rate 2: odd rows and columns have no tap at all', f=(1, 1, 1),
       d=(1, 1, 1)),
    _g('sb_s2', 1, 40, 40, 36, 36, 3, s=2, edge='split data gradient at stride 2 (M = 1600 input pixels)', f=None, d=(1, 1, 1)),
] + [
    # ---- N tail and the column-block width: 129 .. 132 row tiles of 64, the small-grid regime of pick_nt
    _g('ntail_%s%d' % ('f' if fwd else 'd', c), 3, 53, 53, 4 if fwd else c, c if fwd else 4, 3, pro='relu_pos' if c == 100 else 'none',
       edge='%s onto %d columns: nt = %d, %d live columns in the last 16' % ('forward' if fwd else 'data gradient', c, nt, c % 16 or 16),
       f=(nt, 1, 1) if fwd else (1, 1, 1), d=(1, 1, 1) if fwd else (nt, 1, 1))
    for c, nt, fwd in ((4, 1, True), (12, 1, True), (12, 1, False), (20, 2, True), (20, 2, False), (36, 3, True), (36, 3, False), (52, 4, True),
                       (68, 5, False), (84, 6, True), (100, 7, True), (100, 7, False), (116, 8, False), (132, 3, True), (132, 3, False))
]


def gemm_shapes(c):
    """(M, K, N) of the forward and of the data-gradient GEMM of a case"""
    g = geo_of(c)
    return (c.N * g.Ho * g.Wo, c.k * c.k * c.Cin, c.Cout), (c.N * c.H * c.W, c.k * c.k * c.Cout, c.Cin)


def split_cases():
    """[(case, role 0 | 2, (M, K, N))] of every GEMM of the table the split kernels serve with conv_sb = 2: all of them run split"""
    return [(c, role, mkn) for c in GEMM for role, mkn in zip((0, 2), gemm_shapes(c))
            if (role == 2 or c.f is not None) and conv_sb_supported(role, *mkn)]


# Weight gradients (dl3p_conv2d_gemm_bwd_weight).  tile: "wgrad_tile" pin (-1 none); sb: "split_wgrad_tile" pin with conv_sb = 2
# (None: the fp32 kernel, conv_sb = 0).  want: (form, tile index, k tiles x n tiles, slabs) as the query reports them.
Wg = collections.namedtuple('Wg', 'name N H W Cin Cout k s r pad pro tile sb edge want')


def _w(name, N, H, W, Cin, Cout, k, s=1, r=1, pad='same', pro='none', tile=-1, sb=None, edge='', want=None):
    return Wg(name, N, H, W, Cin, Cout, k, s, r, pad, pro, tile, sb, edge, want)


WGRAD = [
    _w('w_1x1', 4, 1, 1, 4, 4, 3, edge='Ho = Wo = 1, M = 4: every divisor of the row decode is 1', want=(0, 0, 1, 1)),
    _w('w_3x5', 5, 3, 5, 4, 36, 3, pro='relu_pos', edge='Wo = 5, Ho = 3; act(shift) != 0 on the padded taps', want=(0, 0, 1, 1)),
    _w('w_m65', 1, 5, 13, 12, 4, 3, edge='M % 32 = 1: a last step with one live row', want=(0, 0, 2, 1)),
    _w('w_7x7', 3, 7, 7, 4, 4, 3, pro='hswish', edge='Ho = Wo = 7: three images inside five steps of 32 rows', want=(0, 0, 1, 1)),
    _w('w_5x3', 5, 5, 3, 4, 4, 2, edge='Wo = 3, Ho = 5 under an even kernel', want=(0, 0, 1, 1)),
    _w('w_127x129', 1, 127, 129, 4, 68, 3, tile=1, edge='Wo = 129, Ho = 127, M % 32 = 31; 128 x 64 tile with Cout % 64 = 4',
       want=(0, 1, 2, 64)),
    _w('w_129x127', 1, 129, 127, 20, 132, 3, tile=3, pro='hswish', edge='Wo = 127, Ho = 129; 128 x 128 tile, K = 180, Cout % 128 = 4',
       want=(0, 3, 4, 64)),
    _w('w_slabs', 2, 17, 19, 4, 36, 3, tile=0, edge='three slabs of 224 rows: boundaries inside an image row (19 pixels)',
       want=(0, 0, 1, 3)),
    _w('w_tile2', 2, 17, 19, 20, 132, 3, tile=2, pro='relu6_pos', edge='64 x 128 tile: K % 64 = 52, Cout % 128 = 4', want=(0, 2, 6, 3)),
    _w('w_s2', 3, 9, 11, 4, 36, 3, s=2, pad=(0, 1, 0, 1), edge='stride 2 with (0,1,0,1): g_mul = 2 in the gather', want=(0, 0, 1, 1)),
    _w('w_r2_k5', 2, 9, 8, 4, 36, 5, r=2, edge='k = 5 at rate 2: taps 8 pixels out', want=(0, 0, 2, 1)),
    _w('w_wo41', 2, 3, 41, 4, 36, 3, pro='relu_pos', edge='Wo = 41: float32(a) * float32(1 / 41) truncates one short at a = 41, 82, 164: the correction step of divmod_small',
       want=(0, 0, 1, 1)),
    _w('w_big', 11156, 2, 47, 4, 32, 3, edge='1048664 rows, Wo = 47 (prime; 30851 row indices need the correction step), 94 pixels per image',
       want=(0, 0, 1, 994)),
] + [
    _w('w_sb%d' % t, 2, 23, 29, 12, co, 3, pro='relu_pos' if t == 1 else 'none', sb=t,
       edge='split tile setting %d at M = 1334, K = 108 (K %% 8 = 4), Cout = %d%s' % (t, co, ': plans as 0' if t == 4 else ''), want=(4, t % 4, 2, 6))
    for t, co in ((0, 132), (1, 36), (2, 68), (3, 32), (4, 132))
]

# The stem (dl3p_stem_conv_fwd / _bwd_weight / _bwd_weight_slabs_bn): 3 x 3, stride 2, Cin = 3.  interior: how many (row, segment)
# tiles of one image take the fast path when the input is packed (ldx = 3)
St = collections.namedtuple('St', 'name N H W Cout pad edge interior')
STEM = [
    St('st_w128', 1, 4, 128, 16, 'same', 'pad_l = 0, W = 128: ix0 + 128 = W, the last column is padding: general path', 0),
    St('st_w129', 1, 4, 129, 16, (0, 1, 0, 1), 'pad_l = 0, W = 129: the first W whose segment 0 is interior (Wo = 64)', 1),
    St('st_w130', 2, 4, 130, 32, 'same', 'pad_l = 0, W = 130: interior, and a second segment of one pixel (Wo = 65)', 1),
    St('st_w255', 1, 4, 255, 16, (1, 1, 1, 1), 'pad_l = 1, W = 255: segment 1 starts at column 127 and ends on the padding', 0),
    St('st_w256', 1, 4, 256, 32, (1, 1, 1, 1), 'pad_l = 1, W = 256: segment 1 is interior on the middle row', 1),
    St('st_w257', 3, 4, 257, 16, 'same', 'pad_l = 1, W = 257: Wo = 129, a third segment of one pixel; 18 tiles (not 4 n)', 1),
    St('st_w258', 1, 2, 258, 16, (1, 1, 1, 1), 'pad_l = 1, W = 258, H = 2: no row has three rows inside', 0),
    St('st_wo1', 3, 2, 1, 32, 'same', 'Wo = 1, H = 2', 0),
    St('st_wo63', 1, 3, 126, 16, 'same', 'Wo = 63: one short segment', 0),
    St('st_h6_w260', 2, 6, 260, 32, (0, 1, 0, 1), 'pad 0: two interior rows x two interior segments (Wo = 130, a third of two pixels)', 4),
]

# conv.hip: the direct kernels and im2col / col2im
Dc = collections.namedtuple('Dc', 'name N H W Cin Cout k s r pad pro edge')
DIRECT = [
    Dc('d_k3_c3', 2, 9, 8, 3, 16, 3, 2, 1, 'same', 'none', 'Cin = 3, k = 3, stride 2: K = 27, one WCHUNK launch, patch row padded to 28'),
    Dc('d_k7_c3', 2, 11, 9, 3, 64, 7, 2, 1, 'same', 'affine', 'Cin = 3, k = 7: K = 147, five WCHUNK launches (last 19), patch row padded to 148'),
    Dc('d_k3_c4', 2, 7, 6, 4, 4, 3, 2, 2, 'same', 'relu_pos', 'Cin = 4 at stride 2 and rate 2: col2im with parity gaps'),
    Dc('d_k3_s2', 2, 8, 7, 4, 16, 3, 2, 1, (0, 1, 0, 1), 'none', 'Cin = 4, stride 2, (0,1,0,1): col2im at stride 2'),
]
