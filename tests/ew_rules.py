"""Rules shared by tests/test_ew_edges_gpu.py (the fp32 BatchNorm / elementwise / pooling / resize kernels on the device) and its CPU
companion tests/test_ew_rules_cpu.py: the lane plans restated, the seeded inputs, the float64 references with their PER-ELEMENT
bounds, an op-for-op float32 emulation of every kernel expression, and the canary planes.

Bound rule.  |got - ref| <= k * U * terms with U = 2^-24: `terms` is the sum of the magnitudes of the terms that formed the element
(every term of the cancelling forms, not the result) and k is the number of fp32 roundings on the element's path as the kernel
writes it, plus one; the count stands beside each op below.  fp32 reductions of n terms delivered in `rows` partial rows get
(n + rows + 4) * U * sum|terms|.  Sums that the kernels accumulate in double get rows * 2^-53 * sum|x| (plus the fp32 roundings
behind them).  There is no tensor-scale (max|want|) term anywhere: a wrong lane, a dropped row or a lost accumulate fails at any
magnitude.

Activation kinks.  The reference forms the prologue u = z * scale + shift in float64; an element whose u lies within
2 U (|z * scale| + |shift|) of a kink (0 for ReLU, 0 and 6 for ReLU6, -3 and +3 for h-swish and h-sigmoid) may match the branch on
either side.  The share of such elements is a condition on the inputs (KINK_SHARE_MAX), asserted in both test files.

References and bounds are torch float64 and run wherever their inputs live (the device in the GPU file, the CPU in the companion);
inputs and the fp32 emulation are numpy."""
import math

import numpy as np
import torch

U = 2.0 ** -24                      # one fp32 rounding, relative
UD = 2.0 ** -53                     # one double rounding, relative
NONE, RELU, RELU6, HSWISH, HSIGMOID = 0, 1, 2, 3, 4
ACTS = (NONE, RELU, RELU6, HSWISH, HSIGMOID)
KINKS = {NONE: (), RELU: (0.0,), RELU6: (0.0, 6.0), HSWISH: (-3.0, 3.0), HSIGMOID: (-3.0, 3.0)}
KINK_SHARE_MAX = 1e-3
F = np.float32
SIXTH32 = F(1.0) / F(6.0)
MAX_STAT_ROWS = 2048
NUM_CUS = 256
LAYOUTS = ('contig', 'ld4', 'off4')
RATE, SEED = 0.3, 0x5EED
# canary fp32 bit patterns: a NaN with a payload, +Inf, -Inf
CANARY = (0x7FA5A5A5, 0x7F800000, 0xFF800000 - (1 << 32))

# C -> (c4s, px, nslab) of pick_lanes, with the reason each width is in the list
LANE_PLANS = {
    4: (1, 256, 1),        # one float4 per pixel: 256 pixel lanes
    12: (3, 85, 1),        # 255 of 256 threads busy (one idle lane)
    20: (5, 51, 1),        # 255 busy
    36: (9, 28, 1),        # 252 busy
    72: (18, 14, 1),       # 252 busy
    120: (30, 8, 1),       # 240 busy: the MobileNetV3 expand width
    268: (67, 3, 1),       # 201 busy: a prime number of float4s below 256
    672: (84, 3, 2),       # two slabs AND idle lanes (MobileNetV3)
    960: (240, 1, 1),      # px = 1: a workgroup is one pixel, 240 busy
    1028: (1, 256, 257),   # 257 float4s (prime above 256): c4s = 1, 257 slabs
    1280: (64, 4, 5),      # five slabs (MobileNetV2 head)
    2048: (256, 1, 2),     # px = 1 with two slabs (ResNet-50)
}
CS = tuple(LANE_PLANS)


# ------------------------------------------------------------------------------------------------ the plans, restated
def pick_lanes(C):
    """csrc/common.h pick_lanes: (c4s, px, nslab)"""
    c4 = C // 4
    best, best_used = 1, 0
    for d in range(1, min(c4, 256) + 1):
        if c4 % d:
            continue
        if d < 32 and d < c4:
            continue
        used = (256 // d) * d
        if used > best_used or (used == best_used and d > best):
            best, best_used = d, used
    return best, 256 // best, c4 // best


def ew_nbx(M, C, max_rows=1 << 20, per_cu=4):
    """ew_setup: workgroups per channel slab (= partial rows of bn_bwd_reduce)"""
    c4s, px, nslab = pick_lanes(C)
    need = -(-M // px)
    target = max(1, NUM_CUS * per_cu // nslab)
    return max(1, min(need, target, max_rows))


def pool_plan(N, HW, C, chunked, want=512):
    """bn_elementwise.hip pool_plan: dict(c4s, px, nslab, nchunk, per, ticket_floats)"""
    c4 = C // 4
    d = 1
    for k in range(1, min(64 if chunked else 16, c4) + 1):
        if c4 % k == 0:
            d = k
    px, nslab = 256 // d, c4 // d
    nchunk = 1
    if chunked:
        nchunk = (want + N * nslab - 1) // (N * nslab)
        nchunk = max(1, min(nchunk, (HW + 4 * px - 1) // (4 * px), 64))
    per = (HW + nchunk - 1) // nchunk
    return dict(c4s=d, px=px, nslab=nslab, nchunk=(HW + per - 1) // per, per=per,
                ticket_floats=((N * nslab + 63) // 64) * 64)


def pool_workspace_floats(N, HW, C):
    pl = pool_plan(N, HW, C, True)
    return pl['ticket_floats'] + N * pl['nchunk'] * C


def gap_fwd_chunks(N, HW, C, workspace):
    """does dl3p_global_avgpool_fwd take the chunked plan?"""
    return bool(workspace) and N * pool_plan(N, HW, C, False)['nslab'] < NUM_CUS // 4


def resize_fwd_path(w, W, C):
    """'seg16' / 'seg8' (the strip kernels) or 'pixel'"""
    if W >= 2 * w and C % 256 == 0:
        return 'seg16' if (15 * w) // W <= 3 else 'seg8'
    return 'pixel'


def touch_range(i, inv_scale, out_size):
    a = (F(i) - F(0.5)) * F(inv_scale) - F(0.5)
    b = (F(i) + F(1.5)) * F(inv_scale) - F(0.5)
    return max(int(math.floor(a)) - 1, 0), min(int(math.ceil(b)) + 1, out_size - 1)


def resize_bwd_windows(w, W):
    """the set of windows resize_bwd_kernel takes over the input columns: 'tight' (RB_TIGHT), 'maxw' (RB_MAXW), 'general'"""
    isx = F(W) / F(w)
    out = set()
    for ix in range(w):
        x0, x1 = touch_range(ix, isx, W)
        if ix == 0:
            x0 = 0
        if ix == w - 1:
            x1 = W - 1
        if F(2.0) * isx < F(8.0) and x1 - x0 < 12:
            out.add('tight')          # (the kernel's own escape from it never fires at these scales)
        elif x1 - x0 < 12:
            out.add('maxw')
        else:
            out.add('general')
    return out


# ------------------------------------------------------------------------------------------------ the cases
def lane_rows(C):
    """M of the lane-plan walkers: 1, px - 1, px, px + 1 and one M at which the grid-stride loop takes a second trip on three lanes"""
    c4s, px, nslab = pick_lanes(C)
    small = sorted({m for m in (1, px - 1, px, px + 1) if m >= 1})
    return small, (1024 // nslab) * px + 3


def lane_cases():
    """(C, M, layouts, act, ract, nulls, big): each operand of a case on a different layout, the options rotating with the case"""
    i = 0
    for C in CS:
        small, big = lane_rows(C)
        for M in small + [big]:
            rot = i % 3
            yield dict(C=C, M=M, lay=LAYOUTS[rot:] + LAYOUTS[:rot], act=ACTS[i % 5], ract=ACTS[(i // 5 + 2) % 5], nulls=i % 4,
                       big=M == big)
            i += 1


def split_rows(M):
    """(N, HW) with N * HW == M for global_avgpool_bwd"""
    for n in (3, 2):
        if M % n == 0 and M > n:
            return n, M // n
    return 1, M


FIN_ROWS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 640, 2048)
FIN_CS = (4, 16, 20, 36)
PART_ROWS, PART_C2 = (1, 64, 65, 128, 129, 200), (8, 24, 40)
RR_WIDE = [(r, n) for r in (1, 4, 5, 15, 16) for n in (1, 63, 65, 257)] + [(17, 65537)]
RR_TALL = [(r, n) for r in (17, 255, 256, 257, 300) for n in (1, 15, 16, 17, 63, 65)]
POOL_CS = (4, 72, 120, 268, 672)


def pool_hws(C, chunked):
    """HW at the edges of the eight-deep unroll of the plan's pixel lanes, and one (a few thousand at most) that its chunk count
    does not divide"""
    px = pool_plan(1, 1, C, chunked)['px']
    return sorted({1, max(px - 1, 1), px + 1, 8 * px - 1, 8 * px, 8 * px + 1}) + [min(21 * px + 5, 2999)]


MAXPOOL_CASES = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]              # (k, stride, pad)
AVGPOOL_CASES = [(2, 2, 7, 9), (3, 2, 8, 10), (3, 3, 8, 10), (2, 3, 9, 7)]      # (k, stride, H, W): H - k and W - k no multiple of stride
# (N, h, w, C, H, W, layouts of x and y)
RESIZE_FWD_STRIP = [
    (2, 2, 4, 256, 3, 16, 'ld4', 'off4'),       # 60 / 16 = 3: SEG 16
    (2, 3, 4, 512, 5, 15, 'off4', 'ld4'),       # 60 / 15 = 4: SEG 8
    (2, 2, 5, 256, 5, 10, 'contig', 'ld4'),
    (2, 2, 33, 512, 3, 65, 'ld4', 'contig'),    # 65 < 2 * 33: one column short of the strip path, the pixel path at two slabs
    (2, 2, 33, 512, 3, 66, 'off4', 'contig'),   # ... and on the switch W >= 2 w: SEG 8 at two slabs
    (2, 1, 1, 256, 2, 2, 'off4', 'contig'),
    (2, 1, 1, 512, 3, 33, 'ld4', 'off4'),
    (2, 2, 33, 256, 3, 129, 'off4', 'ld4'),     # 129 = 8 * 16 + 1: a last segment of one column
    (2, 3, 33, 512, 2, 129, 'contig', 'off4'),
    (2, 7, 4, 256, 3, 16, 'ld4', 'off4'),       # shrinks in y while it grows in x
]
RESIZE_FWD_PIXEL = [(N, h, w, C, H, W, lx, ly)
                    for C, lx, ly in ((4, 'ld4', 'off4'), (120, 'off4', 'contig'), (672, 'contig', 'ld4'))
                    for N, h, w, H, W in ((2, 10, 10, 7, 5), (1, 9, 13, 33, 50), (2, 3, 5, 3, 5))]
# (N, h, w, C, H, W, layouts of gy and gx, the window the columns must reach)
RESIZE_BWD = [
    (2, 2, 33, 256, 3, 129, 'ld4', 'off4', 'tight'),
    (1, 3, 5, 120, 7, 10, 'off4', 'contig', 'tight'),
    (2, 2, 4, 4, 5, 16, 'contig', 'ld4', 'maxw'),
    (1, 2, 4, 672, 3, 16, 'ld4', 'contig', 'maxw'),
    (1, 1, 1, 4, 3, 33, 'off4', 'ld4', 'general'),       # N h w = 1
    (2, 3, 2, 120, 5, 33, 'ld4', 'off4', 'general'),
    (1, 10, 10, 4, 5, 5, 'contig', 'off4', None),        # downsampling
    (2, 10, 10, 120, 7, 7, 'off4', 'ld4', None),
    (1, 7, 1, 4, 3, 33, 'ld4', 'contig', 'general'),     # N h w = 7
    (7, 1, 1, 120, 2, 2, 'contig', 'off4', None),        # N h w = 7 over seven images
    (1, 3, 3, 4, 5, 7, 'off4', 'ld4', None),             # N h w = 9
]


# ------------------------------------------------------------------------------------------------ seeded inputs (numpy)
def lane_inputs(C, M):
    r = np.random.default_rng(1000 * C + M % 997)
    d = {k: (r.standard_normal((M, C)) * 2).astype(F) for k in ('g', 'z', 'x', 'r', 'old')}
    N, _ = split_rows(M)
    d['gp'] = (r.standard_normal((N, C)) * 8).astype(F)
    d.update(channel_inputs(r, C))
    return d


def channel_inputs(r, C):
    d = {}
    for k in ('sc', 'rsc', 'inv'):
        d[k] = r.uniform(0.5, 1.5, C).astype(F)
    for k in ('sh', 'rsh'):
        d[k] = (r.standard_normal(C) * 0.5).astype(F)
    d['mu'] = (r.standard_normal(C) * 0.3).astype(F)
    coef = r.standard_normal((3, C))
    coef[0] = np.abs(coef[0]) + 0.5
    d['coef'] = coef.astype(F)
    return d


def row_inputs(seed, rows, n):
    """hand-made partial rows: O(1) noise plus a per-row offset of 1 .. 4, so that a skipped or doubled row moves every sum by far
    more than any bound here"""
    r = np.random.default_rng(seed)
    return (r.standard_normal((rows, n)) + (1 + np.arange(rows) % 4)[:, None]).astype(F)


# ------------------------------------------------------------------------------------------------ fp32 emulation (numpy)
def fma32(a, b, c):
    """fmaf(a, b, c) exactly: a * b is exact in double, the double sum is corrected where it is a tie of the fp32 rounding"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                     # TwoSum: p + c == s + e exactly
    tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    s = np.where(tie & (e != 0), np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def pro32(z, sc, sh):
    return z if sc is None else fma32(z, sc, sh)


def act32(v, act):
    """common.h act_apply"""
    if act == NONE:
        return v
    if act == RELU:
        return np.maximum(v, F(0))
    if act == RELU6:
        return np.minimum(np.maximum(v, F(0)), F(6))
    t = np.minimum(np.maximum(v + F(3), F(0)), F(6)) * SIXTH32
    return v * t if act == HSWISH else t


def grad32(u, act):
    """common.h act_grad"""
    if act == NONE:
        return np.ones_like(u)
    if act == RELU:
        return (u > 0).astype(F)
    if act == RELU6:
        return ((u > 0) & (u < 6)).astype(F)
    t = u + F(3)
    inside = np.where((t > 0) & (t < 6), SIXTH32, F(0)).astype(F)
    hs = np.minimum(np.maximum(t, F(0)), F(6)) * SIXTH32
    return hs + u * inside if act == HSWISH else inside


def keep_scale32(rate):
    return F(1.0) / (F(1.0) - F(rate))


def emu_bn_bwd_terms(i, o):
    u = pro32(i['z'], o['sc'], o['sh'])
    d = i['g'] * grad32(u, o['act'])
    mu = F(0) if o['mu'] is None else o['mu']
    inv = F(1) if o['inv'] is None else o['inv']
    return d, (i['z'] - mu) * inv


def emu_bn_bwd_apply(i, o, acc):
    d, xh = emu_bn_bwd_terms(i, o)
    c0, c1, c2 = (F(1), F(0), F(0)) if o['coef'] is None else o['coef']
    out = c0 * (d - c1 - xh * c2)
    return out + i['old'] if acc else out


def emu_bn_bwd_reduce(i, o):
    """the partial rows (nbx, 2, C) in the kernel's own order: lane (bx, pl) chains its grid-stride trips (add / fma), then the
    pixel lanes of a workgroup are added in lane order"""
    d, xh = emu_bn_bwd_terms(i, o)
    M, C = d.shape
    px = pick_lanes(C)[1]
    nbx = ew_nbx(M, C, MAX_STAT_ROWS)
    trips = -(-M // (nbx * px))
    pad = np.zeros((trips * nbx * px - M, C), F)             # (a lane without a row adds nothing)
    dz = np.concatenate([d, pad]).reshape(trips, nbx, px, C)
    xz = np.concatenate([np.broadcast_to(xh, d.shape), pad]).reshape(trips, nbx, px, C)
    a0, a1 = np.zeros((nbx, px, C), F), np.zeros((nbx, px, C), F)
    for t in range(trips):
        a0, a1 = a0 + dz[t], fma32(dz[t], xz[t], a1)
    r0, r1 = a0[:, 0], a1[:, 0]
    for q in range(1, px):
        r0, r1 = r0 + a0[:, q], r1 + a1[:, q]
    return np.stack([r0, r1], 1)


def seq_sum32(a):
    return np.cumsum(a, axis=0, dtype=F)[-1]


def emu_affine_act(i, o, residual=True, rate=0.0, keep=None):
    v = act32(pro32(i['x'], o['sc'], o['sh']), o['act'])
    if rate > 0:
        v = np.where(keep > 0, v * keep_scale32(rate), F(0))
    if residual:
        v = v + act32(pro32(i['r'], o['rsc'], o['rsh']), o['ract'])
    return v


def emu_scale_mask_bwd(i, acc, rate=0.0, keep=None):
    v = i['g']
    if rate > 0:
        v = np.where(keep > 0, v * keep_scale32(rate), F(0))
    return v + i['old'] if acc else v


def emu_gap_bwd(i, N, HW, acc):
    g = np.repeat(i['gp'] * (F(1) / F(HW)), HW, axis=0)
    return g + i['old'] if acc else g


def emu_lerp(x, H, W):
    """resize_fwd_kernel per output: top = tl + (tr - tl) tx; bot = bl + (br - bl) tx; out = top + (bot - top) ty, coefficients as
    lerp_coeff forms them"""
    from oracle import np_ops as O
    N, h, w, C = x.shape
    ylo, yhi, ty = O.bilinear_coeffs(h, H)
    xlo, xhi, tx = O.bilinear_coeffs(w, W)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    tl, tr = x[:, ylo][:, :, xlo], x[:, ylo][:, :, xhi]
    bl, br = x[:, yhi][:, :, xlo], x[:, yhi][:, :, xhi]
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    return top + (bot - top) * ty


def emu_resize_bwd(g, h, w):
    """resize_bwd_kernel: acc = fma(g, wy * wx, acc) over the window in (oy, ox) order; zero weights add nothing"""
    from oracle import np_ops as O
    N, H, W, C = g.shape
    ylo, yhi, ty = O.bilinear_coeffs(h, H)
    xlo, xhi, tx = O.bilinear_coeffs(w, W)
    out = np.zeros((N, h, w, C), F)
    for iy in range(h):
        wy = np.where(ylo == iy, F(1) - ty, F(0)) + np.where(yhi == iy, ty, F(0))
        for ix in range(w):
            wx = np.where(xlo == ix, F(1) - tx, F(0)) + np.where(xhi == ix, tx, F(0))
            acc = np.zeros((N, C), F)
            for oy in np.nonzero(wy)[0]:
                for ox in np.nonzero(wx)[0]:
                    acc = fma32(g[:, oy, ox], np.broadcast_to(F(wy[oy] * wx[ox]), acc.shape), acc)
            out[:, iy, ix] = acc
    return out


# ------------------------------------------------------------------------------------------------ float64 references (torch)
def D(a, dev='cpu'):
    if a is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev).double() if not torch.is_tensor(a) else a.to(dev).double()


class Check:
    """a float64 reference, its per-element bound and the alternatives (mask, reference) a near-kink element may match instead"""

    def __init__(self, ref, bound, alts=()):
        self.ref, self.bound, self.alts = ref, bound, list(alts)

    def worst(self, got):
        """max of err / bound over the elements that have no alternative (bound 0 and err 0 counts as 0)"""
        err = (got.double().reshape(self.ref.shape) - self.ref).abs()
        q = torch.where(err == 0, torch.zeros_like(err), err / self.bound)
        for mask, _ in self.alts:
            q = torch.where(mask, torch.zeros_like(q), q)
        return float(q.max())

    def verify(self, got, what):
        got = got.double().reshape(self.ref.shape)
        ok = (got - self.ref).abs() <= self.bound              # (NaN / Inf in got compare false)
        for mask, ref in self.alts:
            ok = ok | (mask & ((got - ref).abs() <= self.bound))
        if not bool(ok.all()):
            i = int((~ok).reshape(-1).nonzero()[0])
            raise AssertionError('%s: %d of %d elements out of bound; first at flat %d: got %r want %r (bound %.3g)' % (
                what, int((~ok).sum()), ok.numel(), i, float(got.reshape(-1)[i]), float(self.ref.reshape(-1)[i]),
                float(self.bound.reshape(-1)[i])))


def pro64(z, sc, sh):
    """u = z * scale + shift and T = |z * scale| + |shift|; the fma is ONE rounding (none without scale / shift)"""
    if sc is None:
        return z, z.abs(), 0
    return z * sc + sh, (z * sc).abs() + sh.abs(), 1


def act64(u, act):
    if act == NONE:
        return u
    if act == RELU:
        return u.clamp_min(0)
    if act == RELU6:
        return u.clamp(0, 6)
    t = (u + 3).clamp(0, 6) / 6
    return u * t if act == HSWISH else t


# roundings of act_apply after the prologue: none for the clamps; h-sigmoid v + 3, * (1/6) and the fp32 constant 1/6 itself = 3;
# h-swish one more for v * t = 4
ACT_K = {NONE: 0, RELU: 0, RELU6: 0, HSIGMOID: 3, HSWISH: 4}


def act_mag(T, act):
    """the magnitude of the terms of act(u) for |u| <= T"""
    if act in (NONE, RELU, RELU6):
        return T
    return (T + 3) / 6 if act == HSIGMOID else T * (T + 3) / 6


def grad_piece(u, act, piece):
    """act'(u) on the piece-th linear / quadratic piece of the activation (pieces are separated by KINKS[act])"""
    one, zero = torch.ones_like(u), torch.zeros_like(u)
    if act == NONE:
        return one
    if act == RELU:
        return (zero, one)[piece]
    if act == RELU6:
        return (zero, one, zero)[piece]
    if act == HSIGMOID:
        return (zero, one / 6, zero)[piece]
    return (zero, (2 * u + 3) / 6, one)[piece]


def grad64(u, act):
    """TF's convention, as common.h act_grad and oracle.np_ops.act_bwd have it: the inner derivative is 0 AT the kinks"""
    if act == NONE:
        return torch.ones_like(u)
    if act == RELU:
        return (u > 0).double()
    if act == RELU6:
        return ((u > 0) & (u < 6)).double()
    t = u + 3
    inside = ((t > 0) & (t < 6)).double() / 6
    return t.clamp(0, 6) / 6 + u * inside if act == HSWISH else inside


# roundings of act_grad: 0 / 1 for the clamps; h-sigmoid the constant 1/6 = 1; h-swish t = u + 3, * (1/6), the constant, u * in and
# the sum = 5
GRAD_K = {NONE: 0, RELU: 0, RELU6: 0, HSIGMOID: 1, HSWISH: 5}


def grad_mag(T, act):
    if act in (NONE, RELU, RELU6):
        return torch.ones_like(T)
    return torch.full_like(T, 1.0 / 6) if act == HSIGMOID else (T + 3) / 6 + T / 6


def near_kinks(u, T, act):
    """[(mask of the elements within 2 U T of kink j, j)]"""
    return [((u - k).abs() <= 2 * U * T, j) for j, k in enumerate(KINKS[act])]


def kink_share(u, T, act):
    near = torch.zeros_like(u, dtype=torch.bool)
    for mask, _ in near_kinks(u, T, act):
        near |= mask
    return float(near.double().mean())


def opts_of(case, i, dev):
    """the options of a lane case as float64 tensors (None where the case passes a null pointer)"""
    n = case['nulls']
    o = dict(act=case['act'], ract=case['ract'])
    for k in ('sc', 'sh', 'rsc', 'rsh', 'mu', 'inv', 'coef'):
        o[k] = D(i[k], dev)
    if n == 1:
        o['sc'] = o['sh'] = None
    if n == 2:
        o['mu'] = o['inv'] = o['rsc'] = o['rsh'] = None
    if n == 3:
        o['coef'] = None
    return o


def np_opts(o):
    return {k: (v.cpu().numpy().astype(F) if torch.is_tensor(v) else v) for k, v in o.items()}


def _bn_bwd_parts(t, o):
    """d = g * act'(u) with its magnitude, its roundings and its near-kink alternatives; xhat = (z - mean) * invstd likewise"""
    u, T, kf = pro64(t['z'], o['sc'], o['sh'])
    g = t['g']
    d = g * grad64(u, o['act'])
    dm = g.abs() * grad_mag(T, o['act'])
    kd = kf + GRAD_K[o['act']] + 1                       # the prologue fma, act_grad, g * act'
    alts = []
    for mask, j in near_kinks(u, T, o['act']):
        for piece in (j, j + 1):
            alts.append((mask, g * grad_piece(u, o['act'], piece)))
    mu = torch.zeros_like(t['z'][0]) if o['mu'] is None else o['mu']
    inv = torch.ones_like(t['z'][0]) if o['inv'] is None else o['inv']
    xh = (t['z'] - mu) * inv
    xm = (t['z'].abs() + mu.abs()) * inv.abs()           # z - mean, * invstd: 2 roundings
    return d, dm, kd, alts, xh, xm, (u, T)


def ref_bn_bwd_apply(t, o, acc):
    """dz = c0 * (d - c1 - xhat * c2) (+ old): roundings kd (d) + 2 (xhat) + 1 (* c2) + 2 (the subtractions) + 1 (c0 *) (+ 1), plus one"""
    d, dm, kd, alts, xh, xm, _ = _bn_bwd_parts(t, o)
    if o['coef'] is None:
        c0, c1, c2 = torch.ones_like(xh[0]), torch.zeros_like(xh[0]), torch.zeros_like(xh[0])
    else:
        c0, c1, c2 = o['coef']
    old = t['old'] if acc else torch.zeros_like(d)
    f = lambda dd: c0 * (dd - c1 - xh * c2) + old  # noqa: E731
    terms = c0.abs() * (dm + c1.abs() + xm * c2.abs()) + old.abs()
    k = kd + 2 + 1 + 2 + 1 + acc + 1
    return Check(f(d), k * U * terms, [(m, f(a)) for m, a in alts])


def ref_bn_bwd_reduce(t, o, rows):
    """[sum d, sum d * xhat] per channel: (M + rows + 4) U sum|terms|, plus for every near-kink element the span of its branches"""
    d, dm, kd, alts, xh, xm, (u, T) = _bn_bwd_parts(t, o)
    M = d.shape[0]
    span = torch.zeros_like(d)
    for i in range(0, len(alts), 2):
        span = torch.maximum(span, alts[i][0].double() * (alts[i][1] - alts[i + 1][1]).abs())
    ref = torch.stack([d.sum(0), (d * xh).sum(0)])
    bound = (M + rows + 4) * U * torch.stack([dm.sum(0), (dm * xm).sum(0)]) + torch.stack([span.sum(0), (span * xh.abs()).sum(0)])
    return Check(ref, bound)


def ref_affine_act(t, o, residual=True, rate=0.0, keep=None):
    """y = dropout(act(x * sc + sh)) + ract(r * rsc + rsh): roundings fma + act (+ 1 for * keep_scale) (+ fma + ract + 1 for the
    add), plus one"""
    u, T, kf = pro64(t['x'], o['sc'], o['sh'])
    a, am, k = act64(u, o['act']), act_mag(T, o['act']), kf + ACT_K[o['act']]
    if rate > 0:
        ks = float(keep_scale32(rate))
        a, am, k = a * ks * keep, am * ks * keep, k + 1
    if residual:
        ur, Tr, kr = pro64(t['r'], o['rsc'], o['rsh'])
        a, am, k = a + act64(ur, o['ract']), am + act_mag(Tr, o['ract']), k + kr + ACT_K[o['ract']] + 1
    return Check(a, (k + 1) * U * am)


def ref_scale_mask_bwd(t, acc, rate=0.0, keep=None):
    """gx = g (* keep_scale where kept, 0 elsewhere) (+ old): roundings (1) (+ 1), plus one"""
    v, k = t['g'], 0
    if rate > 0:
        v, k = v * float(keep_scale32(rate)) * keep, 1
    if acc:
        return Check(v + t['old'], (k + 2) * U * (v.abs() + t['old'].abs()))
    return Check(v, (k + 1) * U * v.abs())


def ref_gap_bwd(t, N, HW, acc):
    """gx[n, i] = gy[n] * (1 / HW) (+ old): roundings 1 / HW, the product (+ 1), plus one"""
    v = (t['gp'] / HW).repeat_interleave(HW, 0)
    if acc:
        return Check(v + t['old'], 4 * U * (v.abs() + t['old'].abs()))
    return Check(v, 3 * U * v.abs())


def lane_kink_shares(t, o):
    out = [kink_share(*pro64(t['z'], o['sc'], o['sh'])[:2], o['act']), kink_share(*pro64(t['x'], o['sc'], o['sh'])[:2], o['act']),
           kink_share(*pro64(t['r'], o['rsc'], o['rsh'])[:2], o['ract'])]
    return max(out)


# ---- finalize
def fin_inputs(rows, C, seed=0):
    r = np.random.default_rng(77 * rows + C + seed)
    part = np.empty((rows, 2, C), F)
    part[:, 0] = row_inputs(rows * 3 + C, rows, C)
    part[:, 1] = np.abs(row_inputs(rows * 5 + C, rows, C)) + 3
    d = dict(part=part, gamma=r.uniform(0.5, 1.5, C).astype(F), beta=(r.standard_normal(C) * 0.5).astype(F),
             mm=(r.standard_normal(C) * 0.5).astype(F), mv=r.uniform(0.5, 1.5, C).astype(F), count=float(rows * 8))
    d['sums'] = part.astype(np.float64).sum(0) * 1.25         # the `sums` path REPLACES the rows: a different total
    return d


EPS, MOM = float(F(1e-3)), float(F(0.99))


def ref_bn_finalize(s, ss, sabs, ssabs, rows, count, gamma, beta, mm, mv, update_moving):
    """{name: Check} from the exact sums s, ss (float64 tensors).  The kernel forms mean, var and invstd in double -- the double sums
    carry rows * 2^-53 * sum|x| -- and rounds: save_mean and save_invstd once (k = 2), scale = gamma * invstd twice (k = 3),
    shift = beta - (float)mean * scale over both terms (mean 1, scale 2, product 1, difference 1: k = 6), the moving averages
    m * mom + (float)v * (1 - mom) over both terms (v 1, 1 - mom 1, two products, the sum: k = 6)"""
    mean = s / count
    dmean = rows * 2 * UD * sabs / count
    var = (ss / count - mean * mean).clamp_min(0)
    dvar = rows * 2 * UD * ssabs / count + 2 * mean.abs() * dmean + 4 * UD * (ss / count + mean * mean)
    invstd = 1 / torch.sqrt(var + EPS)
    dinv = 0.5 * invstd * dvar / (var + EPS) + 4 * UD * invstd
    sc = gamma * invstd
    out = {'save_mean': Check(mean, 2 * U * mean.abs() + dmean),
           'save_invstd': Check(invstd, 2 * U * invstd + dinv),
           'scale': Check(sc, 3 * U * sc.abs() + gamma.abs() * dinv),
           'shift': Check(beta - mean * sc, 6 * U * (beta.abs() + (mean * sc).abs()) + dmean * sc.abs() + mean.abs() * gamma.abs() * dinv)}
    if update_moving:
        mvar = var * (count / (count - 1)) if update_moving == 2 and count > 1 else var
        out['moving_mean'] = Check(mm * MOM + mean * (1 - MOM), 6 * U * ((mm * MOM).abs() + (mean * (1 - MOM)).abs()) + dmean)
        out['moving_var'] = Check(mv * MOM + mvar * (1 - MOM), 6 * U * ((mv * MOM).abs() + mvar * (1 - MOM)) + 2 * dvar)
    return out


def emu_bn_finalize(s, ss, count, gamma, beta, mm, mv, update_moving):
    """bn_finalize_kernel after its reduction, on numpy doubles s, ss"""
    mean = s / count
    var = np.maximum(ss / count - mean * mean, 0.0)
    invstd = (1.0 / np.sqrt(var + np.float64(F(1e-3)))).astype(F)
    sc = gamma * invstd
    out = {'scale': sc, 'shift': beta - mean.astype(F) * sc, 'save_mean': mean.astype(F), 'save_invstd': invstd}
    if update_moving:
        mvar = var * (count / (count - 1.0)) if update_moving == 2 and count > 1 else var
        out['moving_mean'] = mm * F(0.99) + mean.astype(F) * (F(1) - F(0.99))
        out['moving_var'] = mv * F(0.99) + mvar.astype(F) * (F(1) - F(0.99))
    return out


def ref_bn_bwd_finalize(s, sx, sabs, sxabs, rows, count, gamma, invstd):
    """dbeta = (float)s, dgamma = (float)sx, coef = [gamma * invstd, (float)(s / count), (float)(sx / count)]: one rounding each
    (k = 2) behind the double sums"""
    e, ex = rows * 2 * UD * sabs, rows * 2 * UD * sxabs
    c0 = gamma * invstd
    return {'dbeta': Check(s, 2 * U * s.abs() + e), 'dgamma': Check(sx, 2 * U * sx.abs() + ex),
            'coef0': Check(c0, 2 * U * c0.abs()), 'coef1': Check(s / count, 2 * U * (s / count).abs() + e / count),
            'coef2': Check(sx / count, 2 * U * (sx / count).abs() + ex / count)}


def exact_sum(x):
    """column sums of fp32 rows, exact to a double: extended precision on the CPU"""
    x = np.asarray(x)
    return np.asarray(x.astype(np.longdouble).sum(0), np.float64)


def ref_reduce_rows(x, old, dev='cpu'):
    """out = (float)(double sum (+ out)): one rounding (k = 2) behind rows * 2^-53 * sum|x|"""
    s = D(exact_sum(x), dev)
    sa = D(np.abs(np.asarray(x, np.float64)).sum(0), s.device)
    if old is not None:
        s, sa = s + old, sa + old.abs()
    return Check(s, 2 * U * s.abs() + (x.shape[0] + 1) * 2 * UD * sa)


# ---- per-image reductions
def pool_inputs(N, HW, C):
    r = np.random.default_rng(31 * C + HW + N)
    d = {k: (r.standard_normal((N * HW, C)) * 2).astype(F) for k in ('x', 'g', 'old')}
    d['s'] = (r.standard_normal((N, C)) * 3).astype(F)
    d.update(channel_inputs(r, C))
    return d


def ref_gap_fwd(t, o, N, HW, out_scale, nchunk):
    """y[n] = out_scale / HW * sum_i act(x * sc + sh): an fp32 reduction of HW terms in nchunk partial rows"""
    u, T, _ = pro64(t['x'], o['sc'], o['sh'])
    a = act64(u, o['act']).reshape(N, HW, -1)
    am = act_mag(T, o['act']).reshape(N, HW, -1)
    sc = out_scale / HW
    k = HW + nchunk + 4 + ACT_K[o['act']]
    return Check(a.sum(1) * sc, k * U * am.sum(1) * sc)


def ref_scale_bcast_fwd(t, o, N, HW, s_act):
    """y = act(x * sc + sh) * s_act(s[n]): roundings fma + act, s_act, the product, plus one"""
    u, T, kf = pro64(t['x'], o['sc'], o['sh'])
    sv, sm = act64(t['s'], s_act).repeat_interleave(HW, 0), act_mag(t['s'].abs(), s_act).repeat_interleave(HW, 0)
    k = kf + ACT_K[o['act']] + ACT_K[s_act] + 1 + 1
    return Check(act64(u, o['act']) * sv, k * U * act_mag(T, o['act']) * sm)


def ref_scale_bcast_bwd(t, o, N, HW, s_act, acc, nchunk):
    """gx = gy * s_act(s[n]) (+ old) per element; gs[n] = sum_i gy * act(x * sc + sh), an fp32 reduction (fma chain) of HW terms"""
    u, T, kf = pro64(t['x'], o['sc'], o['sh'])
    sv, sm = act64(t['s'], s_act).repeat_interleave(HW, 0), act_mag(t['s'].abs(), s_act).repeat_interleave(HW, 0)
    gx, gm = t['g'] * sv, t['g'].abs() * sm
    k = ACT_K[s_act] + 1 + 1
    if acc:
        gx, gm, k = gx + t['old'], gm + t['old'].abs(), k + 1
    ta = (t['g'] * act64(u, o['act'])).reshape(N, HW, -1)
    tm = (t['g'].abs() * act_mag(T, o['act'])).reshape(N, HW, -1)
    kk = HW + nchunk + 4 + kf + ACT_K[o['act']]
    return Check(gx, k * U * gm), Check(ta.sum(1), kk * U * tm.sum(1))


def emu_pool(i, o, N, HW, s_act, out_scale):
    """global_avgpool_fwd, scale_bcast_fwd, scale_bcast_bwd (gx, gs) with sequential fp32 sums"""
    a = act32(pro32(i['x'], o['sc'], o['sh']), o['act'])
    C = a.shape[1]
    y = seq_sum32(a.reshape(N, HW, C).transpose(1, 0, 2)) * (F(out_scale) / F(HW))
    sv = np.repeat(act32(i['s'], s_act), HW, axis=0)
    g3, a3 = i['g'].reshape(N, HW, C), a.reshape(N, HW, C)
    gs = np.zeros((N, C), F)
    for p in range(HW):
        gs = fma32(g3[:, p], a3[:, p], gs)
    return y, a * sv, i['g'] * sv, gs


# ---- pooling windows
def pool_inputs2d(N, H, W, C, Ho, Wo, seed):
    r = np.random.default_rng(seed)
    d = dict(x=r.standard_normal((N, H, W, C)).astype(F), dy=r.standard_normal((N, Ho, Wo, C)).astype(F),
             old=r.standard_normal((N, H, W, C)).astype(F))
    d.update(channel_inputs(r, C))
    return d


def windows(a, k, s, pad, Ho, Wo):
    """(N, Ho, Wo, C, k*k) taps of the zero-padded map in (ky, kx) order"""
    ap = np.pad(a, ((0, 0), (pad, pad + k), (pad, pad + k), (0, 0)))
    return np.stack([ap[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] for ky in range(k) for kx in range(k)], -1)


def scatter_windows(sel, k, s, pad, H, W):
    """the transpose of windows(): sel (N, Ho, Wo, C, k*k) float64 back onto the (N, H, W, C) map"""
    N, Ho, Wo, C, _ = sel.shape
    gp = np.zeros((N, H + 2 * pad + k, W + 2 * pad + k, C))
    for t in range(k * k):
        ky, kx = divmod(t, k)
        gp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] += sel[..., t]
    return gp[:, pad:pad + H, pad:pad + W, :]


def ref_maxpool(i, act, k, s, pad, Ho, Wo):
    """the forward EXACTLY (the fp32 prologue, then a maximum in float64 with the zero padding taking part), its first-maximum
    tap, the backward gradient in float64 with the magnitude of its terms and the number of windows over each input pixel"""
    a = act32(pro32(i['x'], i['sc'], i['sh']), act)
    win = windows(a.astype(np.float64), k, s, pad, Ho, Wo)
    arg = win.argmax(-1)
    y = np.take_along_axis(win, arg[..., None], -1)[..., 0]
    hit = np.arange(k * k) == arg[..., None]
    N, H, W, C = i['x'].shape
    dy = i['dy'].astype(np.float64)[..., None]
    gx = scatter_windows(np.where(hit, dy, 0.0), k, s, pad, H, W)
    gm = scatter_windows(np.where(hit, np.abs(dy), 0.0), k, s, pad, H, W)
    cnt = scatter_windows(np.ones(hit.shape), k, s, pad, H, W)
    return a, y, arg, gx, gm, cnt


def ref_avgpool(i, act, k, s, Ho, Wo):
    """forward mean of the k*k taps (a chain of k*k fp32 adds and a division) and the backward sum over the covering windows / k*k"""
    u, T, kf = pro64(D(i['x']), D(i['sc']), D(i['sh']))
    a, am = act64(u, act).numpy(), act_mag(T, act).numpy()
    y = windows(a, k, s, 0, Ho, Wo).sum(-1) / (k * k)
    ym = windows(am, k, s, 0, Ho, Wo).sum(-1) / (k * k)
    N, H, W, C = i['x'].shape
    dy = np.broadcast_to(i['dy'].astype(np.float64)[..., None], i['dy'].shape + (k * k,))
    gx = scatter_windows(dy, k, s, 0, H, W) / (k * k)
    gm = scatter_windows(np.abs(dy), k, s, 0, H, W) / (k * k)
    cnt = scatter_windows(np.ones(dy.shape), k, s, 0, H, W)
    kfwd = kf + ACT_K[act] + k * k + 1 + 1                    # prologue, k*k adds, the division, plus one
    return y, kfwd * U * ym, gx, gm, cnt


# ---- bilinear resize
def ref_resize_fwd(x, H, W):
    """oracle.np_ops.resize_bilinear_fwd in float64 (coordinates in fp32) and the bound of the two-level lerp: top and bot are
    3 roundings each over |tl| + (|tr| + |tl|) tx, the last lerp 3 more over |top| + (|bot| + |top|) ty: k = 10"""
    from oracle import np_ops as O
    x = x.astype(np.float64)
    h, w = x.shape[1:3]
    ylo, yhi, ty = O.bilinear_coeffs(h, H)
    xlo, xhi, tx = O.bilinear_coeffs(w, W)
    tx = tx.astype(np.float64)[None, None, :, None]
    ty = ty.astype(np.float64)[None, :, None, None]
    ax = np.abs(x)
    top = ax[:, ylo][:, :, xlo] + (ax[:, ylo][:, :, xhi] + ax[:, ylo][:, :, xlo]) * tx
    bot = ax[:, yhi][:, :, xlo] + (ax[:, yhi][:, :, xhi] + ax[:, yhi][:, :, xlo]) * tx
    return O.resize_bilinear_fwd(x, H, W), 10 * U * (top + (bot + top) * ty)


def ref_resize_bwd(g, h, w):
    """the float64 transpose of the fp32-coefficient operator; an input pixel is an fma chain over its nnz non-zero weights
    wy * wx (1 - t, 1 - t and the product: 3 roundings): (nnz + 3 + 1) U sum|g| |w|"""
    from oracle import np_ops as O
    g = g.astype(np.float64)
    H, W = g.shape[1:3]
    Ry, Rx = O.bilinear_matrix(h, H, np.float64), O.bilinear_matrix(w, W, np.float64)
    gm = O._apply_axis(np.abs(Rx).T, O._apply_axis(np.abs(Ry).T, np.abs(g), 1), 2)
    nnz = ((Ry != 0).sum(0)[:, None] * (Rx != 0).sum(0)[None, :])[None, :, :, None]
    return O.resize_bilinear_bwd(g, h, w), gm, nnz


# ------------------------------------------------------------------------------------------------ canary planes (torch)
class Plane:
    """a (rows, C) fp32 operand inside its own buffer: `after` canary rows past its last row and, for 'ld4' (row stride C + 4) and
    'off4' (base 4 floats in, row stride C + 8), canary channels beside it.  The buffer always holds (rows + after) rows of the
    WIDEST stride, so that nothing outside it is addressed even by a launch that walked it with another operand's stride."""

    def __init__(self, rows, C, layout='contig', after=3, dev='cuda'):
        lo, w = {'contig': (0, C), 'ld4': (0, C + 4), 'off4': (4, C + 8)}[layout]
        n = (rows + after) * (C + 8)
        pat = torch.tensor(CANARY, dtype=torch.int32, device=dev)
        self.bits = pat.repeat((n + 2) // 3)[:n].contiguous()
        self.grid = self.bits[:(rows + after) * w].view(rows + after, w)
        self.t = self.grid.view(torch.float32)[:rows, lo:lo + C]
        self.ld, self.rows, self.C, self.lo, self.after = w, rows, C, lo, after
        self.keep = self.bits.clone()

    def set(self, v):
        self.t.copy_(torch.as_tensor(v).reshape(self.rows, self.C))
        self.keep = self.bits.clone()
        return self

    @property
    def p(self):
        return self.t.data_ptr()

    def intact(self, what):
        same = self.bits == self.keep
        same[:(self.rows + self.after) * self.ld].view(-1, self.ld)[:self.rows, self.lo:self.lo + self.C] = True
        bad = int((~same).sum())
        assert bad == 0, '%s: %d canary elements beside / past the output changed' % (what, bad)


def plane(v, layout, dev='cuda'):
    """an input plane holding v (rows, C)"""
    v = torch.as_tensor(v)
    v = v.reshape(-1, v.shape[-1])
    return Plane(v.shape[0], v.shape[1], layout, dev=dev).set(v)


def out_plane(rows, C, layout, base=None, dev='cuda'):
    """an output plane: canaries everywhere, the view set to `base` (accumulating forms) or left as canaries"""
    o = Plane(rows, C, layout, dev=dev)
    return o.set(base) if base is not None else o


class Vec:
    """a per-channel operand (k, C) with a NaN row behind it"""

    def __init__(self, v, dev='cuda'):
        v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        self.buf = torch.full((v.numel() + 8,), float('nan'), dtype=torch.float32, device=dev)
        self.buf[:v.numel()] = v
        self.p = self.buf.data_ptr()


def vec(v, dev='cuda'):
    return None if v is None else Vec(v, dev)


def ptr(v):
    return None if v is None else v.p
