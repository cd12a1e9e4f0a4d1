"""The fused inverted-residual kernels (csrc/irb_fwd.hip, irb_bwd.hip) per element at every plan edge, against float64.

The cases, the float64 reference and the per-element bounds are tests/irb_rules.py (tests/test_irb_rules_cpu.py holds the tables to
the plan query and the bounds to a float32 evaluation, without a GPU).  Here every row is launched through the C ABI.

Every operand sits in an allocation of its own: an image row and a pixel of guards before and after it and, for the 'view'
layouts, guard channels beside every row (x: ld = K + 8 at channel 4, or K + 2 at 2 for K = 24; y / dy: ld = C + 12 at 8; gx / z0:
ld = K + 8 at 4).  Inputs carry a NaN with a payload, +Inf and -Inf there; outputs one sentinel bit pattern that must come back
bit-identical wherever the kernel does not own the element, and must be gone wherever it does: y, gx, the statistic rows, the slab
workspaces, the front rows, rows_out.  All guards lie inside allocated memory.

y is held BITWISE across CT in {1, 2, 3} and across band counts: every output element is one chain -- the MFMA chain of its nine
inputs (k ascending, the same fragments whatever the channel tile), then mul / fma over the taps with ky, kx ascending (stride 2:
taps 0..2 from the band's first even row or from the previous step's `nxt`, the same three operations; stride 1: a0 = taps 0..2, then
taps 3..5 and 6..8 are added as the next two input rows arrive) -- and masked taps add exact zeros in every plan.  No pair is held to
the bound instead."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from conftest import load_pkg  # noqa: E402
import irb_rules as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IN_CANARY = (0x7FC00A5A, 0x7F800000, -0x00800000)      # int32 bits: a NaN with a payload, +Inf, -Inf
SENTINEL = 0x7FA5C3E1                                  # outputs: one NaN bit pattern no kernel produces
MAX_ROWS = 2048                                        # DL3P_MAX_STAT_ROWS
RATIOS = {}                                            # largest err / bound per kernel, for the record (printed, never asserted)


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return load_pkg('_lib').lib()


@pytest.fixture
def knobs(L):
    """dl3p_irb_set_plan / dl3p_irb_set_bwd_plan for the time of a case, (0, 0) afterwards"""
    def set_(c):
        if isinstance(c, R.F):
            L.irb_set_plan(c.ct, c.waves)
        else:
            L.irb_set_bwd_plan(*c.knobs)
    yield set_
    L.irb_set_plan(0, 0)
    L.irb_set_bwd_plan(0, 0)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _note(kernel, ratio):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print('%s: err / bound %.3f (largest so far %.3f)' % (kernel, ratio, RATIOS[kernel]))


def _canary(n):
    pat = torch.tensor(IN_CANARY, dtype=torch.int32, device=DEV)
    return pat.repeat((n + 2) // 3)[:n].contiguous()


class Plane:
    """a (rows, C) float32 operand inside its own buffer: `guard` rows around it and, for a view, guard channels on either side of
    every row (the view starts `lo` floats into rows of `ld`).  value given: an input (canaries around it) unless out=True."""

    def __init__(self, rows, C, guard, value=None, lo=0, ld=None, out=False):
        ld = ld or C
        Rr = rows + 2 * guard
        if out or value is None:
            self.bits = torch.full((Rr, ld), SENTINEL, dtype=torch.int32, device=DEV)
        else:
            self.bits = _canary(Rr * ld).reshape(Rr, ld)
        self.t = self.bits.view(torch.float32)[guard:guard + rows, lo:lo + C]
        if value is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(value, dtype=np.float32).reshape(rows, C)))
        self.keep = self.bits.clone()
        self.ld, self.rows, self.C, self.lo, self.guard = ld, rows, C, lo, guard

    @property
    def p(self):
        return self.t.data_ptr()

    def own(self):
        return self.t.contiguous().view(torch.int32)

    def intact(self, what):
        mask = torch.ones_like(self.bits, dtype=torch.bool)
        mask[self.guard:self.guard + self.rows, self.lo:self.lo + self.C] = False
        bad = int((self.bits[mask] != self.keep[mask]).sum())
        assert bad == 0, '%s: %d sentinel elements beside / before / past the output changed' % (what, bad)

    def untouched(self, what):
        assert torch.equal(self.bits, self.keep), '%s: written although not asked for' % what

    def written(self, what):
        left = int((self.own() == SENTINEL).sum())
        assert left == 0, '%s: %d output elements never written' % (what, left)

    def numpy(self, shape):
        return self.t.contiguous().cpu().numpy().reshape(shape)


class Flat:
    """a flat float32 output (statistic rows, slabs, front rows): sentinels everywhere, `n` elements of it are the kernel's"""

    def __init__(self, total, guard=256):
        self.guard = guard
        self.bits = torch.full((total + 2 * guard,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.bits.view(torch.float32)[guard:]

    @property
    def p(self):
        return self.t.data_ptr()

    def check(self, n, what):
        g = self.guard
        bad = int((self.bits[:g] != SENTINEL).sum()) + int((self.bits[g + n:] != SENTINEL).sum())
        assert bad == 0, '%s: %d elements before the first / past the last row changed' % (what, bad)
        left = int((self.bits[g:g + n] == SENTINEL).sum())
        assert left == 0, '%s: %d elements of the rows never written' % (what, left)

    def rows(self, n, shape):
        return self.t[:n].cpu().numpy().astype(np.float64).reshape(shape)


def vec(v):
    """a small input (kernels, coefficient vectors) with 64 canaries before and after it; None stays None"""
    if v is None:
        return None
    v = np.ascontiguousarray(v, dtype=np.float32)
    buf = _canary(v.size + 128).view(torch.float32)
    buf[64:64 + v.size].copy_(torch.from_numpy(v.reshape(-1)))
    return buf[64:64 + v.size]


def _p(t):
    return None if t is None else t.data_ptr()


class RowsOut:
    """the host int a launch reports its row count in, between two sentinels"""

    def __init__(self):
        self.a = (ctypes.c_int * 3)(SENTINEL, SENTINEL, SENTINEL)

    @property
    def ref(self):
        return ctypes.cast(ctypes.byref(self.a, 4), ctypes.POINTER(ctypes.c_int))

    def value(self, what):
        assert self.a[0] == SENTINEL and self.a[2] == SENTINEL and self.a[1] != SENTINEL, what + ': rows_out'
        return self.a[1]


def query(L, which, c):
    Ho, Wo, pt, pl = R.geom(c)
    out = (ctypes.c_int * 8)()
    L.irb_plan_query(which, c.N, c.H, c.W, c.K, c.C, c.s, pt, pl, Ho, Wo, out)
    return list(out)


X_VIEW = {'contig': (0, 0), 'view': (4, 8), 'view2': (2, 2)}      # layout -> (channel offset, extra floats per row) of x


def x_plane(c, d, key='x', out=False, value=True):
    lo, extra = X_VIEW[c.layout]
    return Plane(c.N * c.H * c.W, c.K, c.W + 1, d[key] if value else None, lo, c.K + extra, out=out)


def c_plane(c, rows, value=None):
    """an operand with C channels (y, dy): ld = C + 12 at channel 8 in the view layouts"""
    lo, ld = (0, c.C) if c.layout == 'contig' else (8, c.C + 12)
    return Plane(rows, c.C, R.geom(c)[1] + 1, value, lo, ld)


# -------------------------------------------------------------------------------------------------------------------- forward
def launch_forward(L, c, d, dv):
    """-> (Y plane, rows, partial rows Flat); dv: the small operands on the device"""
    Ho, Wo, pt, pl = R.geom(c)
    X = x_plane(c, d)
    Y = c_plane(c, c.N * Ho * Wo)
    part = Flat(MAX_ROWS * 2 * c.C)
    ro = RowsOut()
    L.irb_fwd(X.p, X.ld, _p(dv['xs']), _p(dv['xh']), c.pair[0], _p(dv['w1']), _p(dv['sc']), _p(dv['sh']), c.pair[1], _p(dv['wdw']),
              Y.p, Y.ld, part.p, ro.ref, c.N, c.H, c.W, c.K, c.C, c.s, pt, pl, Ho, Wo, _s())
    torch.cuda.synchronize()
    return Y, ro.value(c.name), part


def small(d, names):
    return {k: vec(d[k]) for k in names}


@pytest.mark.parametrize('c', R.FWD, ids=lambda c: c.name)
def test_forward(L, knobs, c):
    d = R.inputs(c)
    Ho, Wo, pt, pl = R.geom(c)
    knobs(c)
    plan = query(L, 0, c)
    assert (plan[0], plan[1], plan[2], plan[3], plan[6]) == c.plan and plan[7] == 1, plan
    Y, rows, part = launch_forward(L, c, d, small(d, ('xs', 'xh', 'w1', 'sc', 'sh', 'wdw')))
    what = c.name + ' forward'
    assert rows == plan[6] <= MAX_ROWS, (rows, plan)
    Y.intact(what)
    Y.written(what)
    part.check(rows * 2 * c.C, what + ' statistic rows')
    y = Y.numpy((c.N, Ho, Wo, c.C))
    ref, bound = R.fwd_ref(d, c)
    _note(R.fwd_kernel(c, plan[0]), R.inside(y, ref, bound, what))
    val, sbound = R.stat_ref(y)
    R.inside(part.rows(rows * 2 * c.C, (rows, 2, c.C)).sum(0), val, sbound, what + ' statistic rows')


BITWISE = [(2, 9, 17, 16, 96, (1, 2, 3)), (1, 9, 17, 24, 144, (1, 3)), (1, 10, 31, 32, 192, (1, 2, 3)), (2, 11, 9, 24, 96, (1, 2, 3))]


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('pair', [R.FAST, R.GEN['hswish']], ids=['fast', 'generic'])
@pytest.mark.parametrize('shape', BITWISE, ids=lambda v: 'k%d_c%d' % (v[3], v[4]))
def test_forward_bits_do_not_depend_on_the_plan(L, knobs, shape, pair, s):
    """y bitwise across the channel tiles per wave and across the band counts (want_waves 1: one band; BIG: bands of 4)"""
    N, H, W, K, C, cts = shape
    seen, plans = None, set()
    for ct in cts:
        for waves in (1, R.BIG):
            c = R._f('bits_k%d_s%d' % (K, s), N, H, W, K, C, s, None, ct=ct, waves=waves, pair=pair)
            d = R.inputs(c)
            knobs(c)
            plan = query(L, 0, c)
            assert plan[0] == ct, plan
            plans.add((plan[0], plan[2]))
            Y, rows, part = launch_forward(L, c, d, small(d, ('xs', 'xh', 'w1', 'sc', 'sh', 'wdw')))
            Y.written(c.name)
            bits = Y.own()
            assert seen is None or torch.equal(bits, seen), '%s: y differs between plans at ct=%d waves=%d' % (c.name, ct, waves)
            seen = bits
    assert len(plans) == 2 * len(cts), plans


# ------------------------------------------------------------------------------------------------------------------- backward
def launch_pass_b(L, c, d, dv, X, DY, accumulate, want_gx, front):
    Ho, Wo, pt, pl = R.geom(c)
    lo, ld = (0, c.K) if c.layout == 'contig' else (4, c.K + 8)
    n = c.N * c.H * c.W
    G = Plane(n, c.K, c.W + 1, d['base'] if accumulate else None, lo, ld, out=True)
    Z0 = Plane(n, c.K, c.W + 1, d['z0'], lo, ld)
    need = L.irb_bwd_workspace(1, c.N, c.H, c.W, c.K, c.C, c.s, pt, pl)
    slabs, part0, ro = Flat(need // 4), Flat(MAX_ROWS * 2 * c.K), RowsOut()
    f = front
    L.irb_bwd_data(X.p, X.ld, _p(dv['xs']), _p(dv['xh']), c.pair[0], _p(dv['w1']), _p(dv['sc']), _p(dv['sh']), c.pair[1], _p(dv['mu']),
                   _p(dv['inv']), _p(dv['coef']), _p(dv['wdw']), DY.p, DY.ld, slabs.p, need, ro.ref, G.p if want_gx else None, G.ld,
                   int(accumulate), Z0.p if f else None, Z0.ld, _p(dv['s0']) if f else None, _p(dv['h0']) if f else None, c.act0,
                   _p(dv['mu0']) if f else None, _p(dv['is0']) if f else None, part0.p if f else None, c.N, c.H, c.W, c.K, c.C, c.s,
                   pt, pl, Ho, Wo, _s())
    torch.cuda.synchronize()
    return G, slabs, part0, ro.value(c.name), need


@pytest.mark.parametrize('c', R.BWD, ids=lambda c: c.name)
def test_backward(L, knobs, c):
    d = R.inputs(c)
    Ho, Wo, pt, pl = R.geom(c)
    knobs(c)
    pa, pb = query(L, 1, c), query(L, 2, c)
    assert (pa[1], pa[2], pa[3], pa[5], pa[6]) == c.planA and (pb[1], pb[2], pb[3], pb[5], pb[6]) == c.planB, (pa, pb)
    dv = small(d, ('xs', 'xh', 'w1', 'sc', 'sh', 'mu', 'inv', 'coef', 'wdw', 's0', 'h0', 'mu0', 'is0'))
    X = x_plane(c, d)
    DY = c_plane(c, c.N * Ho * Wo, d['dy'])
    K, C, n = c.K, c.C, c.N * c.H * c.W
    ka, kb = R.bwd_kernels(c)
    # ---- pass A
    need = L.irb_bwd_workspace(0, c.N, c.H, c.W, K, C, c.s, pt, pl)
    assert need == pa[6] * 9 * C * 4
    slabs, part, ro = Flat(need // 4), Flat(MAX_ROWS * 2 * C), RowsOut()
    L.irb_bwd_sums(X.p, X.ld, _p(dv['xs']), _p(dv['xh']), c.pair[0], _p(dv['w1']), _p(dv['sc']), _p(dv['sh']), c.pair[1], _p(dv['mu']),
                   _p(dv['inv']), _p(dv['wdw']), DY.p, DY.ld, slabs.p, need, ro.ref, part.p, c.N, c.H, c.W, K, C, c.s, pt, pl, Ho, Wo,
                   _s())
    torch.cuda.synchronize()
    rows = ro.value(c.name)
    what = c.name + ' pass A'
    assert rows == pa[6], (rows, pa)
    slabs.check(rows * 9 * C, what + ' slabs')
    part.check(rows * 2 * C, what + ' BN1 rows')
    a = R.pass_a_ref(d, c)
    assert a['share'] <= R.AMBIGUOUS_CAP
    r1 = R.inside(slabs.rows(rows * 9 * C, (rows, 3, 3, C)).sum(0), a['gwdw'], a['gwdw_b'], what + ' gwdw')
    r2 = R.inside(part.rows(rows * 2 * C, (rows, 2, C)).sum(0), a['rows'], a['rows_b'], what + ' BN1 rows', a['rows_s'])
    _note(ka, max(r1, r2))
    # ---- pass B: with the BatchNorm in front, plain and accumulating
    assert L.irb_bwd_workspace(1, c.N, c.H, c.W, K, C, c.s, pt, pl) == pb[6] * K * C * 4
    used = -(-pb[5] // 4)                                  # workgroups that have a unit; the grid is rounded up to 8
    first = {}
    for accumulate in (False, True):
        what = '%s pass B accumulate %d' % (c.name, accumulate)
        b = R.pass_b_ref(d, c, accumulate, True, a)
        G, slabs, part0, rows, need = launch_pass_b(L, c, d, dv, X, DY, accumulate, True, True)
        assert rows == pb[6] and rows % 8 == 0 and used <= rows, (rows, pb)
        slabs.check(rows * K * C, what + ' gw1 slabs')       # exactly K rows of C per slab: nothing of the pad lanes past them
        part0.check(rows * 2 * K, what + ' front rows')      # ... and exactly K columns per front row
        G.intact(what + ' gx')
        G.written(what + ' gx')
        sl, fr = slabs.rows(rows * K * C, (rows, K, C)), part0.rows(rows * 2 * K, (rows, 2, K))
        assert (sl[used:] == 0).all() and (fr[used:] == 0).all(), what + ': a workgroup without a unit left a non-zero row'
        r = [R.inside(sl.sum(0), b['gw1'], b['gw1_b'], what + ' gw1', b['gw1_s']),
             R.inside(G.numpy((c.N, c.H, c.W, K)), b['gx'], b['gx_b'], what + ' gx', b['gx_s']),
             R.inside(fr.sum(0), b['front'], b['front_b'], what + ' front rows', b['front_s'])]
        _note(kb, max(r))
        if not accumulate:
            first = dict(gw1=slabs.bits.clone(), gx=G.own())
    # ---- without the BatchNorm in front: the same bits, the front rows untouched
    G, slabs, part0, rows, _ = launch_pass_b(L, c, d, dv, X, DY, False, True, False)
    assert torch.equal(slabs.bits, first['gw1']) and torch.equal(G.own(), first['gx']), c.name + ': front absent changes bits'
    assert bool((part0.bits == SENTINEL).all())
    G.intact(c.name + ' gx, no front')
    # ---- without a gradient for the input: the kernel gradient alone, same bits, gx untouched
    G, slabs, part0, rows, _ = launch_pass_b(L, c, d, dv, X, DY, False, False, False)
    assert torch.equal(slabs.bits, first['gw1']), c.name + ': want_gx off changes gw1'
    G.untouched(c.name + ' gx')
    assert bool((part0.bits == SENTINEL).all())
    # the inputs were read only
    X.untouched(c.name + ' x')
    DY.untouched(c.name + ' dy')


# ----------------------------------------------------------------------------------------------------------------- covariance
COV = [(1, 16, 'contig', R.NONE), (63, 24, 'contig', R.NONE), (64, 32, 'view', R.NONE), (65, 16, 'view', R.RELU6), (4097, 24, 'view', R.HSWISH),
       (4097, 32, 'contig', R.RELU)]


@pytest.mark.parametrize('M,K,layout,act', COV, ids=lambda v: str(v))
def test_covariance_rows(L, M, K, layout, act):
    rng = np.random.default_rng(M * 64 + K)
    x, xs, xh = R.f32(rng.standard_normal((M, K))), R.f32(rng.uniform(0.5, 1.5, K)), R.f32(rng.standard_normal(K) * 0.3)
    lo, ld = (0, K) if layout == 'contig' else (4, K + 8)
    X = Plane(M, K, 2, x, lo, ld)
    rmax, n = L.irb_cov_rows_max(), K + K * K
    pat = torch.tensor([0x7FF8A5A5C3E10001], dtype=torch.int64, device=DEV)
    buf = pat.repeat((rmax + 2) * n)
    cov = buf.view(torch.float64)[n:]
    ro = RowsOut()
    dxs, dxh = vec(xs), vec(xh)
    L.irb_cov_stats(X.p, X.ld, _p(dxs), _p(dxh), act, cov.data_ptr(), rmax, ro.ref, M, K, _s())
    sums_buf = pat.repeat(n + 2)
    L.irb_cov_reduce(cov.data_ptr(), ro.a[1], K, sums_buf.view(torch.float64)[1:].data_ptr(), _s())
    torch.cuda.synchronize()
    rows = ro.value('cov')
    assert 0 < rows <= rmax
    own = buf[n:n + rows * n]
    assert int((own == pat).sum()) == 0, 'a row below rows_out was not fully written'
    assert bool((buf[:n] == pat).all()) and bool((buf[n + rows * n:] == pat).all()), 'rows beyond rows_out were touched'
    assert int(sums_buf[0]) == int(pat) and int(sums_buf[-1]) == int(pat)
    X.untouched('cov x')
    xk = R.act32(R.fma32(x, xs, xh), act).astype(np.float64)
    want = np.concatenate([xk.sum(0), (xk.T @ xk).reshape(-1)])
    for got in (cov[:rows * n].cpu().numpy().reshape(rows, n).sum(0), sums_buf.view(torch.float64)[1:1 + n].cpu().numpy()):
        rel = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
        assert rel < 1e-9, rel
