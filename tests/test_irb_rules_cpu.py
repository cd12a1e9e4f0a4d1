"""The case tables, the float64 reference and the bounds of tests/irb_rules.py, held on the CPU (nothing is launched):
the plan every row names is the plan dl3p_irb_plan_query reports, the rows reach every launchable instantiation of the three fused
inverted-residual kernels, a float32 evaluation of the kernels' operations stays inside the bounds in two summation orders, and no
backward case sets more than 2% of its pixels aside as undecided at an activation kink."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from conftest import load_pkg  # noqa: E402
import irb_rules as R  # noqa: E402


def _lib():
    return load_pkg('_lib').lib()


def query(L, which, c, K=None, C=None, geo=None):
    Ho, Wo, pt, pl = geo or R.geom(c)
    out = (ctypes.c_int * 8)()
    L.irb_plan_query(which, c.N, c.H, c.W, K or c.K, C or c.C, c.s, pt, pl, Ho, Wo, out)
    return list(out)


@pytest.fixture
def knobs():
    """dl3p_irb_set_plan / dl3p_irb_set_bwd_plan for the time of a case, (0, 0) afterwards"""
    L = _lib()

    def set_(c):
        if isinstance(c, R.F):
            L.irb_set_plan(c.ct, c.waves)
        else:
            L.irb_set_bwd_plan(*c.knobs)
    yield set_
    L.irb_set_plan(0, 0)
    L.irb_set_bwd_plan(0, 0)


def test_case_names_are_unique():
    assert len({c.name for c in R.FWD}) == len(R.FWD) and len({c.name for c in R.BWD}) == len(R.BWD)


def test_forward_rows_name_the_plan_the_query_reports(knobs):
    L = _lib()
    wrong = {}
    for c in R.FWD:
        knobs(c)
        o = query(L, 0, c)
        Ho, Wo, _, _ = R.geom(c)
        got = (o[0], o[1], o[2], o[3], o[6])
        if got != c.plan or o[7] != 1:
            wrong[c.name] = (got, c.plan)
        ct, nseg, nband, band, rows = got
        # the numbers hang together: segments of 15 / 14 outputs, bands that cover Ho, one row per (image, segment, band)
        assert nseg == -(-Wo // (15 if c.s == 2 else 14)) and (nband - 1) * band < Ho <= nband * band, (c.name, o)
        assert o[4] == c.C // (16 * ct) and o[5] == c.N * nseg * nband * o[4] and rows == c.N * nseg * nband <= 2048, (c.name, o)
    assert not wrong, wrong
    by = {c.name: c for c in R.FWD}
    # the edges the table is built around, read back from the table
    assert [by[n].plan[1] for n in ('s2_w29', 's2_w30', 's2_w31', 's2_w59', 's2_w60', 's2_w61')] == [1, 1, 2, 2, 2, 3]
    assert [by[n].plan[1] for n in ('s1_w14', 's1_w15', 's1_w28', 's1_w29')] == [1, 2, 2, 3]
    assert by['k24_c144_ct2_falls_back'].ct == 2 and by['k24_c144_ct2_falls_back'].plan[0] == 1
    assert by['clamp'].plan[4] <= 2048 < 16 * 3 * 170
    assert all(by[n].plan[3] == 4 for n in by if '_b' in n and by[n].waves == R.BIG)


def test_backward_rows_name_the_plan_the_query_reports(knobs):
    L = _lib()
    wrong = {}
    for c in R.BWD:
        knobs(c)
        a, b = query(L, 1, c), query(L, 2, c)
        got = ((a[1], a[2], a[3], a[5], a[6]), (b[1], b[2], b[3], b[5], b[6]))
        if got != (c.planA, c.planB) or a[7] != 1 or b[7] != 1:
            wrong[c.name] = (got, (c.planA, c.planB))
        csteps = (c.W + R.geom(c)[3] + 1) // 2 if c.s == 2 else c.W
        rsteps = (c.H + R.geom(c)[2] + 1) // 2 if c.s == 2 else c.H
        for o, ncg, rows in ((a, c.C // 16, c.N * a[1] * a[2]), (b, 1, -(-(-(-b[5] // 4)) // 8) * 8)):
            assert o[1] == -(-csteps // 16) and (o[2] - 1) * o[3] < rsteps <= o[2] * o[3], (c.name, o)
            assert o[4] == ncg and o[5] == c.N * o[1] * o[2] * ncg and o[6] == rows, (c.name, o)
    assert not wrong, wrong
    steps = lambda c: ((c.W + R.geom(c)[3] + 1) // 2 if c.s == 2 else c.W, (c.H + R.geom(c)[2] + 1) // 2 if c.s == 2 else c.H)  # noqa: E731
    for s in (1, 2):
        rows = [c for c in R.BWD if c.s == s]
        assert {1, 16, 17, 33} <= {steps(c)[0] for c in rows} and {1, 2, 3, 5} <= {steps(c)[1] for c in rows}, s
    assert {c.planB[3] % 4 for c in R.BWD} == {0, 1, 2, 3}
    assert any(c.planB[3] > 16 for c in R.BWD)                                # more than one group of 8 workgroups
    assert all(-(-c.planB[3] // 4) < c.planB[4] for c in R.BWD)               # every case has workgroups without a unit
    assert any(c.planA[2] == 2 and steps(c)[1] % 2 == 1 and c.planA[1] > 1 for c in R.BWD)
    assert any(c.planA[1] == 1 and c.planA[2] == 5 for c in R.BWD)


def test_the_refusals_are_refused():
    L = _lib()
    ok = R._f('ok', 2, 9, 9, 16, 96, 2, None)
    assert query(L, 0, ok)[7] == 1 and query(L, 1, ok)[7] == 1 and query(L, 2, ok)[7] == 1
    Ho, Wo, pt, pl = R.geom(ok)
    assert query(L, 0, R._f('n2049', 2049, 1, 1, 16, 16, 1, None)) == [0] * 8           # N * nseg > 2048 statistic rows
    assert query(L, 0, R._f('n2048', 2048, 1, 1, 16, 16, 1, None))[6] == 2048
    for K, C in ((20, 96), (16, 100), (16, 1040)):
        assert query(L, 0, ok, K=K, C=C) == [0] * 8, (K, C)
        assert not L.irb_supported(2, 9, 9, K, C, 3, 2, 1, pt, pl, Ho, Wo)
    assert query(L, 0, ok, geo=(Ho, Wo, 2, pl)) == [0] * 8 and query(L, 0, ok, geo=(Ho, Wo, pt, 2)) == [0] * 8   # pad 2
    assert not L.irb_supported(2, 9, 9, 16, 96, 3, 2, 2, pt, pl, Ho, Wo)                                        # rate 2
    assert not L.irb_supported(2, 9, 9, 16, 96, 5, 2, 1, pt, pl, Ho, Wo)
    for which in (1, 2):                                                                                        # backward: C = 6K only
        assert query(L, which, ok, C=64) == [0] * 8 and query(L, which, ok, K=24, C=96) == [0] * 8
    assert query(L, 0, ok, C=64)[7] == 1
    with pytest.raises(Exception):
        query(L, 3, ok)


# every instantiation the host code can launch (irb_fwd_launch, irb_bwd_sums_launch, irb_bwd_data_launch): a literal table
LAUNCHABLE = """
irb_fwd<16,1,1,fast> irb_fwd<16,1,1,generic> irb_fwd<16,1,2,fast> irb_fwd<16,1,2,generic>
irb_fwd<16,2,1,fast> irb_fwd<16,2,1,generic> irb_fwd<16,2,2,fast> irb_fwd<16,2,2,generic>
irb_fwd<16,3,1,fast> irb_fwd<16,3,1,generic> irb_fwd<16,3,2,fast> irb_fwd<16,3,2,generic>
irb_fwd<24,1,1,fast> irb_fwd<24,1,1,generic> irb_fwd<24,1,2,fast> irb_fwd<24,1,2,generic>
irb_fwd<24,2,1,fast> irb_fwd<24,2,1,generic> irb_fwd<24,2,2,fast> irb_fwd<24,2,2,generic>
irb_fwd<24,3,1,fast> irb_fwd<24,3,1,generic> irb_fwd<24,3,2,fast> irb_fwd<24,3,2,generic>
irb_fwd<32,1,1,fast> irb_fwd<32,1,1,generic> irb_fwd<32,1,2,fast> irb_fwd<32,1,2,generic>
irb_fwd<32,2,1,fast> irb_fwd<32,2,1,generic> irb_fwd<32,2,2,fast> irb_fwd<32,2,2,generic>
irb_fwd<32,3,1,fast> irb_fwd<32,3,1,generic> irb_fwd<32,3,2,fast> irb_fwd<32,3,2,generic>
irb_bwd_sums<16,1,fast> irb_bwd_sums<16,1,generic> irb_bwd_sums<16,2,fast> irb_bwd_sums<16,2,generic>
irb_bwd_sums<24,1,fast> irb_bwd_sums<24,1,generic> irb_bwd_sums<24,2,fast> irb_bwd_sums<24,2,generic>
irb_bwd_sums<32,1,fast> irb_bwd_sums<32,1,generic> irb_bwd_sums<32,2,fast> irb_bwd_sums<32,2,generic>
irb_bwd_data<16,1,fast> irb_bwd_data<16,1,generic> irb_bwd_data<16,2,fast> irb_bwd_data<16,2,generic>
irb_bwd_data<24,1,fast> irb_bwd_data<24,1,generic> irb_bwd_data<24,2,fast> irb_bwd_data<24,2,generic>
irb_bwd_data<32,1,fast> irb_bwd_data<32,1,generic> irb_bwd_data<32,2,fast> irb_bwd_data<32,2,generic>
""".split()


def test_every_launchable_instantiation_is_named_by_a_row(knobs):
    L = _lib()
    assert len(LAUNCHABLE) == len(set(LAUNCHABLE)) == 36 + 12 + 12
    reached = set()
    for c in R.FWD:
        knobs(c)
        reached.add(R.fwd_kernel(c, query(L, 0, c)[0]))          # the CT the launch would take, not the CT the row asks for
    for c in R.BWD:
        reached |= set(R.bwd_kernels(c))
    assert set(LAUNCHABLE) - reached == set(), sorted(set(LAUNCHABLE) - reached)
    assert reached - set(LAUNCHABLE) == set(), sorted(reached - set(LAUNCHABLE))
    # every generic activation pair and every pointer form of the fast pair is there, in both directions where it applies
    assert {c.pair for c in R.FWD} == set(R.GEN.values()) | {R.FAST} and {c.affine for c in R.FWD} == {'both', 'scale', 'none'}
    assert {c.pair for c in R.BWD} == set(R.GEN.values()) | {R.FAST}
    assert {c.layout for c in R.FWD} == {'contig', 'view', 'view2'} and {c.layout for c in R.BWD} == {'contig', 'view'}


@pytest.mark.parametrize('c', R.FWD, ids=lambda c: c.name)
def test_float32_forward_stays_inside_its_bound(c):
    d = R.inputs(c)
    y, yb = R.fwd_ref(d, c)
    assert np.isfinite(yb).all() and (yb >= 0).all()
    for order in (1, -1):
        y32 = R.fwd32(d, c, order)
        R.inside(y32, y, yb, '%s forward order %d' % (c.name, order))
        val, bound = R.stat_ref(y32)
        tot = np.stack([R._sum32(y32, order), R._sum32(R.f32(y32 * y32), order)])
        R.inside(tot, val, bound, '%s statistic rows order %d' % (c.name, order))


@pytest.mark.parametrize('c', R.BWD, ids=lambda c: c.name)
def test_float32_backward_stays_inside_its_bound_and_the_ambiguity_cap_holds(c):
    d = R.inputs(c)
    a = R.pass_a_ref(d, c)
    # a condition on the float64 reference alone: the pixels set aside as undecided at a kink
    assert a['share'] <= R.AMBIGUOUS_CAP, (c.name, a['share'])
    for accumulate in (False, True):
        b = R.pass_b_ref(d, c, accumulate, True, a)
        for order in (1, -1):
            got = R.bwd32(d, c, order, accumulate, True)
            what = '%s order %d accumulate %d: ' % (c.name, order, accumulate)
            R.inside(got['gwdw'], a['gwdw'], a['gwdw_b'], what + 'gwdw')
            R.inside(got['rows'], a['rows'], a['rows_b'], what + 'BN1 rows', a['rows_s'])
            R.inside(got['gw1'], b['gw1'], b['gw1_b'], what + 'gw1', b['gw1_s'])
            R.inside(got['gx'], b['gx'], b['gx_b'], what + 'gx', b['gx_s'])
            R.inside(got['front'], b['front'], b['front_b'], what + 'front rows', b['front_s'])
