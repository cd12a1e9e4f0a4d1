"""The fp32 depthwise family (csrc/dwconv.hip) per element at every dispatch edge, against float64.

Every case of CASES names the decomposition it is meant to reach and WANT holds what dl3p_dw_plan_query reports for it (kind, strip
width, band height, bands) for the forward, the data gradient and the weight gradient, plus what dl3p_dw_upsampled_input_supported and
dl3p_dwconv2d_bwd_weight_bn_supported answer.  test_case_table_reaches_its_decompositions (CPU, nothing is launched) holds the table
to the dispatcher, test_every_launchable_instantiation_is_reached holds the table to the list of kernels the host code can launch.

Operands sit in buffers of their own (Plane): an image row and a pixel of canaries before the first row and after the last one and, for the 'view'
layout (row stride C + 8, the view four floats in), canary channels beside every row.  Inputs carry NaN / +Inf / -Inf there, outputs
one sentinel bit pattern that must come back bit-identical.  Every output element is compared with float64 under the per-element bound
of fwd_ref / dgrad_ref / wgrad_ref below: u * (roundings * sum of |terms|), the roundings counted from the kernel's own operations.
There is no tensor-scale term and no constant fitted to a kernel's output.  test_float32_reference_stays_inside_its_bound (CPU)
evaluates the same operations in float32 in two summation orders on the suite's own inputs and holds both to the bound.

The kernels that only environment variables select run in child interpreters (the switches are read once per process), one after
another; each child applies the float64 bound itself and sends SHA-256 digests back.  y of EVERY forward-role decomposition is one
chain fma(a[ky][kx], w[ky][kx], acc) from acc = 0 with ky, kx ascending (dw_fwd_seg, dw5_rows -- input row j meets output row j - ky,
so ky ascends --, the gather; the residue-class kernels skip exactly the taps that the others multiply by an exact zero), so y is
held bitwise across DL3P_DW_FAST_ROWS, DL3P_DW_NT, DL3P_DW5_ROWS, DL3P_DW_LAT3 and DL3P_DW_BALANCE; the statistic rows are held
bitwise where the work split is the same (FAST_ROWS, NT); the weight gradient of DL3P_DW5_WROWS sums the pixels in another order and
is held to the bound only."""
import collections
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from conftest import load_pkg  # noqa: E402
from layer_walk import _taps  # noqa: E402

gpu = pytest.mark.gpu
U = 2.0 ** -24                      # one fp32 rounding, relative
NONE, RELU, RELU6, HSWISH, HSIGMOID = 0, 1, 2, 3, 4
SIXTH = float(np.float32(1.0) / np.float32(6.0))
IN_CANARY = (0x7FC00A5A, 0x7F800000, -0x00800000)      # int32 bits: a NaN with a payload, +Inf, -Inf
SENTINEL = 0x7FA5C3E1                                  # outputs: one NaN bit pattern no kernel produces
BEFORE = AFTER = 66                                    # guard pixels around every operand: a whole image row of the widest map + 1


def _lib():
    return load_pkg('_lib').lib()


# ---------------------------------------------------------------------------------------------------------------- the case table
Case = collections.namedtuple('Case', 'name N H W C k s r pad opts')


def _c(name, N, H, W, C, k=3, s=1, r=1, pad='same', **opts):
    return Case(name, N, H, W, C, k, s, r, pad, tuple(sorted(opts.items())))


CASES = [
    # 3x3 stride 1, strips of 4: Wo with every remainder mod 4
    _c('s1_w16', 2, 9, 16, 8), _c('s1_w17', 2, 9, 17, 8), _c('s1_w18', 2, 9, 18, 8), _c('s1_w19', 2, 9, 19, 8),
    # ... strips of 2 (set_option dw_tw): both remainders
    _c('s1_tw2_w17', 2, 9, 17, 8, dw_tw=2), _c('s1_tw2_w18', 2, 9, 18, 8, dw_tw=2),
    # ceil(Wo / rate) on both sides of 4 (window kernel / gather), H = 1 with W = 4, Wo < 4
    _c('r2_w8_window', 2, 11, 8, 8, r=2), _c('r2_w6_gather', 2, 11, 6, 8, r=2),
    _c('h1_w4', 3, 1, 4, 4), _c('w3_gather', 2, 5, 3, 8),
    # rates 1, 2, 3, 6 with Ho and Wo ragged against the rate: sub-lattices of unequal row and column counts
    _c('r1_ragged', 2, 13, 19, 16), _c('r2_ragged', 2, 13, 19, 16, r=2), _c('r3_ragged', 2, 14, 17, 16, r=3),
    _c('r6_ragged', 1, 27, 29, 16, r=6), _c('r2_tw2_ragged', 2, 13, 19, 16, r=2, dw_tw=2),
    # row bands (dw_maxth / dw_want): one band, two bands of 21 rows (10 + 11), four (5 + 5 + 5 + 6), one band per row
    _c('band_1', 3, 21, 12, 128, dw_maxth=32, dw_want=1), _c('band_2', 3, 21, 12, 128, dw_maxth=16, dw_want=1),
    _c('band_4', 3, 21, 12, 128, dw_maxth=6, dw_want=1), _c('band_uh', 3, 21, 12, 128, dw_want=1000000),
    _c('band_4_tw2_r2', 2, 26, 21, 128, r=2, dw_maxth=4, dw_want=1, dw_tw=2),
    # enough work for multi-row bands without a pin (one pixel lane per workgroup at C = 1024); 41 rows: pick_band's bands of 4
    # (DL3P_DW_BALANCE = 0 | 1) end past the last row
    _c('band_default', 3, 41, 64, 1024),
    # 3x3 stride 2: even and odd maps, 'same', (1, 1, 1, 1) and (0, 1, 0, 1), Wo = 4 and Wo = 3
    _c('s2_same_odd', 2, 11, 13, 16, s=2), _c('s2_same_even', 2, 12, 14, 16, s=2),
    _c('s2_p1111', 2, 12, 10, 16, s=2, pad=(1, 1, 1, 1)), _c('s2_p0101_wo4', 2, 11, 9, 16, s=2, pad=(0, 1, 0, 1)),
    _c('s2_wo4', 2, 7, 8, 16, s=2), _c('s2_wo3_gather', 2, 9, 6, 16, s=2),
    _c('s2_band_3', 3, 19, 24, 128, s=2, dw_maxth=4, dw_want=1),
    # gather: stride 2 with rate 2, rate >= H (Xception 257 x 257 at output stride 8: ASPP rate 36 on 33 x 33), rate == H
    _c('s2_r2_gather', 2, 13, 15, 16, s=2, r=2), _c('r36_on_33', 1, 33, 33, 16, r=36), _c('r_eq_h', 2, 7, 7, 16, r=7),
    # residue-class kernels on both sides of 2 * rate >= H and 3 * rate >= H, H != W, rate = H - 1
    _c('lat2_2r_eq_h', 2, 12, 12, 16, r=6), _c('lat3_2r_eq_h_minus_1', 2, 13, 13, 16, r=6),
    _c('lat3_3r_eq_h', 2, 12, 12, 16, r=4), _c('window_3r_eq_h_minus_1', 2, 13, 13, 16, r=4),
    _c('lat2_h_ne_w', 2, 11, 9, 16, r=6), _c('lat3_h_ne_w', 2, 14, 10, 16, r=5), _c('lat3_h_over_2r', 2, 13, 9, 16, r=6),
    _c('lat2_r_eq_h_minus_1', 2, 9, 9, 16, r=8), _c('gather_h_over_3r', 2, 14, 10, 16, r=4),
    # 5x5: sub-lattice width 40 / 41 (strips of 4 / 2), a map smaller than the window, stride 2, rate 2, the one-lane LDS slab
    # plan (C / 4 = 67, a prime above 64), several slabs (C / 4 = 120 -> 15 slabs of 8 lanes)
    _c('k5_uw40', 1, 7, 40, 8, k=5), _c('k5_uw41', 1, 7, 41, 8, k=5), _c('k5_small_map', 2, 3, 4, 8, k=5),
    _c('k5_s2', 2, 11, 13, 16, k=5, s=2), _c('k5_r2', 2, 13, 19, 16, k=5, r=2), _c('k5_c268', 1, 7, 9, 268, k=5),
    _c('k5_c480', 1, 6, 9, 480, k=5), _c('k5_s2_wo3_gather', 2, 6, 5, 8, k=5, s=2),
    _c('k5_s2_r2_gather', 2, 13, 15, 8, k=5, s=2, r=2), _c('k5_bands', 3, 21, 12, 128, k=5, dw_maxth=6, dw_want=1),
    # channels and batch: C = 4, five channel slabs from pick_lanes (C = 1280), C = 2052 (nine slabs of 57 lanes), N = 1 and 3
    _c('c4_n3', 3, 5, 6, 4), _c('c1280_n3', 3, 6, 7, 1280), _c('c2052_n1', 1, 5, 9, 2052), _c('c2052_s2_n1', 1, 9, 9, 2052, s=2),
]
BY_NAME = {c.name: c for c in CASES}
assert all(c.W + 1 <= AFTER for c in CASES)

# what the dispatcher reports: forward, data gradient, weight gradient as 'kind/tw/th/nbands' (kind 0 gather, 1 stride-1 window, 2
# stride-2 window, 3 residue classes, 4 the data gradient's own stride-2 quads / strided gather), then up (forward), up (weight
# gradient), fold (dl3p_dwconv2d_bwd_weight_bn_supported)
WANT = {
    's1_w16': ('1/4/1/9', '1/4/1/9', '1/4/1/9', 1, 1, 1),
    's1_w17': ('1/4/1/9', '1/4/1/9', '1/4/1/9', 1, 1, 1),
    's1_w18': ('1/4/1/9', '1/4/1/9', '1/4/1/9', 1, 1, 1),
    's1_w19': ('1/4/1/9', '1/4/1/9', '1/4/1/9', 1, 1, 1),
    's1_tw2_w17': ('1/2/1/9', '1/2/1/9', '1/2/1/9', 1, 1, 1),
    's1_tw2_w18': ('1/2/1/9', '1/2/1/9', '1/2/1/9', 1, 1, 1),
    'r2_w8_window': ('1/4/1/6', '1/4/1/6', '1/4/1/6', 0, 0, 1),
    'r2_w6_gather': ('0/0/1/11', '0/0/1/11', '0/0/1/11', 0, 0, 0),
    'h1_w4': ('1/4/1/1', '1/4/1/1', '1/4/1/1', 1, 1, 1),
    'w3_gather': ('0/0/1/5', '0/0/1/5', '0/0/1/5', 0, 0, 0),
    'r1_ragged': ('1/4/1/13', '1/4/1/13', '1/4/1/13', 1, 1, 1),
    'r2_ragged': ('1/4/1/7', '1/4/1/7', '1/4/1/7', 0, 0, 1),
    'r3_ragged': ('1/4/1/5', '1/4/1/5', '1/4/1/5', 0, 0, 1),
    'r6_ragged': ('1/4/1/5', '1/4/1/5', '1/4/1/5', 0, 0, 1),
    'r2_tw2_ragged': ('1/2/1/7', '1/2/1/7', '1/2/1/7', 0, 0, 1),
    'band_1': ('1/4/21/1', '1/4/21/1', '1/4/21/1', 1, 1, 1),
    'band_2': ('1/4/11/2', '1/4/11/2', '1/4/11/2', 1, 1, 1),
    'band_4': ('1/4/6/4', '1/4/6/4', '1/4/6/4', 1, 1, 1),
    'band_uh': ('1/4/1/21', '1/4/1/21', '1/4/1/21', 1, 1, 1),
    'band_4_tw2_r2': ('1/2/4/4', '1/2/4/4', '1/2/4/4', 0, 0, 1),
    'band_default': ('1/4/6/8', '1/4/6/8', '1/4/6/8', 1, 1, 1),
    's2_same_odd': ('2/2/1/6', '4/0/0/0', '2/2/1/6', 0, 0, 1),
    's2_same_even': ('2/2/1/6', '4/0/0/0', '2/2/1/6', 0, 0, 1),
    's2_p1111': ('2/2/1/6', '4/0/0/0', '2/2/1/6', 0, 0, 1),
    's2_p0101_wo4': ('2/2/1/5', '4/0/0/0', '2/2/1/5', 0, 0, 1),
    's2_wo4': ('2/2/1/4', '4/0/0/0', '2/2/1/4', 0, 0, 1),
    's2_wo3_gather': ('0/0/1/5', '4/0/0/0', '0/0/1/5', 0, 0, 0),
    's2_band_3': ('2/2/4/3', '4/0/0/0', '2/2/4/3', 0, 0, 1),
    's2_r2_gather': ('0/0/1/7', '4/0/0/0', '0/0/1/7', 0, 0, 0),
    'r36_on_33': ('0/0/1/33', '0/0/1/33', '0/0/1/33', 0, 0, 0),
    'r_eq_h': ('0/0/1/7', '0/0/1/7', '0/0/1/7', 0, 0, 0),
    'lat2_2r_eq_h': ('3/0/1/6', '3/0/1/6', '0/0/1/12', 0, 0, 0),
    'lat3_2r_eq_h_minus_1': ('3/0/1/6', '3/0/1/6', '0/0/1/13', 0, 0, 0),
    'lat3_3r_eq_h': ('3/0/1/4', '3/0/1/4', '0/0/1/12', 0, 0, 0),
    'window_3r_eq_h_minus_1': ('1/4/1/4', '1/4/1/4', '1/4/1/4', 0, 0, 1),
    'lat2_h_ne_w': ('3/0/1/6', '3/0/1/6', '0/0/1/11', 0, 0, 0),
    'lat3_h_ne_w': ('3/0/1/5', '3/0/1/5', '0/0/1/14', 0, 0, 0),
    'lat3_h_over_2r': ('3/0/1/6', '3/0/1/6', '0/0/1/13', 0, 0, 0),
    'lat2_r_eq_h_minus_1': ('3/0/1/8', '3/0/1/8', '0/0/1/9', 0, 0, 0),
    'gather_h_over_3r': ('0/0/1/14', '0/0/1/14', '0/0/1/14', 0, 0, 0),
    'k5_uw40': ('1/4/1/7', '1/4/1/7', '1/2/1/7', 0, 0, 0),
    'k5_uw41': ('1/2/1/7', '1/2/1/7', '1/2/1/7', 0, 0, 0),
    'k5_small_map': ('1/4/1/3', '1/4/1/3', '1/2/1/3', 0, 0, 0),
    'k5_s2': ('2/1/1/6', '4/0/0/0', '0/0/1/6', 0, 0, 0),
    'k5_r2': ('1/4/1/7', '1/4/1/7', '1/2/1/7', 0, 0, 0),
    'k5_c268': ('1/4/1/7', '1/4/1/7', '1/2/1/7', 0, 0, 0),
    'k5_c480': ('1/4/1/6', '1/4/1/6', '1/2/1/6', 0, 0, 0),
    'k5_s2_wo3_gather': ('0/0/1/3', '4/0/0/0', '0/0/1/3', 0, 0, 0),
    'k5_s2_r2_gather': ('0/0/1/7', '4/0/0/0', '0/0/1/7', 0, 0, 0),
    'k5_bands': ('1/4/6/4', '1/4/6/4', '1/2/6/4', 0, 0, 0),
    'c4_n3': ('1/4/1/5', '1/4/1/5', '1/4/1/5', 1, 1, 1),
    'c1280_n3': ('1/4/1/6', '1/4/1/6', '1/4/1/6', 1, 1, 1),
    'c2052_n1': ('1/4/1/5', '1/4/1/5', '1/4/1/5', 1, 1, 1),
    'c2052_s2_n1': ('2/2/1/5', '4/0/0/0', '2/2/1/5', 0, 0, 1),
}


def geom(c):
    """Ho, Wo, pad_t, pad_l (TF SAME: the odd unit of padding goes to the end)"""
    def same(n):
        ke = c.k + (c.k - 1) * (c.r - 1)
        out = -(-n // c.s)
        return out, max((out - 1) * c.s + ke - n, 0) // 2
    if c.pad == 'same':
        (Ho, pt), (Wo, pl) = same(c.H), same(c.W)
        return Ho, Wo, pt, pl
    pt, pb, pl, pr = c.pad
    ke = c.k + (c.k - 1) * (c.r - 1)
    return (c.H + pt + pb - ke) // c.s + 1, (c.W + pl + pr - ke) // c.s + 1, pt, pl


class options:
    """a case's dl3p_set_option pins for the time of its launches and queries (0 restores each default)"""

    def __init__(self, L, c):
        self.L, self.opts = L, c.opts

    def __enter__(self):
        for k, v in self.opts:
            self.L.set_option(k.encode(), v)

    def __exit__(self, *a):
        for k, _ in self.opts:
            self.L.set_option(k.encode(), 0)


def plan(L, role, c):
    """[kind, tw, th, nbands, nbx, from table] (call inside `options`)"""
    Ho, Wo, pt, pl = geom(c)
    out = (ctypes.c_int * 6)()
    L.dw_plan_query(role, c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo, out)
    return list(out)


def reported(L, c):
    Ho, Wo, pt, pl = geom(c)
    with options(L, c):
        f, d, w = ('%d/%d/%d/%d' % tuple(plan(L, role, c)[:4]) for role in (0, 1, 3))
        up = [L.dw_upsampled_input_supported(role, c.N, c.H, c.W, c.C, 4, c.k, c.s, c.r, pt, pl, Ho, Wo) for role in (0, 1)]
        fold = L.dwconv2d_bwd_weight_bn_supported(c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo)
    return (f, d, w, up[0], up[1], fold)


# ---- which kernel instantiation a launch is (the launch switches of csrc/dwconv.hip -- launch_fwd / launch_fwd_pro for a planned
# forward or flipped problem, launch_bwdw / launch_bwdw_bna behind dw_plan_wgrad, the data-gradient entries' own stride > 1 launches
# -- restated over the plan query); env: the DL3P_* switches of the process
def _pro_of(sc, act):
    return 2 if act != NONE else (1 if sc else 0)


def fwd_kernel(c, kind, tw, pro, env, flip=False, bnb=False, up=False, nt=True):
    k = c.k
    s = 1 if flip else c.s
    if bnb:
        return 'dw_fwd_seg<3,%d,1,0,BNB>' % tw
    fast = pro != 0 and not flip and nt and int(env.get('DL3P_DW_FAST_ROWS', 1)) >= 2 and int(env.get('DL3P_DW_NT', 3)) & 1
    if k == 5:
        if kind == 1:
            uw = -(-(c.W if flip else geom(c)[1]) // c.r)
            v = int(env.get('DL3P_DW5_ROWS', -1))
            rows_tw = v if v >= 0 else (4 if uw <= 40 else 2)
            if rows_tw in (2, 4):
                return 'dw5_rows<%d,%d>' % (rows_tw, pro)
            return 'dw_fwd_seg<5,2,1,%d%s>' % (pro, ',FAST' if fast else '')
        if kind == 2:
            return 'dw_fwd_seg<5,1,2,%d%s>' % (pro, ',FAST' if fast else '')
        return 'dw_fwd_gather<5,%d>' % pro
    if up:
        return 'dw_fwd_seg<3,%d,1,2,UP>' % tw
    if kind in (1, 2):
        return 'dw_fwd_seg<3,%d,%d,%d%s>' % (tw, s, pro, ',FAST' if fast else '')
    if kind == 3:
        lat3 = 2 * c.r < max(c.H, c.W)
        if lat3 and int(env.get('DL3P_DW_LAT3', 1)) == 0:
            return 'dw_fwd_gather<3,%d>' % pro
        return 'dw_fwd_lattice%d<%d>' % (3 if lat3 else 2, pro)
    return 'dw_fwd_gather<3,%d>' % pro


def dgrad_kernel(c, kind, tw, env, bnb=False):
    if c.s == 1:          # (the sums are folded into the 3x3 window kernel only; elsewhere: plain data gradient + dl3p_bn_bwd_reduce)
        return fwd_kernel(c, kind, tw, 0, env, flip=True, bnb=bnb and c.k == 3 and kind == 1)
    if c.s == 2 and c.r == 1:
        return 'dw_bwd_data_s2<%d%s>' % (c.k, ',BNB' if (bnb and c.k == 3) else '')
    return 'dw_bwd_data_strided<%d>' % c.k


def wgrad_kernel(c, kind, tw, pro, env, fold=False, up=False):
    if up:
        return 'dw_bwd_weight_seg<3,%d,1,2,%sUP>' % (tw, 'BNA,' if fold else '')
    if fold:
        return 'dw_bwd_weight_seg<3,%d,%d,%d,BNA>' % (tw, c.s, pro)
    if c.k == 5:
        wrows = int(env.get('DL3P_DW5_WROWS', 2))
        if c.s == 1 and wrows > 0 and kind == 1:
            return 'dw5_wgrad_rows<%d,%d>' % (1 if wrows == 1 else 2, pro)
        return 'dw_bwd_weight<5,%d>' % pro
    if kind in (1, 2):
        return 'dw_bwd_weight_seg<3,%d,%d,%d>' % (tw, c.s, pro)
    return 'dw_bwd_weight<3,%d>' % pro


def launchable():
    """every instantiation the host code of csrc/dwconv.hip names in a launch"""
    ks = set()
    for pro in (0, 1, 2):
        for tw, s in ((4, 1), (2, 1), (2, 2)):
            ks.add('dw_fwd_seg<3,%d,%d,%d>' % (tw, s, pro))
            ks.add('dw_bwd_weight_seg<3,%d,%d,%d>' % (tw, s, pro))
            ks.add('dw_bwd_weight_seg<3,%d,%d,%d,BNA>' % (tw, s, pro))
            if pro:
                ks.add('dw_fwd_seg<3,%d,%d,%d,FAST>' % (tw, s, pro))
        for t in ('dw_fwd_seg<5,2,1,%d>', 'dw_fwd_seg<5,1,2,%d>', 'dw5_rows<2,%d>', 'dw5_rows<4,%d>', 'dw_fwd_gather<3,%d>',
                  'dw_fwd_gather<5,%d>', 'dw_fwd_lattice2<%d>', 'dw_fwd_lattice3<%d>', 'dw_bwd_weight<3,%d>', 'dw_bwd_weight<5,%d>',
                  'dw5_wgrad_rows<1,%d>', 'dw5_wgrad_rows<2,%d>'):
            ks.add(t % pro)
        if pro:
            ks.add('dw_fwd_seg<5,2,1,%d,FAST>' % pro)
            ks.add('dw_fwd_seg<5,1,2,%d,FAST>' % pro)
    for tw in (2, 4):
        ks |= {'dw_fwd_seg<3,%d,1,0,BNB>' % tw, 'dw_fwd_seg<3,%d,1,2,UP>' % tw, 'dw_bwd_weight_seg<3,%d,1,2,UP>' % tw,
               'dw_bwd_weight_seg<3,%d,1,2,BNA,UP>' % tw}
    ks |= {'dw_bwd_data_s2<3>', 'dw_bwd_data_s2<5>', 'dw_bwd_data_s2<3,BNB>', 'dw_bwd_data_strided<3>', 'dw_bwd_data_strided<5>'}
    return ks


# ------------------------------------------------------------------------------------------------ prologues and their roundings
# name -> (has scale / shift, activation).  'act_only' is the PRO == 2 kernel without a scale pointer.
PROS = collections.OrderedDict([('none', (False, NONE)), ('affine', (True, NONE)), ('relu', (True, RELU)), ('relu6', (True, RELU6)),
                                ('hswish', (True, HSWISH)), ('hsigmoid', (True, HSIGMOID)), ('act_only', (False, RELU6))])
# The prologue a = act(fmaf(x, scale, shift)) (common.h act_apply), its error against the float64 value, per element:
#  * the fma rounds once: u * |x*scale + shift| <= u * p with p = |x*scale| + |shift|; the activation passes that on times its
#    Lipschitz constant L (ReLU, ReLU6: 1 and exact on the rounded value; hard-swish: max |d/dv v*relu6(v+3)/6| = 1.5 at v = 3;
#    hard-sigmoid: 1/6, counted as 1)                                                                      -> N_PRO = L, times p
#  * hard-sigmoid t = min(max(v + 3, 0), 6) * fl(1/6): the add rounds once (u * |v + 3| = 6 u t inside the clamp, nothing where the
#    clamp holds, rounding being monotone), fl(1/6) is off by at most u, the product rounds once          -> 3 roundings of |a|
#  * hard-swish v * t: those three on t and one for the product                                           -> 4 roundings of |a|
N_PRO = {NONE: 1.0, RELU: 1.0, RELU6: 1.0, HSWISH: 1.5, HSIGMOID: 1.0}
N_ACT = {NONE: 0, RELU: 0, RELU6: 0, HSWISH: 4, HSIGMOID: 3}


def act64(v, act):
    if act == NONE:
        return v
    if act == RELU:
        return v.clamp_min(0)
    if act == RELU6:
        return v.clamp(0, 6)
    t = (v + 3).clamp(0, 6) / 6
    return v * t if act == HSWISH else t


def pro_terms(x, sc, sh, act):
    """float64 a = act(x*scale + shift) from the exact fp32 operands, and p = |x*scale| + |shift| (0 without an affine)"""
    x = x.double()
    if sc is None:
        return act64(x, act), (x.abs() if act != NONE else torch.zeros_like(x))
    xs = x * sc.double()
    return act64(xs + sh.double(), act), xs.abs() + sh.double().abs()


def conv64(a, w, c):
    Ho, Wo, pt, pl = geom(c)
    out = 0
    for ky, kx, v in _taps(a, c.k, c.s, c.r, pt, pl, Ho, Wo):
        out = out + v * w[ky, kx]
    return out


def fwd_ref(x, w, sc, sh, act, c, ap=None):
    """value and bound of y: k*k FMAs from zero round k*k times (+ 1: second order and the float64 reference itself) -> (k*k + 1) * S
    with S = conv(|a|, |w|); the prologue's roundings reach y through |w|: N_ACT * S + N_PRO * P, P = conv(p, |w|)"""
    a, p = ap or pro_terms(x, sc, sh, act)
    w = w.double()
    S, P = conv64(a.abs(), w.abs(), c), conv64(p, w.abs(), c)
    n_pro = 0.0 if sc is None else N_PRO[act]          # no scale pointer: no fma, the activation works on x itself
    return conv64(a, w, c), U * ((c.k * c.k + 1 + N_ACT[act]) * S + n_pro * P)


def scatter64(dy, w, c, fma=None, order=1):
    """conv transpose: gx[n, oy*s - pt + ky*r, ox*s - pl + kx*r] += w[ky, kx] * dy[n, oy, ox]"""
    Ho, Wo, pt, pl = geom(c)
    Hp = max((Ho - 1) * c.s + (c.k - 1) * c.r + 1, pt + c.H)
    Wp = max((Wo - 1) * c.s + (c.k - 1) * c.r + 1, pl + c.W)
    gp = torch.zeros((c.N, Hp, Wp, c.C), dtype=dy.dtype, device=dy.device)
    for t in list(range(c.k * c.k))[::order]:
        ky, kx = divmod(t, c.k)
        v = gp[:, ky * c.r: ky * c.r + (Ho - 1) * c.s + 1: c.s, kx * c.r: kx * c.r + (Wo - 1) * c.s + 1: c.s]
        v.copy_(v + dy * w[ky, kx] if fma is None else fma(dy, w[ky, kx].expand_as(dy), v))
    return gp[:, pt:pt + c.H, pl:pl + c.W]


def dgrad_ref(dy, w, c, base=None):
    """at most k*k FMAs per input pixel (the flipped window kernels, the gather, the stride-2 quads): (k*k + 1) * S; accumulating
    forms add the old value with one more rounding of |sum| + |old| <= S + |old|"""
    dy, w = dy.double(), w.double()
    val, S = scatter64(dy, w, c), scatter64(dy.abs(), w.abs(), c)
    if base is None:
        return val, U * (c.k * c.k + 1) * S
    return val + base.double(), U * ((c.k * c.k + 2) * S + base.double().abs())


def wgrad_ref(x, dy, sc, sh, act, c, ddy=None, ap=None):
    """gw[ky, kx, c] sums n = N * Ho * Wo products fma(a, dy, acc): any order of an n-term sum stays within n roundings of the sum of
    |terms| (zeros added by idle lanes and by the slab reduction are exact) -> (n + N_ACT) * S + N_PRO * P with S = sum |a| |dy|,
    P = sum p |dy|.  ddy: a per-element error bound of dy itself (the folded form's dz), reaching gw through sum |a| * ddy"""
    Ho, Wo, pt, pl = geom(c)
    a, p = ap or pro_terms(x, sc, sh, act)
    dy = dy.double()
    n = c.N * Ho * Wo
    n_pro = 0.0 if sc is None else N_PRO[act]          # no scale pointer: no fma, the activation works on x itself
    val = torch.zeros((c.k, c.k, c.C), dtype=torch.float64, device=x.device)
    bound = torch.zeros_like(val)
    for (ky, kx, va), (_, _, vp) in zip(_taps(a, c.k, c.s, c.r, pt, pl, Ho, Wo), _taps(p, c.k, c.s, c.r, pt, pl, Ho, Wo)):
        val[ky, kx] = (va * dy).sum((0, 1, 2))
        bound[ky, kx] = U * ((n + 1 + N_ACT[act]) * (va.abs() * dy.abs()).sum((0, 1, 2)) + n_pro * (vp * dy.abs()).sum((0, 1, 2)))
        if ddy is not None:
            bound[ky, kx] += (va.abs() * ddy).sum((0, 1, 2))
    return val, bound


def fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in float64, one rounding to float64 and one to fp32 (the double rounding moves a
    result by at most 2^-29 of an ulp, inside the '+ 1' of every bound)"""
    return (a.double() * b.double() + c.double()).float()


def grad_terms(u, act):
    """act'(u) decided on the fp32 pre-activation u like the device (common.h act_grad), in float64; its magnitude m (hard-swish:
    hs + u * in can cancel -> |hs| + |u * in|) and the roundings of forming it: none for the 0 / 1 of ReLU / ReLU6 / none, hard-swish
    t = u + 3 (1), hs = clamp(t) * fl(1/6) (2), u * fl(1/6) (2), the sum (1)"""
    if act == NONE:
        one = torch.ones_like(u, dtype=torch.float64)
        return one, one, 0
    if act == RELU:
        d = (u > 0).double()
        return d, d, 0
    if act == RELU6:
        d = ((u > 0) & (u < 6)).double()
        return d, d, 0
    t = u + 3
    inside = ((t > 0) & (t < 6)).double() / 6
    hs = t.double().clamp(0, 6) / 6
    if act == HSWISH:
        return hs + u.double() * inside, hs + (u.double() * inside).abs(), 6
    return inside, inside, 1


def grad32(u, act):
    """common.h act_grad in fp32, operation for operation"""
    if act == NONE:
        return torch.ones_like(u)
    if act == RELU:
        return (u > 0).float()
    if act == RELU6:
        return ((u > 0) & (u < 6)).float()
    t = u + 3
    inside = ((t > 0) & (t < 6)).float() * SIXTH
    hs = t.clamp(0, 6) * SIXTH
    return hs + u * inside if act == HSWISH else inside


def stat_pairs(y):
    """the statistic rows of a forward launch from its own y: [(value, sum of |terms|)] and the roundings of forming one term (sum y:
    n adds; sum y^2: n fmas) -- held to (n + 1) * u * sum |terms|"""
    y = y.double()
    return [(y.sum((0, 1, 2)), y.abs().sum((0, 1, 2))), ((y * y).sum((0, 1, 2)), (y * y).sum((0, 1, 2)))], (1, 1)


def bnsum_pairs(g, z, bsc, bsh, mu, inv, act):
    """(sum g', sum g' * xhat) of a finished gradient g: g' = g * act'(u) costs the n_g roundings of act' and one of the product,
    xhat = (z - mean) * invstd two, fma(g', xhat, s) one per term"""
    g = g.double()
    d, m, n_g = grad_terms(fma32(z, bsc.expand_as(z), bsh.expand_as(z)), act)
    xh = (z.double() - mu.double()) * inv.double()
    return [((g * d).sum((0, 1, 2)), (g.abs() * m).sum((0, 1, 2))),
            ((g * d * xh).sum((0, 1, 2)), (g.abs() * m * xh.abs()).sum((0, 1, 2)))], (n_g + 2, n_g + 5)


def _totals(tot, pairs, n, extra, what):
    """fp32 sums `tot` [len(pairs)][C]: within (n + extra) roundings of the sum of |terms| (n: the number of summed terms)"""
    for i, (want, terms) in enumerate(pairs):
        _inside(tot[i], want, (n + extra[i]) * U * terms, '%s [%d]' % (what, i))


# --------------------------------------------------------------------------------------------------------- inputs (CPU, seeded)
def inputs(c, dev):
    """the operands of a case, generated on the CPU from its name (the CPU reference test and the GPU tests see the same numbers)"""
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.name.encode()))
    Ho, Wo, pt, pl = geom(c)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = dict(x=rn(c.N, c.H, c.W, c.C) * 2, w=rn(c.k, c.k, c.C) / c.k, dy=rn(c.N, Ho, Wo, c.C), base=rn(c.N, c.H, c.W, c.C),
             z=rn(c.N, c.H, c.W, c.C) * 2, zo=rn(c.N, Ho, Wo, c.C) * 2)
    d['w'][0, c.k - 1] *= 1e-3            # one low-magnitude tap, off the diagonal: its error must not hide behind the others
    sign = torch.where(torch.rand(c.C, generator=g) < 0.25, -1.0, 1.0)
    d['sc'] = (torch.rand(c.C, generator=g) + 0.5) * sign
    d['sh'] = rn(c.C) * 0.5
    d['mu'] = rn(c.C) * 0.3
    d['inv'] = torch.rand(c.C, generator=g) + 0.5
    d['bsc'] = torch.rand(c.C, generator=g) + 0.5
    d['bsh'] = rn(c.C) * 0.5
    d['coef'] = rn(3, c.C)
    d['coef'][0] = d['coef'][0].abs() + 0.5
    return {k: v.float().contiguous().to(dev) for k, v in d.items()}


def pro_args(inp, name):
    has, act = PROS[name]
    return (inp['sc'], inp['sh'], act) if has else (None, None, act)


# ------------------------------------------------------------------------------------------------------------------ CPU tests
def test_case_table_reaches_its_decompositions():
    """nothing is launched: the plan queries only run the host-side planner.  The band heights and counts of WANT are those of the
    default switches (and of the 256 CUs the planner is compiled for): with a DL3P_DW_* variable set in this process the table says
    nothing about the dispatcher, and the test is skipped"""
    pinned = [v for v in SWITCHES if v in os.environ]
    if pinned:
        pytest.skip('depthwise plan switches set in the environment: %s' % pinned)
    L = _lib()
    assert set(WANT) == set(BY_NAME)
    wrong = {c.name: (reported(L, c), WANT[c.name]) for c in CASES if reported(L, c) != WANT[c.name]}
    assert not wrong, wrong
    kinds = collections.Counter(w[0].split('/')[0] for w in WANT.values())
    assert set(kinds) == {'0', '1', '2', '3'}, kinds
    # the edges the table is built around, read back from the table itself
    assert WANT['r2_w8_window'][0].startswith('1/') and WANT['r2_w6_gather'][0].startswith('0/')
    assert WANT['s2_wo4'][0].startswith('2/') and WANT['s2_wo3_gather'][0].startswith('0/')
    assert WANT['lat3_3r_eq_h'][0].startswith('3/') and WANT['window_3r_eq_h_minus_1'][0].startswith('1/4/')
    assert WANT['k5_uw40'][0].startswith('1/4/') and WANT['k5_uw41'][0].startswith('1/2/')
    assert [WANT[n][0].split('/')[3] for n in ('band_1', 'band_2', 'band_4', 'band_uh')] == ['1', '2', '4', '21']
    assert WANT['r36_on_33'][0].startswith('0/') and WANT['r_eq_h'][0].startswith('0/')


def _reached():
    """the instantiations the GPU tests of this file launch: the case table under default switches x the prologues each role runs,
    and the children's cases under their switches"""
    L = _lib()
    got = set()
    for c in CASES:
        with options(L, c):
            pf, pd, pw = (plan(L, role, c) for role in (0, 1, 3))
        f, d, w, upf, upw, fold = WANT[c.name]
        for sc, act in PROS.values():
            got.add(fwd_kernel(c, pf[0], pf[1], _pro_of(sc, act), {}))
        got.add(dgrad_kernel(c, pd[0], pd[1], {}))
        got.add(dgrad_kernel(c, pd[0], pd[1], {}, bnb=True))
        for name in WGRAD_PROS:
            got.add(wgrad_kernel(c, pw[0], pw[1], _pro_of(*PROS[name]), {}))
            if fold:
                got.add(wgrad_kernel(c, pw[0], pw[1], _pro_of(*PROS[name]), {}, fold=True))
        if upf:
            got.add(fwd_kernel(c, pf[0], pf[1], 2, {}, up=True))
        if upw:
            got.add(wgrad_kernel(c, pw[0], pw[1], 2, {}, up=True))
            got.add(wgrad_kernel(c, pw[0], pw[1], 2, {}, fold=True, up=True))
    for env in CHILD_ENVS.values():
        for name in CHILD_CASES:
            c = BY_NAME[name]
            with options(L, c):
                pf, pd, pw = (plan(L, role, c) for role in (0, 1, 3))
            # (the 5x5 strip width the query reports follows DL3P_DW5_ROWS of THIS process; fwd_kernel reads the child's switch)
            for pname in CHILD_PROS:
                got.add(fwd_kernel(c, pf[0], pf[1], _pro_of(*PROS[pname]), env))
            got.add(dgrad_kernel(c, pd[0], pd[1], env))
            kind_w = pw[0] if not (c.k == 5 and c.s == 1) else (1 if int(env.get('DL3P_DW5_WROWS', 2)) > 0 and pw[0] == 1 else 0)
            got.add(wgrad_kernel(c, kind_w, pw[1], 2, env))
            got.add(wgrad_kernel(c, kind_w, pw[1], 1, env))
            got.add(wgrad_kernel(c, kind_w, pw[1], 0, env))
    return got


def test_every_launchable_instantiation_is_reached():
    missing = launchable() - _reached()
    assert not missing, sorted(missing)


def _named_in_source():
    """the instantiations csrc/dwconv.hip names in a dl3p_launch / hipLaunchKernelGGL call, in launchable()'s spelling with the
    prologue (a template parameter of the launching function in most calls) written P"""
    import re
    src = open(os.path.join(os.path.dirname(load_pkg('_lib').__file__), 'csrc', 'dwconv.hip')).read()
    pro_at = {'dw_fwd_seg': 3, 'dw_bwd_weight_seg': 3, 'dw5_rows': 1, 'dw5_wgrad_rows': 1, 'dw_fwd_gather': 1, 'dw_fwd_lattice2': 0,
              'dw_fwd_lattice3': 0, 'dw_bwd_weight': 1}
    out = set()
    for name, args in re.findall(r'(?:dl3p_launch\(|hipLaunchKernelGGL\(\()(dw5?_\w+)<([^>]*)>', src):
        a = [v.strip() for v in args.split(',')]
        if name in pro_at:
            a[pro_at[name]] = 'P'
        flags = {'dw_fwd_seg': (4, ('BNB', 'UP', 'FAST')), 'dw_bwd_weight_seg': (4, ('BNA', 'UP')), 'dw_bwd_data_s2': (1, ('BNB',))}.get(name)
        if flags:
            a = a[:flags[0]] + [f for f, v in zip(flags[1], a[flags[0]:]) if v == 'true']
        out.add('%s<%s>' % (name, ','.join(a)))
    return out


def test_launchable_is_what_the_source_launches():
    """launchable() is a restatement: hold it to the launch calls of csrc/dwconv.hip itself, so that a new instantiation cannot be
    missed by both lists"""
    import re
    pro_at = {'dw_fwd_seg': 3, 'dw_bwd_weight_seg': 3, 'dw5_rows': 1, 'dw5_wgrad_rows': 1, 'dw_fwd_gather': 1, 'dw_fwd_lattice2': 0,
              'dw_fwd_lattice3': 0, 'dw_bwd_weight': 1}
    mine = set()
    for k in launchable():
        name, args = re.match(r'(\w+)<(.*)>', k).groups()
        a = args.split(',')
        if name in pro_at:
            a[pro_at[name]] = 'P'
        mine.add('%s<%s>' % (name, ','.join(a)))
    assert mine == _named_in_source(), (sorted(mine - _named_in_source()), sorted(_named_in_source() - mine))


def _wsum32(a32, dy32, order):
    """sum over (n, oy, ox) of fma(a, dy, acc) in fp32, in two orders: columns first then rows then images, or rows (backwards)
    first, then columns (backwards), then images"""
    N, Ho, Wo, C = dy32.shape
    if order == 1:
        acc = torch.zeros((N, Ho, C))
        for ox in range(Wo):
            acc = fma32(a32[:, :, ox], dy32[:, :, ox], acc)
        tot = torch.zeros((N, C))
        for oy in range(Ho):
            tot = tot + acc[:, oy]
    else:
        acc = torch.zeros((N, Wo, C))
        for oy in reversed(range(Ho)):
            acc = fma32(a32[:, oy], dy32[:, oy], acc)
        tot = torch.zeros((N, C))
        for ox in reversed(range(Wo)):
            tot = tot + acc[:, ox]
    out = torch.zeros((C,))
    for n in range(N):
        out = out + tot[n]
    return out


def pro32(x, sc, sh, act):
    """the device's prologue in fp32, operation for operation"""
    v = x if sc is None else fma32(x, sc.expand_as(x), sh.expand_as(x))
    if act == NONE:
        return v
    if act == RELU:
        return v.clamp_min(0)
    if act == RELU6:
        return v.clamp(0, 6)
    t = (v + 3).clamp(0, 6) * SIXTH
    return v * t if act == HSWISH else t


def _inside(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        i = int((~ok).reshape(-1).nonzero()[0])
        raise AssertionError('%s: %d of %d elements out of bound; first at flat %d: got %r want %r (bound %.3g, err %.3g)' % (
            what, int((~ok).sum()), ok.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
            float(bound.reshape(-1)[i]), float(err.reshape(-1)[i])))
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize('c', [c for c in CASES if c.C <= 480], ids=lambda c: c.name)
def test_float32_reference_stays_inside_its_bound(c):
    """the operations of the kernels in fp32 on the CPU, each in two summation orders, against the float64 value: both inside the
    bound, so the bound is not met by the reference's own slack and not by one lucky order"""
    inp = inputs(c, 'cpu')
    Ho, Wo, pt, pl = geom(c)
    for name in PROS:
        sc, sh, act = pro_args(inp, name)
        ref, bound = fwd_ref(inp['x'], inp['w'], sc, sh, act, c)
        a32 = pro32(inp['x'], sc, sh, act)
        for order in (1, -1):
            acc = torch.zeros((c.N, Ho, Wo, c.C))
            for ky, kx, v in list(_taps(a32, c.k, c.s, c.r, pt, pl, Ho, Wo))[::order]:
                acc = fma32(v, inp['w'][ky, kx].expand_as(v), acc)
            _inside(acc, ref, bound, 'forward %s order %d' % (name, order))
        if name in WGRAD_PROS:
            wref, wbound = wgrad_ref(inp['x'], inp['dy'], sc, sh, act, c)
            for order in (1, -1):
                gw = torch.stack([_wsum32(v, inp['dy'], order) for _, _, v in _taps(a32, c.k, c.s, c.r, pt, pl, Ho, Wo)]).reshape(c.k, c.k, c.C)
                _inside(gw, wref, wbound, 'weight gradient %s order %d' % (name, order))
    ref, bound = dgrad_ref(inp['dy'], inp['w'], c)
    aref, abound = dgrad_ref(inp['dy'], inp['w'], c, base=inp['base'])
    for order in (1, -1):
        gx = scatter64(inp['dy'], inp['w'], c, fma=fma32, order=order)
        _inside(gx, ref, bound, 'data gradient order %d' % order)
        _inside(gx + inp['base'], aref, abound, 'accumulating data gradient order %d' % order)
        # the BatchNorm-backward sums of that gradient, and the statistic rows of the last forward above
        for act in (RELU6, HSWISH, NONE):
            pairs, extra = bnsum_pairs(gx, inp['z'], inp['bsc'], inp['bsh'], inp['mu'], inp['inv'], act)
            u32 = fma32(inp['z'], inp['bsc'].expand_as(gx), inp['bsh'].expand_as(gx))
            d32 = gx * grad32(u32, act)
            xh32 = (inp['z'] - inp['mu']) * inp['inv']
            _totals(torch.stack([_wsum32(d32, torch.ones_like(d32), order), _wsum32(d32, xh32, order)]), pairs, c.N * c.H * c.W, extra,
                    'BatchNorm-backward sums act %d order %d' % (act, order))
        pairs, extra = stat_pairs(acc)
        _totals(torch.stack([_wsum32(acc, torch.ones_like(acc), order), _wsum32(acc, acc, order)]), pairs, c.N * Ho * Wo, extra,
                'statistic rows order %d' % order)
    # the folded weight gradient's dz (elementwise: one order) and the UP form's lerps
    g, z, (c0, c1, c2) = inp['dy'], inp['zo'], inp['coef']
    for fa_act, affine in ((RELU6, True), (NONE, True), (HSWISH, True), (RELU, False)):
        fa_sc, fa_sh = (inp['bsc'], inp['bsh']) if affine else (None, None)
        dz, dzb = fold_ref(inp, fa_sc, fa_sh, fa_act, c)
        u32 = z if fa_sc is None else fma32(z, fa_sc.expand_as(z), fa_sh.expand_as(z))
        bC = (c0 * inp['inv']) * c2
        bD = bC * inp['mu'] - c0 * c1
        _inside(fma32(c0.expand_as(z), g * grad32(u32, fa_act), fma32(-bC.expand_as(z), z, bD.expand_as(z))), dz, dzb, 'folded dz act %d' % fa_act)
    gen = torch.Generator()
    gen.manual_seed(zlib.crc32(c.name.encode()) + 1)
    upx = torch.randn(c.N, max(1, (c.H + 2) // 4), max(1, (c.W + 1) // 3), c.C, generator=gen) * 2
    val, m4 = upsample_terms(upx, c.H, c.W)
    _inside(upsample_terms(upx, c.H, c.W, f32=True)[0], val, 6 * U * m4, 'UP lerps')


# ------------------------------------------------------------------------------------------------------- operands with canaries
class Plane:
    """a (rows, C) fp32 operand inside its own buffer: BEFORE / AFTER canary rows around it and, for 'view', 4 canary channels on
    either side of every row (ld = C + 8).  Nothing outside the buffer is ever addressed by a correct kernel."""

    def __init__(self, rows, C, layout, dev, value=None, out=None):
        lo, w = (0, C) if layout == 'contig' else (4, C + 8)
        R = rows + BEFORE + AFTER
        if (value is None) if out is None else out:
            self.bits = torch.full((R, w), SENTINEL, dtype=torch.int32, device=dev)
        else:
            pat = torch.tensor(IN_CANARY, dtype=torch.int32, device=dev)
            self.bits = pat.repeat((R * w + 2) // 3)[:R * w].reshape(R, w).contiguous()
        self.t = self.bits.view(torch.float32)[BEFORE:BEFORE + rows, lo:lo + C]
        if value is not None:
            self.t.copy_(value.reshape(rows, C))
        self.keep = self.bits.clone()
        self.ld, self.rows, self.C, self.lo = w, rows, C, lo

    @property
    def p(self):
        return self.t.data_ptr()

    def intact(self, what):
        mask = torch.ones_like(self.bits, dtype=torch.bool)
        mask[BEFORE:BEFORE + self.rows, self.lo:self.lo + self.C] = False
        bad = int((self.bits[mask] != self.keep[mask]).sum())
        assert bad == 0, '%s: %d sentinel elements beside / before / past the output changed' % (what, bad)

    def written(self, what):
        """every element of the view was stored to (the sentinel is no value a kernel produces)"""
        left = int((self.t.contiguous().view(torch.int32) == SENTINEL).sum())
        assert left == 0, '%s: %d output elements never written' % (what, left)


class Flat:
    """a flat fp32 output (statistic rows, weight-gradient slabs): `n` elements that matter, sentinels after them"""

    def __init__(self, n, dev, tail=256, total=None):
        self.n = n
        self.bits = torch.full((max(total or 0, n + tail),), SENTINEL, dtype=torch.int32, device=dev)
        self.t = self.bits.view(torch.float32)

    @property
    def p(self):
        return self.t.data_ptr()

    def intact(self, what):
        bad = int((self.bits[self.n:] != SENTINEL).sum())
        assert bad == 0, '%s: %d elements past the last partial row changed' % (what, bad)
        left = int((self.bits[:self.n] == SENTINEL).sum())
        assert left == 0, '%s: %d elements of the partial rows never written' % (what, left)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sums(part, rows, nv, C, pairs, n, extra, what):
    """partial rows [rows][nv][C] of fp32 sums, added in float64: within (n + extra) roundings of the sum of |terms|, whatever the
    split into rows was (n: the number of summed terms, extra: the roundings of forming one term)"""
    _totals(part[:rows * nv * C].double().reshape(rows, nv, C).sum(0), pairs, n, extra, what)


# --------------------------------------------------------------------------------------------------------------- the roles
def run_forward(L, c, inp, pname, layout, stats=True, up=None):
    """-> (y plane, statistic rows or None).  up = (tensor (N, h, w, up_C), its Plane): the UP form"""
    dev = inp['x'].device
    Ho, Wo, pt, pl = geom(c)
    sc, sh, act = pro_args(inp, pname)
    x = inp['x']
    if up is not None:
        upx, up_C = up
        x = x.clone()
        x[..., :up_C] = float('nan')                  # these channels of x are not read
        UPP = Plane(upx.shape[0] * upx.shape[1] * upx.shape[2], up_C, layout, dev, upx)
    X = Plane(c.N * c.H * c.W, c.C, layout, dev, x)
    Y = Plane(c.N * Ho * Wo, c.C, layout, dev)
    with options(L, c):
        nbx = plan(L, 0, c)[4]
        part = Flat(nbx * 2 * c.C, dev) if stats else None
        rows = ctypes.c_int(0)
        if up is not None:
            L.dw_upsampled_input(UPP.p, UPP.ld, upx.shape[1], upx.shape[2], up_C, _s())
        L.dwconv2d_fwd(X.p, X.ld, _ptr(sc), _ptr(sh), act, inp['w'].data_ptr(), Y.p, Y.ld, part.p if stats else None,
                       ctypes.byref(rows), c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo, _s())
    what = '%s forward %s %s%s' % (c.name, pname, layout, ' UP' if up is not None else '')
    assert rows.value == nbx, (what, rows.value, nbx)
    y = Y.t.reshape(c.N, Ho, Wo, c.C)
    if up is None:
        ref, bound = fwd_ref(inp['x'], inp['w'], sc, sh, act, c)
    else:
        ref, bound = up_fwd_ref(inp['x'], upx, up_C, inp['w'], sc, sh, act, c)
    _inside(y, ref, bound, what)
    Y.intact(what)
    if stats:
        part.intact(what + ' statistics')
        pairs, extra = stat_pairs(y)
        _sums(part.t, nbx, 2, c.C, pairs, c.N * Ho * Wo, extra, what + ' statistics')
    return Y, (part.t[:nbx * 2 * c.C] if stats else None)


def run_dgrad(L, c, inp, layout, accumulate=False):
    dev = inp['x'].device
    Ho, Wo, pt, pl = geom(c)
    D = Plane(c.N * Ho * Wo, c.C, layout, dev, inp['dy'])
    G = Plane(c.N * c.H * c.W, c.C, layout, dev, inp['base'] if accumulate else None, out=True)
    with options(L, c):
        L.dwconv2d_bwd_data(D.p, D.ld, inp['w'].data_ptr(), G.p, G.ld, int(accumulate), c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl,
                            Ho, Wo, _s())
    what = '%s data gradient %s%s' % (c.name, layout, ' accumulate' if accumulate else '')
    ref, bound = dgrad_ref(inp['dy'], inp['w'], c, base=inp['base'] if accumulate else None)
    _inside(G.t.reshape(c.N, c.H, c.W, c.C), ref, bound, what)
    G.intact(what)
    return G


def run_dgrad_bn(L, c, inp, layout, act, plain):
    """gx bitwise the plain data gradient's; the sums (sum g', sum g' * xhat) of the finished gradient within their bound"""
    dev = inp['x'].device
    Ho, Wo, pt, pl = geom(c)
    D = Plane(c.N * Ho * Wo, c.C, layout, dev, inp['dy'])
    G = Plane(c.N * c.H * c.W, c.C, layout, dev)
    Z = Plane(c.N * c.H * c.W, c.C, layout, dev, inp['z'])
    part = Flat(0, dev, total=2048 * 2 * c.C + 256)
    rows = ctypes.c_int(0)
    with options(L, c):
        L.dwconv2d_bwd_data_bn(D.p, D.ld, inp['w'].data_ptr(), G.p, G.ld, 0, c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo,
                               Z.p, Z.ld, inp['bsc'].data_ptr(), inp['bsh'].data_ptr(), act, inp['mu'].data_ptr(),
                               inp['inv'].data_ptr(), part.p, ctypes.byref(rows), _s())
    what = '%s data gradient + BN sums (act %d) %s' % (c.name, act, layout)
    assert 0 < rows.value <= 2048, (what, rows.value)
    part.n = rows.value * 2 * c.C
    part.intact(what)
    G.intact(what)
    assert torch.equal(G.t.contiguous().view(torch.int32), plain.t.contiguous().view(torch.int32)), what + ': gx differs from the plain data gradient'
    pairs, extra = bnsum_pairs(G.t.reshape(c.N, c.H, c.W, c.C), inp['z'], inp['bsc'], inp['bsh'], inp['mu'], inp['inv'], act)
    _sums(part.t, rows.value, 2, c.C, pairs, c.N * c.H * c.W, extra, what)


def run_wgrad(L, c, inp, pname, layout, slabs=False, up=None):
    dev = inp['x'].device
    Ho, Wo, pt, pl = geom(c)
    sc, sh, act = pro_args(inp, pname)
    x = inp['x']
    if up is not None:
        upx, up_C = up
        x = x.clone()
        x[..., :up_C] = float('nan')
        UPP = Plane(upx.shape[0] * upx.shape[1] * upx.shape[2], up_C, layout, dev, upx)
    X = Plane(c.N * c.H * c.W, c.C, layout, dev, x)
    D = Plane(c.N * Ho * Wo, c.C, layout, dev, inp['dy'])
    need = L.dwconv2d_bwd_weight_workspace(c.N, Ho, Wo, c.C, c.k)
    ws = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=dev)      # every float read must have been written
    GW = Flat(c.k * c.k * c.C, dev)
    rows = ctypes.c_int(0)
    what = '%s weight gradient %s %s%s%s' % (c.name, pname, layout, ' slabs' if slabs else '', ' UP' if up is not None else '')
    with options(L, c):
        if up is not None:
            L.dw_upsampled_input(UPP.p, UPP.ld, upx.shape[1], upx.shape[2], up_C, _s())
        if slabs:
            L.dwconv2d_bwd_weight_slabs(X.p, X.ld, _ptr(sc), _ptr(sh), act, D.p, D.ld, ws.data_ptr(), need, ctypes.byref(rows),
                                        c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo, _s())
            nbx = plan(L, 3, c)[4]
            assert rows.value == nbx, (what, rows.value, nbx)
        else:
            L.dwconv2d_bwd_weight(X.p, X.ld, _ptr(sc), _ptr(sh), act, D.p, D.ld, GW.p, ws.data_ptr(), need, c.N, c.H, c.W, c.C,
                                  c.k, c.s, c.r, pt, pl, Ho, Wo, _s())
    if up is None:
        ref, bound = wgrad_ref(inp['x'], inp['dy'], sc, sh, act, c)
    else:
        ref, bound = up_wgrad_ref(inp['x'], upx, up_C, inp['dy'], sc, sh, act, c)
    if slabs:
        n = c.k * c.k * c.C
        assert bool(torch.isnan(ws[rows.value * n:]).all()), what + ': workspace written past the last slab'
        got = ws[:rows.value * n].double().reshape(rows.value, c.k, c.k, c.C).sum(0)
        _inside(got, ref, bound, what)
        return got
    GW.intact(what)
    _inside(GW.t[:GW.n].reshape(c.k, c.k, c.C), ref, bound, what)
    return GW.t[:GW.n]


def fold_ref(inp, fa_sc, fa_sh, fa_act, c):
    """dz = c0 * (g * act'(u) - c1 - xhat * c2) as the kernel forms it: bA = c0, bC = (c0 * invstd) * c2 (2 roundings), bD =
    bC * mean - c0 * c1 (1 + 1 + 1), dz = fma(bA, g * act', fma(-bC, z, bD)).  Roundings a term passes: bC * z: 2 + the two fmas = 4;
    bC * mean: 2 + 1 + 1 + 2 = 6; c0 * c1: 1 + 1 + 2 = 4; c0 * g * act': the product, the outer fma and those of act' -> every term
    within 6 + n_g roundings, + 1 for second order: (7 + n_g) * u * T with T the sum of the terms' magnitudes"""
    g, z = inp['dy'].double(), inp['zo']
    c0, c1, c2 = (inp['coef'][i].double() for i in range(3))
    mu, inv = inp['mu'].double(), inp['inv'].double()
    u32 = z if fa_sc is None else fma32(z, fa_sc.expand_as(z), fa_sh.expand_as(z))
    d, m, n_g = grad_terms(u32, fa_act)
    zd = z.double()
    dz = c0 * (g * d - c1 - (zd - mu) * inv * c2)
    T = c0.abs() * (g.abs() * m + c1.abs() + (zd.abs() + mu.abs()) * inv * c2.abs())
    return dz, (7 + n_g) * U * T


def run_wgrad_bn(L, c, inp, pname, layout, fa_act, fa_affine=True, want_dz=True, up=None):
    """the folded weight gradient: dz into a slice (or not at all), gw from the kernel's own dz"""
    dev = inp['x'].device
    Ho, Wo, pt, pl = geom(c)
    sc, sh, act = pro_args(inp, pname)
    fa_sc, fa_sh = (inp['bsc'], inp['bsh']) if fa_affine else (None, None)
    x = inp['x']
    if up is not None:
        upx, up_C = up
        x = x.clone()
        x[..., :up_C] = float('nan')
        UPP = Plane(upx.shape[0] * upx.shape[1] * upx.shape[2], up_C, layout, dev, upx)
    X = Plane(c.N * c.H * c.W, c.C, layout, dev, x)
    Gp = Plane(c.N * Ho * Wo, c.C, layout, dev, inp['dy'])
    Z = Plane(c.N * Ho * Wo, c.C, layout, dev, inp['zo'])
    DZ = Plane(c.N * Ho * Wo, c.C, layout, dev)
    need = L.dwconv2d_bwd_weight_workspace(c.N, Ho, Wo, c.C, c.k)
    ws = torch.full((need // 4,), float('nan'), dtype=torch.float32, device=dev)
    rows = ctypes.c_int(0)
    what = '%s folded weight gradient %s %s fa_act %d%s%s' % (c.name, pname, layout, fa_act, '' if want_dz else ' no dz', ' UP' if up is not None else '')
    with options(L, c):
        if up is not None:
            L.dw_upsampled_input(UPP.p, UPP.ld, upx.shape[1], upx.shape[2], up_C, _s())
        L.dwconv2d_bwd_weight_slabs_bn(X.p, X.ld, _ptr(sc), _ptr(sh), act, Gp.p, Gp.ld, Z.p, Z.ld, _ptr(fa_sc), _ptr(fa_sh), fa_act,
                                       inp['mu'].data_ptr(), inp['inv'].data_ptr(), inp['coef'].data_ptr(),
                                       DZ.p if want_dz else None, DZ.ld if want_dz else 0, ws.data_ptr(), need, ctypes.byref(rows),
                                       c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo, _s())
        nbx = plan(L, 3, c)[4]
    assert rows.value == nbx, (what, rows.value, nbx)
    dz, dzb = fold_ref(inp, fa_sc, fa_sh, fa_act, c)
    DZ.intact(what)
    if want_dz:
        _inside(DZ.t.reshape(c.N, Ho, Wo, c.C), dz, dzb, what + ' dz')
    else:
        assert bool((DZ.bits == SENTINEL).all()), what + ': dz written although none was asked for'
    n = c.k * c.k * c.C
    assert bool(torch.isnan(ws[rows.value * n:]).all()), what + ': workspace written past the last slab'
    got = ws[:rows.value * n].double().reshape(rows.value, c.k, c.k, c.C).sum(0)
    if up is None:
        ref, bound = wgrad_ref(inp['x'], dz, sc, sh, act, c, ddy=dzb)
    else:
        ref, bound = up_wgrad_ref(inp['x'], upx, up_C, dz, sc, sh, act, c, ddy=dzb)
    _inside(got, ref, bound, what + ' gw')
    return ws[:rows.value * n], (DZ if want_dz else None)


# ---- the UP form: channels [0, up_C) of the input are the bilinear upsampling of up_x, formed on the fly
def _lerp_index(out, inn):
    """dw_lerp in fp32, operation for operation (numpy float32): lo, hi, t for every output coordinate"""
    scale = np.float32(inn) / np.float32(out)
    src = (np.arange(out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    fl = np.floor(src)
    lo = np.maximum(fl.astype(np.int64), 0)
    hi = np.minimum(np.ceil(src).astype(np.int64), inn - 1)
    return lo, hi, (src - fl).astype(np.float32)


def upsample_terms(upx, H, W, f32=False):
    """float64 value of the upsampled input from the fp32 coefficients the kernel uses, and M4 = |tl| + |tr| + |bl| + |br|.
    top = tl + (tr - tl) * tx, bottom likewise, out = top + (bottom - top) * ty: three roundings each (no contraction), the first two
    of |tl| + |tr| resp. |bl| + |br|, the last of |top| + |bottom| and passing the first two on -> within 6 * u * M4"""
    dev = upx.device
    ly, hy, ty = _lerp_index(H, upx.shape[1])
    lx, hx, tx = _lerp_index(W, upx.shape[2])
    ty = torch.from_numpy(ty).to(dev).reshape(1, H, 1, 1)
    tx = torch.from_numpy(tx).to(dev).reshape(1, 1, W, 1)
    u = upx          # f32: the kernel's own operations in fp32 (no contraction: every -, * and + rounds)
    if not f32:
        ty, tx, u = ty.double(), tx.double(), upx.double()
    ly, hy, lx, hx = (torch.from_numpy(v).to(dev) for v in (ly, hy, lx, hx))
    tl, tr, bl, br = u[:, ly][:, :, lx], u[:, ly][:, :, hx], u[:, hy][:, :, lx], u[:, hy][:, :, hx]
    top, bot = tl + (tr - tl) * tx, bl + (br - bl) * tx
    return top + (bot - top) * ty, tl.abs() + tr.abs() + bl.abs() + br.abs()


def _up_input(x, upx, up_C, sc, sh, act):
    """a and p of the composed input: on the upsampled channels the lerps' 6 * u * M4 enters the affine through |scale|, so p there is
    (1 + 6) * |scale| * M4 + |shift| (|value| <= M4)"""
    val, m4 = upsample_terms(upx, x.shape[1], x.shape[2])
    xin = x.double().clone()
    xin[..., :up_C] = val
    a = act64(xin * sc.double() + sh.double(), act)
    p = (xin * sc.double()).abs() + sh.double().abs()
    p[..., :up_C] = 7 * sc.double()[:up_C].abs() * m4 + sh.double()[:up_C].abs()
    return a, p


def up_fwd_ref(x, upx, up_C, w, sc, sh, act, c):
    return fwd_ref(x, w, sc, sh, act, c, ap=_up_input(x, upx, up_C, sc, sh, act))


def up_wgrad_ref(x, upx, up_C, dy, sc, sh, act, c, ddy=None):
    return wgrad_ref(x, dy, sc, sh, act, c, ddy=ddy, ap=_up_input(x, upx, up_C, sc, sh, act))


# ------------------------------------------------------------------------------------------------------------ GPU: the case table
WGRAD_PROS = ('none', 'affine', 'hswish')
DEV = 'cuda'


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_forward(ops, c):
    """every prologue on views; without a statistics buffer y is bitwise the same; contiguous operands give the same bits too"""
    L, inp = ops.lib(), inputs(c, DEV)
    for pname in PROS:
        Y, part = run_forward(L, c, inp, pname, 'view')
        if pname in ('affine', 'relu6'):
            Y2, _ = run_forward(L, c, inp, pname, 'view', stats=False)
            assert torch.equal(_bits(Y.t), _bits(Y2.t)), '%s %s: y differs without a statistics buffer' % (c.name, pname)
            Y3, part3 = run_forward(L, c, inp, pname, 'contig')
            assert torch.equal(_bits(Y.t), _bits(Y3.t)) and torch.equal(_bits(part), _bits(part3)), '%s %s: contiguous differs' % (c.name, pname)


@gpu
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_data_gradient(ops, c):
    L, inp = ops.lib(), inputs(c, DEV)
    G = run_dgrad(L, c, inp, 'view')
    G.written('%s data gradient' % c.name)
    Gc = run_dgrad(L, c, inp, 'contig')
    assert torch.equal(_bits(G.t), _bits(Gc.t))
    run_dgrad(L, c, inp, 'view', accumulate=True)
    for act in (RELU6, HSWISH, NONE):
        run_dgrad_bn(L, c, inp, 'view', act, G)


@gpu
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_weight_gradient(ops, c):
    L, inp = ops.lib(), inputs(c, DEV)
    for pname in WGRAD_PROS:
        gw = run_wgrad(L, c, inp, pname, 'view')
        run_wgrad(L, c, inp, pname, 'view', slabs=True)
        if pname == 'hswish':
            assert torch.equal(_bits(gw), _bits(run_wgrad(L, c, inp, pname, 'contig')))


FOLD_CASES = [c for c in CASES if c.k == 3]


@gpu
@pytest.mark.parametrize('c', FOLD_CASES, ids=lambda c: c.name)
def test_folded_weight_gradient(ops, c):
    """dl3p_dwconv2d_bwd_weight_slabs_bn where the window kernels serve the geometry, a loud refusal where they do not"""
    L, inp = ops.lib(), inputs(c, DEV)
    if not WANT[c.name][5]:
        with pytest.raises(ops.Dl3pError):
            run_wgrad_bn(L, c, inp, 'relu6', 'view', RELU6)
        return
    for pname, fa_act, fa_affine in (('none', RELU6, True), ('affine', NONE, True), ('relu6', HSWISH, True), ('hswish', RELU, False)):
        slabs, DZ = run_wgrad_bn(L, c, inp, pname, 'view', fa_act, fa_affine)
        DZ.written('%s folded dz' % c.name)
        if pname == 'relu6':
            slabs2, _ = run_wgrad_bn(L, c, inp, pname, 'view', fa_act, fa_affine, want_dz=False)
            assert torch.equal(_bits(slabs), _bits(slabs2)), '%s: gw slabs differ without dz' % c.name


UP_CASES = [c for c in CASES if c.k == 3 and c.s == 1 and c.r == 1 and c.C <= 1280]


@gpu
@pytest.mark.parametrize('c', UP_CASES, ids=lambda c: c.name)
def test_upsampled_input(ops, c):
    """the UP form of the forward and of both weight gradients with up_C < C (where C allows) and up_C == C; a loud refusal where the
    launch would not be a stride-1 window kernel"""
    L, inp = ops.lib(), inputs(c, DEV)
    g = torch.Generator()
    g.manual_seed(zlib.crc32(c.name.encode()) + 1)
    h, w = max(1, (c.H + 2) // 4), max(1, (c.W + 1) // 3)
    for up_C in sorted({max(4, c.C // 2 // 4 * 4), c.C}):
        upx = (torch.randn(c.N, h, w, up_C, generator=g) * 2).to(DEV)
        if not WANT[c.name][3]:
            with pytest.raises(ops.Dl3pError):
                run_forward(L, c, inp, 'relu6', 'view', up=(upx, up_C))
            continue          # (the armed description was consumed by the refused call: dw_take_up is the entry's first action)
        for pname in ('relu6', 'hswish'):
            run_forward(L, c, inp, pname, 'view', up=(upx, up_C))
        run_wgrad(L, c, inp, 'relu6', 'view', up=(upx, up_C))
        run_wgrad(L, c, inp, 'hswish', 'view', slabs=True, up=(upx, up_C))
        _, DZ = run_wgrad_bn(L, c, inp, 'relu6', 'view', RELU6, up=(upx, up_C))
        DZ.written('%s folded UP dz' % c.name)


@gpu
def test_bad_arguments_fail_loudly(ops):
    """out-of-contract arguments are refused by the host guards, nothing is launched"""
    L, c = ops.lib(), BY_NAME['s1_w17']
    inp = inputs(c, DEV)
    Ho, Wo, pt, pl = geom(c)
    x, y = inp['x'], torch.empty((c.N, Ho, Wo, c.C), device=DEV)
    a = (c.N, c.H, c.W, c.C, c.k, c.s, c.r, pt, pl, Ho, Wo, _s())
    with pytest.raises(ops.Dl3pError):          # ld below C
        L.dwconv2d_fwd(x.data_ptr(), c.C - 4, None, None, NONE, inp['w'].data_ptr(), y.data_ptr(), c.C, None, None, *a)
    with pytest.raises(ops.Dl3pError):          # ld not a multiple of 4
        L.dwconv2d_fwd(x.data_ptr(), c.C, None, None, NONE, inp['w'].data_ptr(), y.data_ptr(), c.C + 2, None, None, *a)
    with pytest.raises(ops.Dl3pError):          # a base that is not 16-byte aligned
        L.dwconv2d_fwd(x.data_ptr() + 4, c.C, None, None, NONE, inp['w'].data_ptr(), y.data_ptr(), c.C, None, None, *a)
    with pytest.raises(ops.Dl3pError):          # kernel size 4
        L.dwconv2d_fwd(x.data_ptr(), c.C, None, None, NONE, inp['w'].data_ptr(), y.data_ptr(), c.C, None, None,
                       c.N, c.H, c.W, c.C, 4, c.s, c.r, pt, pl, Ho, Wo, _s())
    with pytest.raises(ops.Dl3pError):          # a workspace too small for the weight gradient
        L.dwconv2d_bwd_weight(x.data_ptr(), c.C, None, None, NONE, y.data_ptr(), c.C, y.data_ptr(), y.data_ptr(), 64, *a)
    with pytest.raises(ops.Dl3pError):          # dz aliasing g in the folded weight gradient
        L.dwconv2d_bwd_weight_slabs_bn(x.data_ptr(), c.C, None, None, NONE, y.data_ptr(), c.C, y.data_ptr(), c.C, None, None, NONE,
                                       inp['mu'].data_ptr(), inp['inv'].data_ptr(), inp['coef'].data_ptr(), y.data_ptr(), c.C,
                                       y.data_ptr(), 1 << 40, ctypes.byref(ctypes.c_int(0)), *a)


# ------------------------------------------------------------------------------------- environment-selected kernels, in children
# the cases every child runs: 3x3 strips of 4 and of 2 with interior and edge strips, bands of one row (the small maps: one band per
# row), a rate whose last band holds no row of the odd sub-lattice (r2: 13 rows -> 7 + 6), forced bands, stride 2, the 5x5 kernels
# at stride 1 (both strip widths, rate 2, bands, the one-lane slab plan) and stride 2, both residue-class kernels, the gather
CHILD_CASES = ('s1_w17', 's1_w19', 's1_tw2_w17', 'r2_ragged', 'r2_tw2_ragged', 'r6_ragged', 'band_1', 'band_4', 'band_uh',
               'band_4_tw2_r2', 'band_default', 's2_same_odd', 's2_p1111', 's2_band_3', 'k5_uw40', 'k5_uw41', 'k5_r2', 'k5_s2', 'k5_c268', 'k5_bands',
               'lat2_2r_eq_h', 'lat3_3r_eq_h', 'lat3_h_ne_w', 'r36_on_33', 'c2052_n1')
CHILD_PROS = ('affine', 'relu6')        # PRO == 1 and PRO == 2
PROD = (16, 129, 129, 304)              # the one production launch that takes FAST_K by the 200 MiB rule
CHILD_ENVS = collections.OrderedDict([
    ('fast2', {'DL3P_DW_FAST_ROWS': '2', 'DL3P_DW5_ROWS': '0'}),
    ('fast0', {'DL3P_DW_FAST_ROWS': '0', 'DL3P_DW5_ROWS': '0'}),
    ('default', {}),
    ('fast0_nt0', {'DL3P_DW_FAST_ROWS': '0', 'DL3P_DW_NT': '0'}),
    ('rows2', {'DL3P_DW5_ROWS': '2', 'DL3P_DW5_WROWS': '1', 'DL3P_DW_LAT3': '0', 'DL3P_DW_BALANCE': '1'}),
    ('rows4', {'DL3P_DW5_ROWS': '4', 'DL3P_DW5_WROWS': '0', 'DL3P_DW_BALANCE': '0'}),
])
SWITCHES = ('DL3P_DW_FAST_ROWS', 'DL3P_DW5_ROWS', 'DL3P_DW5_WROWS', 'DL3P_DW_LAT3', 'DL3P_DW_BALANCE', 'DL3P_DW_NT', 'DL3P_DW_WANT',
            'DL3P_DW_MAXTH', 'DL3P_DW_BAND', 'DL3P_DW_TUNED', 'DL3P_DWF_PER_CU', 'DL3P_DWW_PER_CU')


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def child_main(prod):
    """runs in a fresh interpreter under the parent's switches: every child case through the forward (PRO 1 and 2; contiguous, on
    views, without statistics), the data gradient and the weight gradient, each held to the float64 bound here; digests go back"""
    ops = load_pkg('ops')
    L = ops.lib()
    out, fails, plans = {}, [], {}
    for name in CHILD_CASES:
        c = BY_NAME[name]
        inp = inputs(c, DEV)
        with options(L, c):
            plans[name] = [plan(L, role, c)[:4] for role in (0, 1, 3)]
        try:
            for pname in CHILD_PROS:
                for layout, stats in (('contig', True), ('view', True), ('contig', False)):
                    Y, part = run_forward(L, c, inp, pname, layout, stats=stats)
                    out['%s fwd %s %s %d' % (name, pname, layout, stats)] = [_digest(Y.t), _digest(part) if stats else '']
            out['%s dgrad' % name] = [_digest(run_dgrad(L, c, inp, 'view').t), '']
            out['%s wgrad' % name] = ['', _digest(run_wgrad(L, c, inp, 'relu6', 'view'))]
            run_wgrad(L, c, inp, 'affine', 'contig')
            run_wgrad(L, c, inp, 'none', 'contig')
        except AssertionError as e:
            fails.append(str(e)[:400])
    if prod:
        N, H, W, C = PROD
        g = torch.Generator(device=DEV)
        g.manual_seed(11)
        x = torch.randn(N, H, W, C, device=DEV, generator=g)
        w = torch.randn(3, 3, C, device=DEV, generator=g) / 3
        sc, sh = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g) * 0.3
        part = ops.new_partials(C, DEV)
        y, rows = ops.dwconv2d_fwd(x, w, 1, 1, 'same', sc, sh, RELU6, partials=part)
        out['prod'] = [_digest(y), _digest(part[:rows * 2 * C])]
    torch.cuda.synchronize()
    print('RESULT ' + json.dumps({'digests': out, 'fails': fails, 'plans': plans}))


_children = {}
_child_dead = []


def _child(key):
    """the child of CHILD_ENVS[key], run once per session; after a child that ended abnormally or ran out of time no other is started"""
    if key in _children:
        return _children[key]
    if _child_dead:
        pytest.skip('an earlier child ended abnormally (%s): no further child is started' % _child_dead[0])
    torch.cuda.empty_cache()          # (the children run on the same GPU)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(CHILD_ENVS[key])
    prod = key in ('default', 'fast0_nt0')
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(int(prod))], env=env, capture_output=True,
                           text=True, timeout=420)
    except subprocess.TimeoutExpired:
        _child_dead.append(key + ': timeout')
        raise AssertionError('child %s ran out of time' % key)
    if r.returncode != 0:
        _child_dead.append('%s: exit %d' % (key, r.returncode))
        raise AssertionError('child %s exit %d: %s' % (key, r.returncode, r.stderr[-2000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1]
    _children[key] = json.loads(line[len('RESULT '):])
    return _children[key]


def _same(a, b, which, keys=None):
    da, db = _child(a)['digests'], _child(b)['digests']
    keys = [k for k in da if k in db] if keys is None else keys
    assert len(keys) > 0
    return [k for k in keys if any(da[k][i] != db[k][i] for i in which)]


@gpu
def test_counted_wait_rows_change_no_bit(ops):
    """DL3P_DW_FAST_ROWS=2 (every launch that can takes a FAST_K kernel: 3x3 strips of 4 and 2, 3x3 stride 2, 5x5 stride 2 and, with
    DL3P_DW5_ROWS=0, the 5x5 stride-1 window kernel; PRO 1 and 2; contiguous, views, no statistics) against DL3P_DW_FAST_ROWS=0: y and
    the statistic rows bit for bit, and each side inside the float64 bound"""
    new, old = _child('fast2'), _child('fast0')
    assert not new['fails'] and not old['fails'], (new['fails'], old['fails'])
    assert new['digests'].keys() == old['digests'].keys() and len(new['digests']) == len(CHILD_CASES) * 8
    diff = _same('fast2', 'fast0', (0, 1))
    assert not diff, diff


@gpu
def test_streaming_stores_and_the_production_fast_launch_change_no_bit(ops):
    """default switches (streaming stores; (16, 129, 129, 304) takes FAST_K by the 200 MiB rule) against DL3P_DW_FAST_ROWS=0 with
    DL3P_DW_NT=0: every digest equal, the production launch included"""
    new, old = _child('default'), _child('fast0_nt0')
    assert not new['fails'] and not old['fails'], (new['fails'], old['fails'])
    assert 'prod' in new['digests'] and new['digests'].keys() == old['digests'].keys()
    diff = _same('default', 'fast0_nt0', (0, 1))
    assert not diff, diff


@gpu
@pytest.mark.parametrize('key', ['fast0', 'rows2', 'rows4'])
def test_switch_selected_kernels(ops, key):
    """DL3P_DW5_ROWS = 0 | 2 | 4, DL3P_DW5_WROWS = 1 | 0, DL3P_DW_LAT3 = 0, DL3P_DW_BALANCE = 1 | 0: inside the float64 bound (checked in
    the child); y and the data gradient bitwise the default's (one fma chain per element in every decomposition, see the module
    docstring); the statistic rows and the weight gradient follow the work split and are held to the bound only"""
    res, ref = _child(key), _child('default')
    assert not res['fails'] and not ref['fails'], (res['fails'], ref['fails'])
    diff = _same(key, 'default', (0,))
    assert not diff, diff
    if key == 'rows2':      # DL3P_DW_LAT3=0 sends the 3 x 3 classes to the gather; DL3P_DW_BALANCE=1 takes pick_band's power-of-two bands
        assert res['plans']['lat3_3r_eq_h'][0][0] == 0 and ref['plans']['lat3_3r_eq_h'][0][0] == 3
        assert res['plans']['band_default'][0][2:] == [4, 11] and ref['plans']['band_default'][0][2:] == [6, 8], (res['plans'], ref['plans'])
    if key == 'rows4':      # DL3P_DW_BALANCE=0: the same bands of 4, the last one reaching past row 41
        assert res['plans']['band_default'][0][2:] == [4, 11], res['plans']


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        child_main(bool(int(sys.argv[2])))
