"""The fused inverted-residual kernels (csrc/irb_fwd.hip, irb_bwd.hip) in float64, with per-element error bounds (numpy, CPU).

Reference: xk = act_in(x * xs + xh);  z = xk W1;  u = z * scale + shift;  a = act(u);  y = depthwise3x3(a) (forward);
da1 = depthwise^T(dy), g' = da1 * act'(u), the depthwise kernel's gradient sum a * dy and the BatchNorm rows (sum g', sum g' xhat)
with xhat = (z - mean) * invstd (pass A);  dz = c0 (g' - c1 - xhat c2), gw1 = xk^T dz, gx = dz W1^T (+ base) and the rows
(sum gx act0'(u0), sum gx act0'(u0) xhat0) of a BatchNorm in front of the block (pass B).  scale / shift / mean / invstd and the
coefficient triple are INPUTS of the kernels: the reference is evaluated at exactly the float32 values the device is given.

Bounds: U * (roundings * sum of |terms|), U = 2^-24, the roundings counted from the kernels' own operations (each count carries
one more for second-order terms and the float64 reference).  No tensor-scale term, no constant fitted to an output.

 * u, forward, fast pair (the prologue is folded): the weight fl(fl(w xs) scale) is rounded twice, its product once, the MFMA
   chain adds K times -> (K + 3 + 1) * Tz, Tz = |scale| sum_k |w xs x|.  The chain starts from the folded shift
   fma(scale, chain_k fma(w, xh), shift): K + 1 roundings, then the K adds -> (2K + 1 + 1) * Tb, Tb = |shift| + |scale| sum_k |w xh|.
 * u, forward, generic pair: xk costs N_PRO roundings of p = |x xs| + |xh| (the activation's Lipschitz constant) and N_ACT of
   |xk|; z = chain from 0: (K + 1) * Z, Z = sum_k |w xk|; u = fma(z, scale, shift): one of |scale| Z + |shift|
   -> (K + 3) |scale| Z + 2 |shift| + |scale| sum_k |w| dxk.
 * zc = z - mean, backward, fast pair: weight fl(w xs) once, product, K adds -> (K + 3) * Tz; start value chain_k fma(w, xh) - mean:
   K + 1, then K adds -> (2K + 2) * (sum_k |w xh| + |mean|).  Generic pair: chain from -mean (pass A) or chain from 0 and one
   subtraction (pass B) -> (K + 3) * Z + (K + 2) |mean| + sum_k |w| dxk.
   u = fma(zc, scale, fma(scale, mean, shift)): |scale| dzc + 2 |zc scale| + 3 (|scale mean| + |shift|).
 * a = act(u): L * du + N_ACT * |a| (L = 1; 1.5 for hard-swish).  y: nine fmas -> (9 + 1) * conv(|a|, |w|) + conv(da, |w|).
 * da1: at most nine fmas -> 10 * Sda, Sda = depthwise^T(|dy|, |w|); g' = da1 act'(u): n_g + 2 more of Sda m (m = |act'|), and
   Sda * Lg * du where act' is Lipschitz inside a piece (hard-swish: 1/3).
 * dz = g + fma(A, zc, B), g from the depthwise kernel pre-scaled by c0 (1 rounding), its chain (9), the product with act' (1 + n_g),
   the add (1) -> (13 + n_g) * T1; A = fl(fl(-c0 c2) invstd) (2), the fma, the add -> 5 * T2 and |A| dzc; B = fl(-c0 c1) -> 4 * T3.
 * sums of n terms: n + 1 roundings of the sum of |terms| whatever the order (+ the roundings of forming a term), plus the terms'
   own bounds, summed.

Kinks (0 for ReLU, 0 and 6 for ReLU6, -3 and 3 for hard-swish): an element whose float64 u lies within its own bound du of a kink is
AMBIGUOUS: the device may take either branch of act', which moves g' by at most |da1| (slack).  Outputs carry bound and slack
separately; slack is zero on every pixel without an ambiguous element.  The forward needs none (act is continuous)."""
import collections
import zlib

import numpy as np

U = 2.0 ** -24
NONE, RELU, RELU6, HSWISH = 0, 1, 2, 3
SIXTH = np.float32(1.0) / np.float32(6.0)
N_PRO = {NONE: 1.0, RELU: 1.0, RELU6: 1.0, HSWISH: 1.5}      # Lipschitz constant of the activation
N_ACT = {NONE: 0, RELU: 0, RELU6: 0, HSWISH: 4}              # roundings of forming it (v + 3, fl(1/6), * fl(1/6), v * t)
N_GRAD = {NONE: 0, RELU: 0, RELU6: 0, HSWISH: 6}             # roundings of act' (t, hs = clamp * fl(1/6): 2, u * fl(1/6): 2, the sum)
L_GRAD = {NONE: 0.0, RELU: 0.0, RELU6: 0.0, HSWISH: 1.0 / 3}  # Lipschitz constant of act' inside a piece
KINKS = {NONE: (), RELU: (0.0,), RELU6: (0.0, 6.0), HSWISH: (-3.0, 3.0)}
AMBIGUOUS_CAP = 0.02
EPS = 1e-3
FAST = (NONE, RELU6)

# ---------------------------------------------------------------------------------------------------------------- the case tables
# pad: 'same' or (top, bottom, left, right).  ct / waves: dl3p_irb_set_plan.  pair: (in_act, bn_act); affine: which of in_scale /
# in_shift are given ('both', 'scale', 'none').  layout: 'contig', 'view' (ldx = K + 8 at channel 4, ldy = C + 12 at 8), 'view2'
# (K = 24: ldx = K + 2 at 2, the float2 path).  plan = what dl3p_irb_plan_query must report: (CT, nseg, nband, band, rows).
F = collections.namedtuple('F', 'name N H W K C s pad ct waves pair affine layout plan')
BIG = 1 << 20


def _f(name, N, H, W, K, C, s, plan, pad='same', ct=0, waves=0, pair=FAST, affine='both', layout='contig'):
    return F(name, N, H, W, K, C, s, pad, ct, waves, pair, affine, layout, plan)


GEN = {'relu': (NONE, RELU), 'hswish': (NONE, HSWISH), 'none': (NONE, NONE), 'r6r6': (RELU6, RELU6), 'hsr6': (HSWISH, RELU6)}
FWD = [
    # ---- stride 2 columns: Wo in {1, 14, 15, 16, 30, 31}, W odd (pad_l 1) and even (pad_l 0); 15 outputs per segment
    _f('s2_w1', 2, 5, 1, 16, 48, 2, (1, 1, 1, 3, 2)), _f('s2_w2', 2, 5, 2, 16, 48, 2, (3, 1, 1, 3, 2), ct=3),
    _f('s2_w27', 2, 5, 27, 16, 48, 2, (1, 1, 1, 3, 2), pair=GEN['relu']), _f('s2_w28', 2, 5, 28, 16, 48, 2, (3, 1, 1, 3, 2), ct=3, pair=GEN['hswish']),
    _f('s2_w29', 2, 5, 29, 24, 96, 2, (2, 1, 1, 3, 2)), _f('s2_w30', 2, 5, 30, 24, 96, 2, (2, 1, 1, 3, 2), pair=GEN['none']),
    _f('s2_w31', 2, 5, 31, 32, 192, 2, (2, 2, 1, 3, 4)), _f('s2_w32', 2, 5, 32, 32, 192, 2, (3, 2, 1, 3, 4), ct=3, pair=GEN['r6r6']),
    _f('s2_w59', 1, 5, 59, 24, 144, 2, (1, 2, 1, 3, 2)), _f('s2_w60', 1, 5, 60, 24, 144, 2, (3, 2, 1, 3, 2), ct=3, pair=GEN['hsr6']),
    _f('s2_w61', 1, 5, 61, 32, 192, 2, (1, 3, 1, 3, 3), ct=1), _f('s2_w62', 1, 5, 62, 16, 96, 2, (2, 3, 1, 3, 3)),
    # ---- stride 1 columns: Wo in {1, 2, 13, 14, 15, 28, 29}; 14 outputs per segment
    _f('s1_w1', 2, 5, 1, 16, 48, 1, (1, 1, 2, 4, 4)), _f('s1_w2', 2, 5, 2, 16, 48, 1, (3, 1, 2, 4, 4), ct=3, pair=GEN['relu']),
    _f('s1_w13', 2, 5, 13, 24, 96, 1, (2, 1, 2, 4, 4)), _f('s1_w14', 2, 5, 14, 24, 144, 1, (3, 1, 2, 4, 4), ct=3),
    _f('s1_w15', 2, 5, 15, 32, 192, 1, (2, 2, 2, 4, 8), pair=GEN['hswish']), _f('s1_w28', 1, 5, 28, 32, 192, 1, (3, 2, 2, 4, 4), ct=3),
    _f('s1_w29', 1, 5, 29, 16, 96, 1, (2, 3, 2, 4, 6), pair=GEN['none']),
    # ---- explicit padding
    _f('s1_p0000', 2, 8, 17, 16, 48, 1, (1, 2, 2, 4, 8), pad=(0, 0, 0, 0)), _f('s2_p1111', 2, 10, 16, 16, 48, 2, (1, 1, 2, 4, 4), pad=(1, 1, 1, 1)),
    _f('s2_p0101', 2, 9, 17, 24, 96, 2, (2, 1, 1, 4, 2), pad=(0, 1, 0, 1), pair=GEN['relu']),
    # ---- rows: Ho in {1, 2, 3} (below the minimum band of 4), H = 1 with W = 1
    _f('s1_h1_w1', 1, 1, 1, 16, 16, 1, (1, 1, 1, 1, 1)), _f('s2_h1_w1', 1, 1, 1, 16, 16, 2, (1, 1, 1, 1, 1)),
    _f('s1_h2', 2, 2, 9, 16, 48, 1, (1, 1, 1, 2, 2)), _f('s1_h3', 2, 3, 9, 24, 144, 1, (1, 1, 1, 3, 2), pair=GEN['r6r6']),
    _f('s2_h2', 2, 2, 9, 32, 192, 2, (2, 1, 1, 1, 2), pair=GEN['none']), _f('s2_h3', 2, 3, 9, 16, 48, 2, (1, 1, 1, 2, 2)),
    _f('s2_h6', 2, 6, 9, 24, 144, 2, (1, 1, 1, 3, 2), ct=2, pair=GEN['relu']),
    # ---- bands of 4 (want_waves = BIG): Ho in {4, 5, 6, 7, 9} -> last bands of 4, 1, 2, 3, 1 rows; stride 1: every residue of the
    # 3-fold unroll; stride 2: odd and even band lengths on even H (the bottom padding row is reached) and odd H
    _f('s1_b4', 2, 4, 9, 16, 48, 1, (1, 1, 1, 4, 2), waves=BIG), _f('s1_b5', 2, 5, 9, 24, 144, 1, (1, 1, 2, 4, 4), waves=BIG, pair=GEN['hswish']),
    _f('s1_b6', 2, 6, 9, 16, 96, 1, (2, 1, 2, 4, 4), waves=BIG), _f('s1_b7', 2, 7, 9, 32, 192, 1, (1, 1, 2, 4, 4), waves=BIG, ct=1, pair=GEN['hsr6']),
    _f('s1_b9', 2, 9, 9, 16, 48, 1, (3, 1, 3, 4, 6), waves=BIG, ct=3),
    _f('s2_b4_h7', 2, 7, 9, 16, 48, 2, (1, 1, 1, 4, 2), waves=BIG), _f('s2_b4_h8', 2, 8, 9, 16, 48, 2, (1, 1, 1, 4, 2), waves=BIG, pair=GEN['hswish']),
    _f('s2_b5_h9', 2, 9, 9, 24, 144, 2, (1, 1, 2, 4, 4), waves=BIG), _f('s2_b5_h10', 2, 10, 9, 24, 144, 2, (3, 1, 2, 4, 4), waves=BIG, ct=3, pair=GEN['none']),
    _f('s2_b6_h11', 2, 11, 9, 32, 192, 2, (1, 1, 2, 4, 4), waves=BIG, ct=1, pair=GEN['relu']), _f('s2_b6_h12', 2, 12, 9, 32, 192, 2, (2, 1, 2, 4, 4), waves=BIG),
    _f('s2_b7_h13', 2, 13, 9, 16, 96, 2, (2, 1, 2, 4, 4), waves=BIG), _f('s2_b7_h14', 2, 14, 9, 16, 96, 2, (3, 1, 2, 4, 4), waves=BIG, ct=3),
    _f('s2_b9_h17', 1, 17, 9, 24, 96, 2, (2, 1, 3, 4, 3), waves=BIG, pair=GEN['r6r6']), _f('s2_b9_h18', 1, 18, 9, 24, 96, 2, (1, 1, 3, 4, 3), waves=BIG, ct=1),
    # ---- one long band (want_waves = 1): the unrolled row loops run several rounds
    _f('s1_one_band', 2, 11, 9, 16, 48, 1, (1, 1, 1, 11, 2), waves=1), _f('s2_one_band', 2, 13, 9, 24, 144, 2, (1, 1, 1, 7, 2), waves=1, pair=GEN['relu']),
    # ---- the statistic-row clamp decides the band count: 2048 / (16 * 3) = 42 bands of ceil(170 / 42) = 5 rows -> 34 bands
    _f('clamp', 16, 170, 29, 16, 16, 1, (1, 3, 34, 5, 1632), waves=BIG),
    # ---- channels: K = 16 with C in {16, 48, 96, 1024}; K = 24 with C = 96 (CT 2) and 144 (CT 1, 3; a request of 2 falls back to 1);
    # K = 32 with C = 192 (CT 1, 2, 3)
    _f('c16', 2, 5, 9, 16, 16, 2, (1, 1, 1, 3, 2)), _f('c1024', 1, 5, 9, 16, 1024, 1, (2, 1, 2, 4, 2)),
    _f('k24_c144_ct2_falls_back', 2, 5, 9, 24, 144, 2, (1, 1, 1, 3, 2), ct=2), _f('k24_c144_ct3_s1_gen', 2, 5, 9, 24, 144, 1, (3, 1, 2, 4, 4), ct=3, pair=GEN['relu']),
    _f('k24_c96_ct2_s1_gen', 2, 5, 9, 24, 96, 1, (2, 1, 2, 4, 4), pair=GEN['hsr6']), _f('k24_c144_ct1_s1', 2, 5, 9, 24, 144, 1, (1, 1, 2, 4, 4)),
    _f('k24_c96_ct2_s2_gen', 2, 5, 9, 24, 96, 2, (2, 1, 1, 3, 2), pair=GEN['hswish']),
    _f('k32_ct1_s1', 2, 5, 9, 32, 192, 1, (1, 1, 2, 4, 4), ct=1), _f('k32_ct2_s1', 2, 5, 9, 32, 192, 1, (2, 1, 2, 4, 4)),
    _f('k32_ct3_s2', 2, 5, 9, 32, 192, 2, (3, 1, 1, 3, 2), ct=3), _f('k32_ct1_s1_gen', 2, 5, 9, 32, 192, 1, (1, 1, 2, 4, 4), ct=1, pair=GEN['relu']),
    _f('k32_ct3_s1_gen', 2, 5, 9, 32, 192, 1, (3, 1, 2, 4, 4), ct=3, pair=GEN['none']), _f('k32_ct2_s2_gen', 2, 5, 9, 32, 192, 2, (2, 1, 1, 3, 2), pair=GEN['hsr6']),
    _f('k32_ct1_s2_gen', 2, 5, 9, 32, 192, 2, (1, 1, 1, 3, 2), ct=1, pair=GEN['relu']),
    _f('k16_ct1_s1_gen', 2, 5, 9, 16, 48, 1, (1, 1, 2, 4, 4), pair=GEN['r6r6']), _f('k16_ct2_s1_gen', 2, 5, 9, 16, 96, 1, (2, 1, 2, 4, 4), pair=GEN['hsr6']),
    _f('k16_ct2_s2_gen', 2, 5, 9, 16, 96, 2, (2, 1, 1, 3, 2), pair=GEN['relu']), _f('k16_ct3_s1', 2, 5, 9, 16, 96, 1, (3, 1, 2, 4, 4), ct=3),
    _f('k24_ct1_s2_gen', 2, 5, 9, 24, 144, 2, (1, 1, 1, 3, 2), pair=GEN['none']), _f('k24_ct1_s1_gen', 2, 5, 9, 24, 144, 1, (1, 1, 2, 4, 4), pair=GEN['hswish']),
    _f('k24_ct2_s1', 2, 5, 9, 24, 96, 1, (2, 1, 2, 4, 4)), _f('k24_ct3_s2', 2, 5, 9, 24, 144, 2, (3, 1, 1, 3, 2), ct=3),
    _f('k32_ct3_s1', 2, 5, 9, 32, 192, 1, (3, 1, 2, 4, 4), ct=3), _f('k32_ct3_s2_gen', 2, 5, 9, 32, 192, 2, (3, 1, 1, 3, 2), ct=3, pair=GEN['hswish']),
    _f('k32_ct2_s1_gen', 2, 5, 9, 32, 192, 1, (2, 1, 2, 4, 4), pair=GEN['r6r6']), _f('k16_ct3_s2_gen', 2, 5, 9, 16, 48, 2, (3, 1, 1, 3, 2), ct=3, pair=GEN['none']),
    # ---- the fast pair's pointers: none, only the scale, both (every other fast row: both)
    _f('fast_no_affine', 2, 7, 17, 16, 96, 2, (2, 1, 1, 4, 2), affine='none'), _f('fast_scale_only', 2, 7, 17, 24, 144, 1, (1, 2, 2, 4, 8), affine='scale'),
    # ---- views
    _f('view_s2', 3, 9, 33, 16, 96, 2, (2, 2, 2, 4, 12), layout='view', waves=BIG), _f('view_s1_gen', 2, 6, 15, 32, 192, 1, (2, 2, 2, 4, 8), layout='view', pair=GEN['relu']),
    _f('view_k24', 2, 7, 17, 24, 144, 2, (1, 1, 1, 4, 2), layout='view'), _f('view2_k24', 2, 7, 16, 24, 144, 1, (3, 2, 2, 4, 8), ct=3, layout='view2'),
    _f('view2_k24_s2_gen', 2, 7, 17, 24, 96, 2, (2, 1, 1, 4, 2), layout='view2', pair=GEN['hswish']),
]

# backward: knobs = dl3p_irb_set_bwd_plan(pass A waves, pass B workgroups); 0 = the defaults (they ask for far more bands than these
# maps have row steps: bands of 2, the minimum).  planA / planB = (nseg, nband, band, units, rows).
B = collections.namedtuple('B', 'name N H W K C s knobs pair layout act0 planA planB')
K3 = ((16, 96), (24, 144), (32, 192))


def _b(name, N, H, W, kc, s, planA, planB, knobs=(0, 0), pair=FAST, layout='contig', act0=NONE):
    return B(name, N, H, W, kc[0], kc[1], s, knobs, pair, layout, act0, planA, planB)


BWD = [
    # ---- stride 2: column steps (W + pad_l + 1) / 2 in {1, 16, 17, 33}, row steps (H + pad_t + 1) / 2 in {1, 2, 3, 5}
    _b('s2_w1', 1, 3, 1, K3[0], 2, (1, 1, 2, 6, 1), (1, 1, 2, 1, 8)),                                  # pass B: 1 unit (units % 4 = 1)
    _b('s2_w2', 2, 3, 2, K3[1], 2, (1, 1, 2, 18, 2), (1, 1, 2, 2, 8), pair=GEN['relu']),               # 2 units
    _b('s2_w31', 3, 3, 31, K3[2], 2, (1, 1, 2, 36, 3), (1, 1, 2, 3, 8)),                               # 16 column steps, 3 units
    _b('s2_w32', 1, 3, 32, K3[0], 2, (1, 1, 2, 6, 1), (1, 1, 2, 1, 8), pair=GEN['hswish'], layout='view'),
    _b('s2_w33', 1, 4, 33, K3[1], 2, (2, 1, 2, 18, 2), (2, 1, 2, 2, 8), layout='view'),                # 17 column steps
    _b('s2_w34', 1, 2, 34, K3[2], 2, (2, 1, 1, 24, 2), (2, 1, 1, 2, 8), pair=GEN['r6r6']),             # 1 row step
    _b('s2_w65', 1, 1, 65, K3[0], 2, (3, 1, 1, 18, 3), (3, 1, 1, 3, 8)),                               # 33 column steps, 1 row step
    _b('s2_w66_h5', 1, 5, 66, K3[1], 2, (3, 2, 2, 54, 6), (3, 2, 2, 6, 8), pair=GEN['none']),           # 3 row steps: bands of 2 and 1
    _b('s2_h9', 2, 9, 5, K3[2], 2, (1, 3, 2, 72, 6), (1, 3, 2, 6, 8), pair=GEN['hsr6'], layout='view', act0=RELU6),   # 5 row steps: 2, 2, 1
    _b('s2_h10_single', 2, 10, 6, K3[0], 2, (1, 1, 5, 12, 2), (1, 1, 5, 2, 8), knobs=(1, 1), pair=GEN['relu']),   # one band of 5
    _b('s2_k24_single', 3, 9, 7, K3[1], 2, (1, 1, 5, 27, 3), (1, 1, 5, 3, 8), knobs=(1, 1)),
    _b('s2_k32_gen', 2, 5, 9, K3[2], 2, (1, 2, 2, 48, 4), (1, 2, 2, 4, 8), pair=GEN['relu']),
    _b('s2_k24_gen', 2, 6, 9, K3[1], 2, (1, 2, 2, 36, 4), (1, 2, 2, 4, 8), pair=GEN['hswish']),
    _b('s2_two_rows_of_wgs', 3, 9, 33, K3[0], 2, (2, 3, 2, 108, 18), (2, 3, 2, 18, 8), layout='view'),   # 18 units: 5 workgroups of 8
    # ---- stride 1: column steps W in {1, 16, 17, 33}, row steps H in {1, 2, 3, 5}
    _b('s1_w1', 1, 3, 1, K3[1], 1, (1, 2, 2, 18, 2), (1, 2, 2, 2, 8)),
    _b('s1_w16', 3, 1, 16, K3[0], 1, (1, 1, 1, 18, 3), (1, 1, 1, 3, 8), pair=GEN['relu']),
    _b('s1_w17', 1, 2, 17, K3[2], 1, (2, 1, 2, 24, 2), (2, 1, 2, 2, 8)),
    _b('s1_w33', 1, 3, 33, K3[0], 1, (3, 2, 2, 36, 6), (3, 2, 2, 6, 8), layout='view'),
    _b('s1_h5', 1, 5, 7, K3[1], 1, (1, 3, 2, 27, 3), (1, 3, 2, 3, 8), pair=GEN['r6r6'], layout='view'),
    _b('s1_h5_single', 1, 5, 7, K3[2], 1, (1, 1, 5, 12, 1), (1, 1, 5, 1, 8), knobs=(1, 1), pair=GEN['hswish']),
    _b('s1_k16_hsr6', 2, 3, 18, K3[0], 1, (2, 2, 2, 48, 8), (2, 2, 2, 8, 8), pair=GEN['hsr6'], act0=RELU6),
    _b('s1_k24_none', 2, 4, 9, K3[1], 1, (1, 2, 2, 36, 4), (1, 2, 2, 4, 8), pair=GEN['none']),
    _b('s1_k32', 2, 5, 9, K3[2], 1, (1, 3, 2, 72, 6), (1, 3, 2, 6, 8), layout='view'),
    _b('s1_k32_gen', 1, 4, 20, K3[2], 1, (2, 2, 2, 48, 4), (2, 2, 2, 4, 8), pair=GEN['relu']),
]


def geom(c, pad=None):
    """Ho, Wo, pad_t, pad_l (TF SAME: the odd unit of padding goes to the end)"""
    pad = getattr(c, 'pad', 'same') if pad is None else pad

    def same(n):
        out = -(-n // c.s)
        return out, max((out - 1) * c.s + 3 - n, 0) // 2
    if pad == 'same':
        (Ho, pt), (Wo, pl) = same(c.H), same(c.W)
        return Ho, Wo, pt, pl
    pt, pb, pl, pr = pad
    return (c.H + pt + pb - 3) // c.s + 1, (c.W + pl + pr - 3) // c.s + 1, pt, pl


def fwd_kernel(c, ct):
    return 'irb_fwd<%d,%d,%d,%s>' % (c.K, ct, c.s, 'fast' if c.pair == FAST else 'generic')


def bwd_kernels(c):
    v = 'fast' if c.pair == FAST else 'generic'
    return 'irb_bwd_sums<%d,%d,%s>' % (c.K, c.s, v), 'irb_bwd_data<%d,%d,%s>' % (c.K, c.s, v)


# ------------------------------------------------------------------------------------------------------------------ activations
def act64(v, act):
    if act == NONE:
        return v
    if act == RELU:
        return np.maximum(v, 0)
    if act == RELU6:
        return np.clip(v, 0, 6)
    return v * np.clip(v + 3, 0, 6) / 6


def grad64(u, act):
    """act'(u) (TF: 0 at the kinks), and its magnitude m (hard-swish: hs + u / 6 can cancel)"""
    if act == NONE:
        one = np.ones_like(u)
        return one, one
    if act == RELU:
        d = (u > 0).astype(np.float64)
        return d, d
    if act == RELU6:
        d = ((u > 0) & (u < 6)).astype(np.float64)
        return d, d
    t = u + 3
    inside = ((t > 0) & (t < 6)) / 6.0
    hs = np.clip(t, 0, 6) / 6
    return hs + u * inside, hs + np.abs(u * inside)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def fma32(a, b, c):
    """fmaf on float32 arrays (exact product in float64; the double rounding is inside the '+ 1' of every bound)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def act32(v, act):
    """common.h act_apply in float32, operation for operation"""
    if act == NONE:
        return v
    if act == RELU:
        return np.maximum(v, np.float32(0))
    if act == RELU6:
        return np.clip(v, np.float32(0), np.float32(6))
    t = np.clip(v + np.float32(3), np.float32(0), np.float32(6)) * SIXTH
    return v * t


def grad32(u, act):
    """common.h act_grad in float32, operation for operation"""
    if act == NONE:
        return np.ones_like(u)
    if act == RELU:
        return (u > 0).astype(np.float32)
    if act == RELU6:
        return ((u > 0) & (u < 6)).astype(np.float32)
    t = u + np.float32(3)
    inside = ((t > 0) & (t < 6)).astype(np.float32) * SIXTH
    hs = np.clip(t, np.float32(0), np.float32(6)) * SIXTH
    return hs + u * inside


# ----------------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    """the float32 operands of a case, seeded by its name.  The BatchNorm coefficients are those of the float64 batch statistics of
    z (u ~ N(beta, gamma) with beta ~ 1, gamma ~ 1), the coefficient triple that of the float64 backward sums."""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    N, H, W, K, C = c.N, c.H, c.W, c.K, c.C
    Ho, Wo, pt, pl = geom(c)
    affine = getattr(c, 'affine', 'both')
    d = dict(x=rng.standard_normal((N, H, W, K)), w1=rng.standard_normal((K, C)) / np.sqrt(K), wdw=rng.standard_normal((3, 3, C)) * 0.4,
             dy=rng.standard_normal((N, Ho, Wo, C)), base=rng.standard_normal((N, H, W, K)), z0=rng.standard_normal((N, H, W, K)),
             mu0=rng.standard_normal(K) * 0.2, is0=rng.uniform(0.5, 2.0, K), s0=rng.uniform(0.5, 1.5, K), h0=rng.standard_normal(K) * 0.3 + 1.0)
    d['wdw'][:, :, 0] *= 1e-3                  # a channel with a small depthwise weight: its error must not hide behind the others
    d['wdw'][0, 2] *= 1e-2                     # ... and one low-magnitude tap
    sign = np.where(rng.uniform(size=K) < 0.25, -1.0, 1.0)
    d['xs'] = rng.uniform(0.5, 1.5, K) * sign if affine != 'none' else None
    d['xh'] = rng.standard_normal(K) * 0.3 if affine == 'both' else None
    d = {k: (None if v is None else f32(v)) for k, v in d.items()}
    xk = prologue64(d, c.pair[0])[0]
    z = xk.reshape(-1, K) @ d['w1'].astype(np.float64)
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.standard_normal(C) * 0.5 + 1.0
    mu, inv = z.mean(0), 1.0 / np.sqrt(z.var(0) + EPS)
    d['mu'], d['inv'] = f32(mu), f32(inv)
    d['sc'] = f32(gamma * d['inv'])
    d['sh'] = f32(beta - d['mu'].astype(np.float64) * d['sc'])
    # the BatchNorm-backward coefficient triple as dl3p_bn_bwd_finalize forms it: (gamma invstd, sum g' / M, sum g' xhat / M)
    if isinstance(c, B):
        r = pass_a_ref(d, c)
        M = N * H * W
        d['coef'] = f32(np.stack([d['sc'].astype(np.float64), r['rows'][0] / M, r['rows'][1] / M]))
    return d


# -------------------------------------------------------------------------------------------------------------------- geometry
def taps(a, c, Ho, Wo, pt, pl):
    """(ky, kx, a[n, oy*s - pt + ky, ox*s - pl + kx]) with zeros outside the map"""
    N, H, W, C = a.shape
    Hp, Wp = max((Ho - 1) * c.s + 3, pt + H), max((Wo - 1) * c.s + 3, pl + W)
    ap = np.zeros((N, Hp, Wp, C), dtype=a.dtype)
    ap[:, pt:pt + H, pl:pl + W] = a
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, ap[:, ky:ky + (Ho - 1) * c.s + 1:c.s, kx:kx + (Wo - 1) * c.s + 1:c.s]


def scatter(dy, w, c, pt, pl, fma=None, order=1):
    """depthwise^T: g[n, oy*s - pt + ky, ox*s - pl + kx] += w[ky, kx] * dy[n, oy, ox]"""
    N, Ho, Wo, C = dy.shape
    Hp, Wp = max((Ho - 1) * c.s + 3, pt + c.H), max((Wo - 1) * c.s + 3, pl + c.W)
    g = np.zeros((N, Hp, Wp, C), dtype=dy.dtype)
    for t in list(range(9))[::order]:
        ky, kx = divmod(t, 3)
        v = g[:, ky:ky + (Ho - 1) * c.s + 1:c.s, kx:kx + (Wo - 1) * c.s + 1:c.s]
        v[...] = v + dy * w[ky, kx] if fma is None else fma(dy, w[ky, kx], v)
    return g[:, pt:pt + c.H, pl:pl + c.W]


# ------------------------------------------------------------------------------------------------------------- float64 + bounds
def prologue64(d, act):
    """xk = act(x xs + xh) computed by one fma and the activation, and its bound dxk"""
    x = d['x'].astype(np.float64)
    if d['xs'] is None and d['xh'] is None and act == NONE:
        return x, np.zeros_like(x)
    s = 1.0 if d['xs'] is None else d['xs'].astype(np.float64)
    h = 0.0 if d['xh'] is None else d['xh'].astype(np.float64)
    xk = act64(x * s + h, act)
    return xk, U * (N_PRO[act] * (np.abs(x * s) + np.abs(h)) + N_ACT[act] * np.abs(xk))


def u_terms(d, c, backward):
    """u (N, H, W, C), its bound du, zc = z - mean and its bound dzc (backward only)"""
    K = c.K
    w1 = d['w1'].astype(np.float64)
    sc, sh = d['sc'].astype(np.float64), d['sh'].astype(np.float64)
    x = d['x'].astype(np.float64)
    xk, dxk = prologue64(d, c.pair[0])
    z = xk @ w1
    u = z * sc + sh
    fold = c.pair == FAST
    s = 1.0 if d['xs'] is None else d['xs'].astype(np.float64)
    h = np.zeros(K) if d['xh'] is None else d['xh'].astype(np.float64)
    if fold:
        Tz, Tb = np.abs(x * s) @ np.abs(w1), np.abs(h) @ np.abs(w1)
    else:
        Z, dZ = np.abs(xk) @ np.abs(w1), dxk @ np.abs(w1)
    if not backward:
        if fold:
            du = U * ((K + 4) * np.abs(sc) * Tz + (2 * K + 2) * (np.abs(sh) + np.abs(sc) * Tb))
        else:
            du = U * ((K + 3) * np.abs(sc) * Z + 2 * np.abs(sh)) + np.abs(sc) * dZ
        return u, du, None, None
    mu = d['mu'].astype(np.float64)
    zc = z - mu
    if fold:
        dzc = U * ((K + 3) * Tz + (2 * K + 2) * (Tb + np.abs(mu)))
    else:
        dzc = U * ((K + 3) * Z + (K + 2) * np.abs(mu)) + dZ
    du = np.abs(sc) * dzc + U * (2 * np.abs(zc * sc) + 3 * (np.abs(sc * mu) + np.abs(sh)))
    return u, du, zc, dzc


def fwd_ref(d, c):
    """-> y, its bound (N, Ho, Wo, C)"""
    Ho, Wo, pt, pl = geom(c)
    act = c.pair[1]
    u, du, _, _ = u_terms(d, c, False)
    a = act64(u, act)
    da = N_PRO[act] * du + N_ACT[act] * U * np.abs(a)
    w = d['wdw'].astype(np.float64)
    y, S, D = 0.0, 0.0, 0.0
    for (ky, kx, va), (_, _, vd) in zip(taps(a, c, Ho, Wo, pt, pl), taps(da, c, Ho, Wo, pt, pl)):
        y = y + va * w[ky, kx]
        S = S + np.abs(va) * np.abs(w[ky, kx])
        D = D + vd * np.abs(w[ky, kx])
    return y, U * 10 * S + D


def stat_ref(y):
    """the statistic rows from the device's OWN y (float32): (sum y, sum y^2) and the bound of summing n terms (n adds / n fmas)"""
    y = y.astype(np.float64)
    n = y.shape[0] * y.shape[1] * y.shape[2]
    val = np.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))])
    return val, (n + 1) * U * np.stack([np.abs(y).sum((0, 1, 2)), (y * y).sum((0, 1, 2))])


def ambiguous(u, du, act):
    amb = np.zeros(u.shape, dtype=bool)
    for k in KINKS[act]:
        amb |= np.abs(u - k) <= du
    return amb


def pass_a_ref(d, c):
    """-> dict: gwdw (3, 3, C) + bound; rows (2, C) + bound + slack; and what pass B builds on"""
    Ho, Wo, pt, pl = geom(c)
    act = c.pair[1]
    u, du, zc, dzc = u_terms(d, c, True)
    a = act64(u, act)
    da = N_PRO[act] * du + N_ACT[act] * U * np.abs(a)
    w, dy = d['wdw'].astype(np.float64), d['dy'].astype(np.float64)
    inv = d['inv'].astype(np.float64)
    n_out, n = c.N * Ho * Wo, c.N * c.H * c.W
    gw, gwb = np.zeros((3, 3, c.C)), np.zeros((3, 3, c.C))
    for (ky, kx, va), (_, _, vd) in zip(taps(a, c, Ho, Wo, pt, pl), taps(da, c, Ho, Wo, pt, pl)):
        gw[ky, kx] = (va * dy).sum((0, 1, 2))
        gwb[ky, kx] = (n_out + 1) * U * (np.abs(va) * np.abs(dy)).sum((0, 1, 2)) + (vd * np.abs(dy)).sum((0, 1, 2))
    da1, Sda = scatter(dy, w, c, pt, pl), scatter(np.abs(dy), np.abs(w), c, pt, pl)
    g, m = grad64(u, act)
    gp = da1 * g
    dgp = U * (10 + N_GRAD[act] + 2) * Sda * m + Sda * L_GRAD[act] * du
    amb = ambiguous(u, du, act)
    flip = np.abs(da1) * amb
    xhat = zc * inv
    rows = np.stack([gp.sum((0, 1, 2)), (gp * xhat).sum((0, 1, 2))])
    rowsb = np.stack([(n + 1) * U * np.abs(gp).sum((0, 1, 2)) + dgp.sum((0, 1, 2)),
                      (n + 3) * U * np.abs(gp * xhat).sum((0, 1, 2)) + ((dgp * np.abs(zc) + np.abs(gp) * dzc) * inv).sum((0, 1, 2))])
    slack = np.stack([flip.sum((0, 1, 2)), (flip * np.abs(xhat)).sum((0, 1, 2))])
    return dict(gwdw=gw, gwdw_b=gwb, rows=rows, rows_b=rowsb, rows_s=slack, u=u, du=du, zc=zc, dzc=dzc, gp=gp, Sda=Sda, m=m, amb=amb,
                flip=flip, share=float(amb.any(-1).mean()))


def pass_b_ref(d, c, accumulate, front, a=None):
    """-> dict: gw1 (K, C), gx (N, H, W, K) [+ base], front rows (2, K), each with bound (_b) and slack (_s)"""
    a = a or pass_a_ref(d, c)
    act = c.pair[1]
    c0, c1, c2 = (d['coef'][i].astype(np.float64) for i in range(3))
    inv, w1 = d['inv'].astype(np.float64), d['w1'].astype(np.float64)
    zc, dzc = a['zc'], a['dzc']
    dz = c0 * (a['gp'] - c1 - zc * inv * c2)
    T1, T2, T3 = np.abs(c0) * a['Sda'] * a['m'], np.abs(c0 * c2 * inv) * np.abs(zc), np.abs(c0 * c1)
    ddz = U * ((13 + N_GRAD[act]) * T1 + 5 * T2 + 4 * T3) + np.abs(c0 * c2 * inv) * dzc + np.abs(c0) * a['Sda'] * L_GRAD[act] * a['du']
    dflip = a['flip'] * np.abs(c0)
    n = c.N * c.H * c.W
    xk, dxk = prologue64(d, c.pair[0])
    if d['xs'] is None and d['xh'] is None and c.pair[0] == NONE:
        dxk = np.zeros_like(xk)
    X, DX = np.abs(xk).reshape(n, c.K), dxk.reshape(n, c.K)
    out = dict(gw1=xk.reshape(n, c.K).T @ dz.reshape(n, c.C),
               gw1_b=(n + 4) * U * (X.T @ np.abs(dz).reshape(n, c.C)) + DX.T @ np.abs(dz).reshape(n, c.C) + X.T @ ddz.reshape(n, c.C),
               gw1_s=X.T @ dflip.reshape(n, c.C))
    gx = dz @ w1.T
    S = np.abs(dz) @ np.abs(w1).T
    gxb = (c.C + 2) * U * S + ddz @ np.abs(w1).T
    if accumulate:
        base = d['base'].astype(np.float64)
        gx = gx + base
        gxb = gxb + U * (S + np.abs(base))
    out.update(gx=gx, gx_b=gxb, gx_s=dflip @ np.abs(w1).T)
    if front:
        act0 = c.act0
        z0 = d['z0']
        u0 = fma32(z0, d['s0'], d['h0'])                 # the device decides act0' on this float32 value
        g0, m0 = grad64(u0.astype(np.float64), act0)
        xh0 = (z0.astype(np.float64) - d['mu0'].astype(np.float64)) * d['is0'].astype(np.float64)
        ng = N_GRAD[act0]
        out['front'] = np.stack([(gx * g0).sum((0, 1, 2)), (gx * g0 * xh0).sum((0, 1, 2))])
        out['front_b'] = np.stack([(n + ng + 2) * U * (np.abs(gx) * m0).sum((0, 1, 2)) + (out['gx_b'] * m0).sum((0, 1, 2)),
                                   (n + ng + 5) * U * (np.abs(gx) * m0 * np.abs(xh0)).sum((0, 1, 2)) + (out['gx_b'] * m0 * np.abs(xh0)).sum((0, 1, 2))])
        out['front_s'] = np.stack([(out['gx_s'] * m0).sum((0, 1, 2)), (out['gx_s'] * m0 * np.abs(xh0)).sum((0, 1, 2))])
    return out


def inside(got, ref, bound, what, slack=None):
    """every element of `got` within bound (+ slack, zero wherever no activation branch is undecided) of ref -> largest err / bound"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    if slack is not None:
        err = np.maximum(err - slack, 0.0)
    ok = err <= bound                                      # (a NaN fails)
    if not ok.all():
        i = int(np.flatnonzero(~ok.reshape(-1))[0])
        raise AssertionError('%s: %d of %d elements out of bound; first at %s: got %r want %r (bound %.3g, err %.3g)' % (
            what, int((~ok).sum()), ok.size, np.unravel_index(i, ok.shape), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
            float(bound.reshape(-1)[i]), float(err.reshape(-1)[i])))
    return float((err / np.maximum(bound, 1e-300)).max())


# ----------------------------------------------------------------------------------------------- the kernels' operations in float32
def _chain(wf, x, init, order):
    """init + sum_k x[..., k] * wf[k] as K fmas, k in `order`"""
    acc = np.broadcast_to(f32(init), x.shape[:-1] + (wf.shape[1],)).copy()
    for k in list(range(wf.shape[0]))[::order]:
        acc = fma32(x[..., k:k + 1], wf[k], acc)
    return acc


def _ones(d, K):
    xs = np.ones(K, np.float32) if d['xs'] is None else d['xs']
    xh = np.zeros(K, np.float32) if d['xh'] is None else d['xh']
    return xs, xh


def fwd32(d, c, order):
    Ho, Wo, pt, pl = geom(c)
    xs, xh = _ones(d, c.K)
    if c.pair == FAST:
        wf = f32(f32(d['w1'] * xs[:, None]) * d['sc'][None])
        b = d['sh']
        if d['xh'] is not None:
            b = fma32(d['sc'], _chain(d['w1'], xh[None], np.zeros(c.C), 1)[0], d['sh'])
        u = _chain(wf, d['x'], b, order)
    else:
        xk = act32(fma32(d['x'], xs, xh), c.pair[0])
        u = fma32(_chain(d['w1'], xk, np.zeros(c.C), order), d['sc'], d['sh'])
    a = act32(u, c.pair[1])
    y = np.zeros((c.N, Ho, Wo, c.C), np.float32)
    for ky, kx, v in list(taps(a, c, Ho, Wo, pt, pl))[::order]:
        y = fma32(v, d['wdw'][ky, kx], y)
    return y


def _sum32(a, order):
    """float32 sum over the pixels, in one of two orders"""
    return np.sum(a.reshape(-1, a.shape[-1])[::order], axis=0, dtype=np.float32)


def bwd32(d, c, order, accumulate, front):
    """pass A and pass B in float32 -> dict with the names of pass_a_ref / pass_b_ref"""
    Ho, Wo, pt, pl = geom(c)
    xs, xh = _ones(d, c.K)
    xk = act32(fma32(d['x'], xs, xh), c.pair[0])
    if c.pair == FAST:
        zc0 = f32(_chain(d['w1'], xh[None], np.zeros(c.C), 1)[0] - d['mu'])
        zc = _chain(f32(d['w1'] * xs[:, None]), d['x'], zc0, order)
    else:
        zc = _chain(d['w1'], xk, -d['mu'], order)
    u = fma32(zc, d['sc'], fma32(d['sc'], d['mu'], d['sh']))
    act = c.pair[1]
    a, g = act32(u, act), grad32(u, act)
    gw = np.stack([_sum32(f32(v * d['dy']), order) for _, _, v in taps(a, c, Ho, Wo, pt, pl)]).reshape(3, 3, c.C)
    gp = f32(scatter(d['dy'], d['wdw'], c, pt, pl, fma=fma32, order=order) * g)
    rows = np.stack([_sum32(gp, order), f32(_sum32(f32(gp * zc), order) * d['inv'])])
    c0, c1, c2 = d['coef']
    gq = f32(scatter(d['dy'], f32(d['wdw'] * c0), c, pt, pl, fma=fma32, order=order) * g)
    dz = f32(gq + fma32(f32(f32(-c0 * c2) * d['inv']), zc, f32(-c0 * c1)))
    n = c.N * c.H * c.W
    gx = np.zeros((c.N, c.H, c.W, c.K), np.float32)
    for ch in list(range(c.C))[::order]:
        gx = fma32(dz[..., ch:ch + 1], d['w1'][:, ch], gx)
    if accumulate:
        gx = f32(gx + d['base'])
    gw1 = np.zeros((c.K, c.C), np.float32)
    X, DZ = xk.reshape(n, c.K), dz.reshape(n, c.C)
    for p in list(range(n))[::order]:
        gw1 = fma32(X[p][:, None], DZ[p][None], gw1)
    out = dict(gwdw=gw, rows=rows, gw1=gw1, gx=gx)
    if front:
        u0 = fma32(d['z0'], d['s0'], d['h0'])
        dd = f32(gx * grad32(u0, c.act0))
        xh0 = f32(f32(d['z0'] - d['mu0']) * d['is0'])
        out['front'] = np.stack([_sum32(dd, order), _sum32(f32(dd * xh0), order)])
    return out
