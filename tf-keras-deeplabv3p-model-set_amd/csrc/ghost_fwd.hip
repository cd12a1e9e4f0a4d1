// Fused ghost-module FORWARD (deeplabv3p_ghostnet.py:81-153, GhostModule with ratio 2 and dw_size 3) for a module whose
// BatchNorm coefficients are known before the launch (inference, or a frozen backbone):
//   z1 = a W1 (primary 1x1 conv, K -> C)          -> y[..., 0:C)
//   z2 = DepthwiseConv2D(3x3, stride 1, 'same')(act1(z1 s1 + h1))   -> y[..., C:2C)
// in ONE launch: z1 goes from the matrix pipe to memory and, in registers, on into the depthwise conv; it is never read back.
// K + 2C floats per pixel move instead of the K + 3C of dl3p_pwconv_fwd + dl3p_dwconv2d_fwd.
//
// The sibling of irb_fwd.hip (stride 1 form) with the conventions of irb_common.h: the pixel on the lane, 16-channel tiles on
// v_mfma_f32_16x16x4_f32, input rows walked once with the three output rows they feed in rolling registers, horizontal taps by
// DPP row shifts.  What differs: BOTH halves are stored, the coefficients are given, and C need not fill its last tile
// (C = 8, 12, 24, 36 against 16-wide tiles).
//
// One wave = one (image, segment of 14 output columns, band of output rows), all ceil(C / 16) channel tiles.  Lane j of a 16-lane
// row holds input column 14 seg - 1 + j; lanes 1 .. 14 produce (and store) the outputs centred there, so every column is expanded
// 16 / 14 times, and a band of B rows expands B + 2: the halo recompute factor is 16 / 14 * (B + 2) / B.  z1 is stored by the one
// wave that owns the pixel (lanes 1 .. 14, the band's own rows); a halo pixel's z1 is bit-identical in both waves (same chain).
//
// Padding is by SELECTION: an out-of-image column or row is loaded from a clamped in-image address and its activation is replaced
// by 0 (zero AFTER BatchNorm and activation, what 'same' means); channels >= C of the last tile get weight 0, are never stored, and
// their coefficients are read from a clamped in-range index.  Nothing beyond K input channels, C coefficients or 2C output channels
// of a pixel is touched, so NaN in the neighbouring channels of a wider buffer cannot reach an output.  Offsets are 64-bit.
#include "irb_common.h"

struct GhostParams {
  const float* x; int ldx; const float* xs; const float* xh; int xact;   // module input + its lazy prologue
  const float* w1;                                                        // primary kernel [K][C]
  const float* s1; const float* h1; int act1;                             // BatchNorm 1 scale / shift + activation
  const float* wdw;                                                       // cheap-operation kernel [9][C]
  float* y; int ldy;                                                      // [N][H][W][ldy]: z1 in [0, C), z2 in [C, 2C)
  int N, H, W, C;
  int nseg, nband, band, units;
};

// a lane's KQ = K / 4 contiguous input channels: 16-byte loads where KQ is a multiple of 4, 8-byte loads otherwise (KQ is even)
template <int KQ>
__device__ __forceinline__ void ghost_load_x(const float* p, float (&v)[KQ]) {
  if constexpr (KQ % 4 == 0) {
#pragma unroll
    for (int i = 0; i < KQ / 4; ++i) {
      const float4 t = ld4(p + 4 * i);
      v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
  } else {
    static_assert(KQ % 2 == 0, "K / 4 must be even");
#pragma unroll
    for (int i = 0; i < KQ / 2; ++i) {
      const float2 t = *reinterpret_cast<const float2*>(p + 2 * i);
      v[2 * i] = t.x; v[2 * i + 1] = t.y;
    }
  }
}

template <int KQ, int CT>
__global__ __launch_bounds__(256) void ghost_fwd_kernel(GhostParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int unit = blockIdx.x * 4 + wave;            // (scalar)
  if (unit >= p.units) return;                       // (no barrier in this kernel)
  int rr = unit;
  const int band = rr % p.nband; rr /= p.nband;
  const int seg = rr % p.nseg;
  const int n = rr / p.nseg;
  const int H = p.H, W = p.W, C = p.C;

  // per-lane constants.  A operand: lane (j, q) holds W1[q KQ + s][16 ct + j]; result registers: channels 16 ct + 4 q + 0 .. 3
  float wf[CT][KQ], xs[KQ], xh[KQ];
  float4 sc[CT], sh[CT], wt[CT][9];
  bool qok[CT];
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    xs[s] = p.xs ? p.xs[q * KQ + s] : 1.f;
    xh[s] = p.xh ? p.xh[q * KQ + s] : 0.f;
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int ch = 16 * ct + j;
    const bool chok = ch < C;
    const int chc = chok ? ch : 0;
#pragma unroll
    for (int s = 0; s < KQ; ++s) {
      const float w = p.w1[(size_t)(q * KQ + s) * C + chc];
      wf[ct][s] = chok ? w : 0.f;
    }
    qok[ct] = 16 * ct + 4 * q < C;                   // (C is a multiple of 4: a quad is whole or absent)
    const int cq = qok[ct] ? 16 * ct + 4 * q : 0;
    sc[ct] = make_float4(p.s1[cq], p.s1[cq + 1], p.s1[cq + 2], p.s1[cq + 3]);
    sh[ct] = make_float4(p.h1[cq], p.h1[cq + 1], p.h1[cq + 2], p.h1[cq + 3]);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float* wp = p.wdw + (size_t)t * C + cq;
      wt[ct][t] = make_float4(wp[0], wp[1], wp[2], wp[3]);
    }
  }
  const int xact = p.xact, act1 = p.act1;
  const int oy0 = band * p.band;
  const int oy1 = oy0 + p.band < H ? oy0 + p.band : H;
  const int nrows = oy1 - oy0;

  // column geometry: 'same' 3x3 stride 1 has one column of padding in front
  const int ix = seg * 14 - 1 + j;                   // the column this lane expands == the output column it produces
  const bool va = ix >= 0 && ix < W;
  const bool out_ok = j >= 1 && j <= 14 && ix < W;   // (j >= 1 makes ix >= 0)
  const int ixc = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
  const size_t rowpitch_x = (size_t)W * p.ldx, rowpitch_y = (size_t)W * p.ldy;
  const float* xn_ = p.x + (size_t)n * H * rowpitch_x + (size_t)ixc * p.ldx + q * KQ;
  float* yn_ = p.y + (size_t)n * H * rowpitch_y + (size_t)ixc * p.ldy + 4 * q;

  auto load_row = [&](int iy, float (&r)[KQ]) {
    const int iyc = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
    ghost_load_x<KQ>(xn_ + (size_t)iyc * rowpitch_x, r);
  };

  float X0[KQ], X1[KQ], X2[KQ];
  float4 a2[CT], a1[CT], a0[CT];                      // output rows iy - 1, iy, iy + 1 of the input row iy being expanded
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) { a2[ct] = zero4(); a1[ct] = zero4(); a0[ct] = zero4(); }
  int iy = oy0 - 1;
  load_row(iy, X0);
  load_row(iy + 1, X1);
  auto step = [&](int t, float (&xc)[KQ], float (&xn)[KQ]) {
    load_row(iy + 2, xn);                             // two rows ahead, into the set the step after the next computes from
    if (iy >= 0 && iy < H) {                          // (wave-uniform)
#pragma unroll
      for (int s = 0; s < KQ; ++s) xc[s] = act_apply(fmaf(xc[s], xs[s], xh[s]), xact);
      const bool own = t >= 1 && t <= nrows;          // the band's own rows: this wave stores their z1
      float* yrow = yn_ + (size_t)iy * rowpitch_y;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        irb_f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KQ; ++s) z = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ct][s], xc[s], z, 0, 0, 0);
        const float4 z4 = irb_f4_to_float4(z);
        if (own && out_ok && qok[ct]) st4(yrow + 16 * ct, z4);
        const float4 ta = irb_sel4(va, act_apply4(fma4(z4, sc[ct], sh[ct]), act1));
        const float4 tl = irb_from_prev4(ta), tr = irb_from_next4(ta);
        a2[ct] = fma4(wt[ct][6], tl, a2[ct]);
        a2[ct] = fma4(wt[ct][7], ta, a2[ct]);
        a2[ct] = fma4(wt[ct][8], tr, a2[ct]);
        a1[ct] = fma4(wt[ct][3], tl, a1[ct]);
        a1[ct] = fma4(wt[ct][4], ta, a1[ct]);
        a1[ct] = fma4(wt[ct][5], tr, a1[ct]);
        a0[ct] = mul4(wt[ct][0], tl);
        a0[ct] = fma4(wt[ct][1], ta, a0[ct]);
        a0[ct] = fma4(wt[ct][2], tr, a0[ct]);
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) a0[ct] = zero4();
    }
    if (t >= 2 && out_ok) {                           // output row oy0 + t - 2 = iy - 1 is complete
      float* yp = yn_ + (size_t)(iy - 1) * rowpitch_y + C;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (qok[ct]) st4(yp + 16 * ct, a2[ct]);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { a2[ct] = a1[ct]; a1[ct] = a0[ct]; }
    ++iy;
  };
  int t = 0;
  for (; t + 2 < nrows + 2; t += 3) {
    step(t, X0, X2);
    step(t + 1, X1, X0);
    step(t + 2, X2, X1);
  }
  if (t < nrows + 2) { step(t, X0, X2); ++t; }
  if (t < nrows + 2) { step(t, X1, X0); ++t; }
}

static bool ghost_k_ok(int K) { return K == 16 || K == 24 || K == 48 || K == 72; }

extern "C" int dl3p_ghost_fwd_supported(int N, int H, int W, int K, int C) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  if (!ghost_k_ok(K) || C % 4 != 0 || C < 4 || C > 48) return 0;
  if (K > 24 && C > 16) return 0;                               // (the long reductions are built for one channel tile)
  if ((long long)N * H * W >= (1ll << 31) / 16) return 0;       // (work units and pixel indices stay in int; offsets are 64-bit)
  return 1;
}

static void ghost_plan(GhostParams& p) {
  p.nseg = ceil_div(p.W, 14);
  const long long per = (long long)p.N * p.nseg;
  int nband = (int)ceil_div_ll(4096, per);
  if (nband < 1) nband = 1;
  int band = ceil_div(p.H, nband);
  const int min_band = 4;
  if (band < min_band) band = p.H < min_band ? p.H : min_band;
  p.band = band;
  p.nband = ceil_div(p.H, band);
  p.units = (int)(per * p.nband);
}

template <int KQ, int MAXCT>
static bool ghost_launch(const GhostParams& p, hipStream_t st) {
  const dim3 grid(ceil_div(p.units, 4)), block(256);
  const int ct = ceil_div(p.C, 16);
  if (ct == 1) dl3p_launch(ghost_fwd_kernel<KQ, 1>, grid, block, 0, st, p);
  else if constexpr (MAXCT >= 3) {
    if (ct == 2) dl3p_launch(ghost_fwd_kernel<KQ, 2>, grid, block, 0, st, p);
    else if (ct == 3) dl3p_launch(ghost_fwd_kernel<KQ, 3>, grid, block, 0, st, p);
    else return false;
  } else return false;
  return true;
}

extern "C" int dl3p_ghost_fwd(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act, const float* w1,
                              const float* s1, const float* h1, int act1, const float* wdw, float* y, int ldy, int N, int H,
                              int W, int K, int C, void* stream) {
  DL3P_CHECK_ARG(x && w1 && s1 && h1 && wdw && y, "dl3p_ghost_fwd: null pointer");
  DL3P_CHECK_ARG(dl3p_ghost_fwd_supported(N, H, W, K, C), "dl3p_ghost_fwd: unsupported shape N=%d H=%d W=%d K=%d C=%d", N, H, W, K, C);
  DL3P_CHECK_ARG(ldx >= K && ldx % 4 == 0 && aligned16(x) && ldy >= 2 * C && ldy % 4 == 0 && aligned16(y),
                 "dl3p_ghost_fwd: bad layout (ldx=%d, ldy=%d; multiples of 4, 16-byte aligned bases)", ldx, ldy);
  DL3P_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "dl3p_ghost_fwd: in_scale and in_shift come together");
  DL3P_CHECK_ARG(in_act >= DL3P_ACT_NONE && in_act <= DL3P_ACT_HSIGMOID && act1 >= DL3P_ACT_NONE && act1 <= DL3P_ACT_HSIGMOID,
                 "dl3p_ghost_fwd: unknown activation code");
  GhostParams p = {};
  p.x = x; p.ldx = ldx; p.xs = in_scale; p.xh = in_shift; p.xact = in_act; p.w1 = w1; p.s1 = s1; p.h1 = h1; p.act1 = act1;
  p.wdw = wdw; p.y = y; p.ldy = ldy; p.N = N; p.H = H; p.W = W; p.C = C;
  ghost_plan(p);
  hipStream_t st = (hipStream_t)stream;
  bool launched = false;
  if (K == 16) launched = ghost_launch<4, 3>(p, st);
  else if (K == 24) launched = ghost_launch<6, 3>(p, st);
  else if (K == 48) launched = ghost_launch<12, 1>(p, st);
  else if (K == 72) launched = ghost_launch<18, 1>(p, st);
  DL3P_CHECK_ARG(launched, "dl3p_ghost_fwd: no kernel for K=%d C=%d", K, C);
  DL3P_CHECK_LAUNCH("dl3p_ghost_fwd");
  return DL3P_OK;
}
