// The fp32 MFMA weight-gradient kernels: the tiled kernel and the streaming small-K.N kernel.  Included and instantiated
// by pwconv.hip only (after pw_gemm_kernels.h).
#pragma once
#include "pw_gemm_kernels.h"

// ------------------------------------------------------------------------------ weight gradient
// One workgroup = one 64(k) x 64(n) tile of GW over one slice of M; slices are summed by
// dl3p_reduce_rows (fixed order -> deterministic).  Both operands are staged in their natural
// [m][channel] layout (pitch 68: rows 4 apart land 16 banks apart) and read as ds_read_b32 fragments.
struct WgradParams {
  const float* X; int ldx; const float* scale; const float* shift; int act;
  const float* DY; int lddy;
  float* slabs;
  int M, K, N;
  int ktiles, ntiles, mchunk;
  // implicit-GEMM gather of X (GX instantiations; see GemmParams): row m = (n, y, x) over g_RH x g_RW output pixels,
  // column k = tap * g_C + c, element = input [N][g_SH][g_SW][ldx] at (y * g_mul + g_ay + ky * g_d, ...), zero outside
  int g_RH, g_RW, g_SH, g_SW, g_C, g_kw, g_mul, g_ay, g_ax, g_d;
  float g_invRW, g_invRH;   // 1 / g_RW, 1 / g_RH for divmod_small
  // BNA instantiations: DY is the gradient g of act(BN(z)), not of z.  dz = c0 * (g * act'(z*scale+shift) - c1 - xhat * c2)
  // (what dl3p_bn_bwd_apply writes) is formed while the tile is staged and, by the workgroups of the first k tile, written
  // to DZ for the data gradient that follows: the apply pass over (g, z, dz) and its launch disappear.
  const float* Z; int ldz;
  const float* b_scale; const float* b_shift; const float* b_mean; const float* b_invstd; const float* b_coef; int b_act;
  float* DZ; int lddz;
};

// q = a / d, *r = a % d for 0 <= a < 2^24 (exact in float) and 0 < d < 2^14: one multiply by the reciprocal and one
// correction step instead of the ~30-instruction 32-bit division (the weight-gradient gather decodes every staged row)
__device__ __forceinline__ int divmod_small(int a, int d, float inv, int* r) {
  int q = (int)((float)a * inv);
  int rem = a - q * d;
  if (rem < 0) { --q; rem += d; }
  if (rem >= d) { ++q; rem -= d; }
  *r = rem;
  return q;
}

// Tile = (64 KW) x (16 NW) of GW: wave w owns k rows [16 KW w, 16 KW (w+1)) and all NW column tiles.  Larger
// tiles re-read X (N / TN times) and DY (K / TK times) less often -- at 64 x 64 the 304 x 256 decoder layer
// pulls 2.7 GB through L2 for 0.6 GB of operands.  Loads are unconditional on clamped offsets, zeroed by select.
template <int KW, int NW, bool GX = false, bool BNA = false>
__global__ __launch_bounds__(256, 2) void pw_wgrad_kernel(WgradParams p) {
  constexpr int TK = 64 * KW, TN = 16 * NW;
  constexpr int XP = TK + 4, DP = TN + 4;      // pitches: rows 4 apart land 16 banks apart
  constexpr int XQ = TK / 4, DQ = TN / 4;      // float4 per staged row
  constexpr int NX = (32 * XQ) / 256, ND = (32 * DQ + 255) / 256;
  __shared__ __attribute__((aligned(16))) float Xs[32 * XP];
  __shared__ __attribute__((aligned(16))) float Ds[32 * DP];
  const int t = threadIdx.x, l = t & 63, w = t >> 6, l15 = l & 15, q = l >> 4;
  const int tile = blockIdx.x;
  const int kt = tile / p.ntiles, nt = tile - kt * p.ntiles;
  const int k0 = kt * TK, n0 = nt * TN;
  const int m_begin = blockIdx.y * p.mchunk;
  const int m_end = min(p.M, m_begin + p.mchunk);
  // per-thread staging constants
  int xr[NX], dr[ND];
  uint32_t xo[NX], dof[ND];
  bool xok[NX], dok[ND];
  float4 xsc[NX], xsh[NX];
  int gx_dy[GX ? NX : 1], gx_dx[GX ? NX : 1];
  uint32_t gx_ok = 0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const int idx = t + 256 * i;
    xr[i] = idx / XQ;
    const int c = k0 + (idx - xr[i] * XQ) * 4;
    xok[i] = c < p.K;
    xo[i] = (uint32_t)min(c, p.K - 4) * 4u;
    xsc[i] = make_float4(1.f, 1.f, 1.f, 1.f); xsh[i] = zero4();
    if (GX) {
      // this thread's k columns never change: tap offsets and channel of each, once
      const int k = min(c, p.K - 4);
      const int tap = k / p.g_C, ch = k - tap * p.g_C;
      const int ky = tap / p.g_kw, kx = tap - ky * p.g_kw;
      gx_dy[i] = p.g_ay + ky * p.g_d;
      gx_dx[i] = p.g_ax + kx * p.g_d;
      xo[i] = (uint32_t)ch * 4u;
      if (p.scale) { xsc[i] = ld4(p.scale + ch); xsh[i] = ld4(p.shift + ch); }
    } else if (p.scale) { xsc[i] = ld4(p.scale + min(c, p.K - 4)); xsh[i] = ld4(p.shift + min(c, p.K - 4)); }
  }
  // BNA: dz = bA * g * act'(z * bsc + bsh) - bC * z + bD per channel (bA = c0, bC = c0 * invstd * c2, bD = bC * mean - c0 * c1)
  float4 bA[BNA ? ND : 1], bC[BNA ? ND : 1], bD[BNA ? ND : 1], bsc[BNA ? ND : 1], bsh[BNA ? ND : 1];
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int idx = min(t + 256 * i, 32 * DQ - 1);
    dr[i] = idx / DQ;
    const int c = n0 + (idx - dr[i] * DQ) * 4;
    dok[i] = (t + 256 * i < 32 * DQ) && c < p.N;
    dof[i] = (uint32_t)min(c, p.N - 4) * 4u;
    if (BNA) {
      const int cc = min(c, p.N - 4);
      const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
      bsc[i] = p.b_scale ? ld4(p.b_scale + cc) : one;
      bsh[i] = p.b_shift ? ld4(p.b_shift + cc) : zero4();
      const float4 mu = ld4(p.b_mean + cc), is = ld4(p.b_invstd + cc);
      const float4 c0 = ld4(p.b_coef + cc), c1 = ld4(p.b_coef + p.N + cc), c2 = ld4(p.b_coef + 2 * p.N + cc);
      bA[i] = c0;
      bC[i] = mul4(mul4(c0, is), c2);
      bD[i] = make_float4(bC[i].x * mu.x - c0.x * c1.x, bC[i].y * mu.y - c0.y * c1.y, bC[i].z * mu.z - c0.z * c1.z,
                          bC[i].w * mu.w - c0.w * c1.w);
    }
  }
  const float act_lo = p.act == DL3P_ACT_NONE ? -DL3P_INF : 0.f;
  const float act_hi = (p.act == DL3P_ACT_NONE || p.act == DL3P_ACT_RELU) ? DL3P_INF : 6.f;
  const char* Xb = reinterpret_cast<const char*>(p.X);
  const char* Db = reinterpret_cast<const char*>(p.DY);
  const char* Zb = reinterpret_cast<const char*>(p.Z);
  char* DZb = reinterpret_cast<char*>(p.DZ);
  const bool write_dz = BNA && p.DZ != nullptr && kt == 0;
  float4 rx[NX], rd[ND], rz[BNA ? ND : 1];
  auto gather_x = [&](int m0_) {
    gx_ok = 0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int m = m0_ + xr[i];
      const int mc = min(m, m_end - 1);
      int x, y;
      const int row = divmod_small(mc, p.g_RW, p.g_invRW, &x);
      const int n = divmod_small(row, p.g_RH, p.g_invRH, &y);
      const int sy = y * p.g_mul + gx_dy[i], sx = x * p.g_mul + gx_dx[i];
      const bool ok = m < m_end && sy >= 0 && sx >= 0 && sy < p.g_SH && sx < p.g_SW;
      const uint32_t off = ok ? (((uint32_t)n * (uint32_t)(p.g_SH * p.g_SW) + (uint32_t)(sy * p.g_SW + sx)) * (uint32_t)p.ldx) * 4u + xo[i] : 0u;
      rx[i] = *reinterpret_cast<const float4*>(Xb + off);
      gx_ok |= ok ? (1u << i) : 0u;
    }
  };
#define WT_PREFETCH(m0_)                                                                                              \
  {                                                                                                                   \
    if (GX) gather_x(m0_);                                                                                            \
    else _Pragma("unroll") for (int i = 0; i < NX; ++i)                                                               \
      rx[i] = *reinterpret_cast<const float4*>(Xb + ((uint32_t)min((m0_) + xr[i], m_end - 1) * (uint32_t)p.ldx * 4u + xo[i]));   \
    _Pragma("unroll") for (int i = 0; i < ND; ++i)                                                                    \
      rd[i] = *reinterpret_cast<const float4*>(Db + ((uint32_t)min((m0_) + dr[i], m_end - 1) * (uint32_t)p.lddy * 4u + dof[i])); \
    if (BNA) _Pragma("unroll") for (int i = 0; i < ND; ++i)                                                           \
      rz[i] = *reinterpret_cast<const float4*>(Zb + ((uint32_t)min((m0_) + dr[i], m_end - 1) * (uint32_t)p.ldz * 4u + dof[i])); \
  }
  f32x4 acc[KW][NW];
#pragma unroll
  for (int a = 0; a < KW; ++a)
#pragma unroll
    for (int b = 0; b < NW; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (m_begin < m_end) WT_PREFETCH(m_begin)
  for (int m0 = m_begin; m0 < m_end; m0 += 32) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      float4 v = fma4(rx[i], xsc[i], xsh[i]);
      if (p.act >= DL3P_ACT_HSWISH) v = act_apply4(v, p.act);
      else v = make_float4(__builtin_amdgcn_fmed3f(v.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.y, act_lo, act_hi),
                           __builtin_amdgcn_fmed3f(v.z, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.w, act_lo, act_hi));
      const bool ok = xok[i] && (GX ? ((gx_ok >> i) & 1u) != 0 : m0 + xr[i] < m_end);
      *reinterpret_cast<float4*>(&Xs[xr[i] * XP + (t + 256 * i - xr[i] * XQ) * 4]) = ok ? v : zero4();
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const int idx = t + 256 * i;
      if (idx < 32 * DQ) {
        const bool ok = dok[i] && m0 + dr[i] < m_end;
        float4 v = make_float4(rd[i].x, rd[i].y, rd[i].z, rd[i].w);
        if (BNA) {
          const float4 z = rz[i];
          const float4 u = fma4(z, bsc[i], bsh[i]);
          const int act = p.b_act;
          v = make_float4(fmaf(bA[i].x, v.x * act_grad(u.x, act), fmaf(-bC[i].x, z.x, bD[i].x)),
                          fmaf(bA[i].y, v.y * act_grad(u.y, act), fmaf(-bC[i].y, z.y, bD[i].y)),
                          fmaf(bA[i].z, v.z * act_grad(u.z, act), fmaf(-bC[i].z, z.z, bD[i].z)),
                          fmaf(bA[i].w, v.w * act_grad(u.w, act), fmaf(-bC[i].w, z.w, bD[i].w)));
          if (write_dz && ok) st4(reinterpret_cast<float*>(DZb + ((uint32_t)(m0 + dr[i]) * (uint32_t)p.lddz * 4u + dof[i])), v);
        }
        *reinterpret_cast<float4*>(&Ds[dr[i] * DP + (idx - dr[i] * DQ) * 4]) = ok ? v : zero4();
      }
    }
    __syncthreads();
    if (m0 + 32 < m_end) WT_PREFETCH(m0 + 32)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float a[KW][4];
#pragma unroll
      for (int kw = 0; kw < KW; ++kw)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[kw][j] = Xs[(g * 16 + q * 4 + j) * XP + (w * KW + kw) * 16 + l15];
#pragma unroll
      for (int ni = 0; ni < NW; ++ni) {
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = Ds[(g * 16 + q * 4 + j) * DP + ni * 16 + l15];
#pragma unroll
        for (int kw = 0; kw < KW; ++kw)
#pragma unroll
          for (int j = 0; j < 4; ++j)   // D[n][k]: lane ends with 4 consecutive n for k = l15
            acc[kw][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[kw][j], acc[kw][ni], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#undef WT_PREFETCH
  float* slab = p.slabs + (size_t)blockIdx.y * p.K * p.N;
#pragma unroll
  for (int kw = 0; kw < KW; ++kw) {
    const int k = k0 + (w * KW + kw) * 16 + l15;
#pragma unroll
    for (int ni = 0; ni < NW; ++ni) {
      const int n = n0 + ni * 16 + q * 4;
      if (k < p.K && n < p.N)
        st4(slab + (size_t)k * p.N + n, make_float4(acc[kw][ni][0], acc[kw][ni][1], acc[kw][ni][2], acc[kw][ni][3]));
    }
  }
}

// ------------------------------------------------------------------------------ weight gradient, small K x N
// High-resolution layers have tiny kernels (16x96, 24x144, 32x192 ...) and millions of rows: the weight
// gradient is a pure stream over X and DY.  Here every WAVE owns the whole K x N gradient (KT x NTN
// accumulators) and walks its own 16-row tiles of M: it loads 16 whole rows of X and DY (contiguous
// 16-B lanes), writes them to a wave-private LDS slice, reads them back as MFMA fragments and multiplies.
// No workgroup barrier in the loop -- the 16 waves of a CU drift apart and cover each other's latencies --
// every input byte is read exactly once, and the next tile's loads are in flight during the MFMAs.
// The four waves of a workgroup are summed through LDS at the end (fixed order), one slab per workgroup.
template <int KT, int NTN, bool BNA = false>
__global__ __launch_bounds__(256, 2) void pw_wgrad_small_kernel(WgradParams p) {
  constexpr int KP = 16 * KT, NP = 16 * NTN;
  constexpr int XP = KP + 4, DP = NP + 4;          // pitches: rows 4 apart land 16 banks apart
  constexpr int WAVE_FLOATS = 16 * (XP + DP);
  constexpr int CF = BNA ? 5 * NP : 0;             // BNA: per-channel bA, bC, bD, scale, shift of the folded BatchNorm apply
  extern __shared__ __attribute__((aligned(16))) float ws_lds[];
  // layout: [scale KP][shift KP][BNA: 5 x NP coefficients][4 waves x WAVE_FLOATS]; the end-of-kernel reduction reuses it from 0
  float* sc_s = ws_lds;
  float* sh_s = ws_lds + KP;
  float* cf_s = ws_lds + 2 * KP;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, l15 = l & 15, q = l >> 4;
  float* Xs = ws_lds + 2 * KP + CF + w * WAVE_FLOATS;
  float* Ds = Xs + 16 * XP;
  for (int i = t; i < KP; i += 256) {
    sc_s[i] = (p.scale && i < p.K) ? p.scale[i] : 1.f;
    sh_s[i] = (p.scale && i < p.K) ? p.shift[i] : 0.f;
  }
  if (BNA) {
    // dz = bA * g * act'(z * scale + shift) - bC * z + bD  (bA = c0, bC = c0 * invstd * c2, bD = bC * mean - c0 * c1)
    for (int i = t; i < NP; i += 256) {
      const bool in = i < p.N;
      const float c0 = in ? p.b_coef[i] : 0.f, c1 = in ? p.b_coef[p.N + i] : 0.f, c2 = in ? p.b_coef[2 * p.N + i] : 0.f;
      const float bc = in ? c0 * p.b_invstd[i] * c2 : 0.f;
      cf_s[i] = c0;
      cf_s[NP + i] = bc;
      cf_s[2 * NP + i] = in ? bc * p.b_mean[i] - c0 * c1 : 0.f;
      cf_s[3 * NP + i] = (in && p.b_scale) ? p.b_scale[i] : 1.f;
      cf_s[4 * NP + i] = (in && p.b_shift) ? p.b_shift[i] : 0.f;
    }
  }
  // columns K..KP-1 / N..NP-1 of the wave's slices are never loaded: zero them once
  for (int i = l; i < 16 * XP; i += 64) Xs[i] = 0.f;
  for (int i = l; i < 16 * DP; i += 64) Ds[i] = 0.f;
  __syncthreads();

  const int k4 = p.K >> 2, n4 = p.N >> 2;          // float4 per row
  const int nx = 4 * p.K, nd = 4 * p.N;            // float4 per 16-row tile
  // per-lane constants of the i-th load of a tile: row within the tile, LDS offset, global offset
  int xrow[KT], drow[NTN];
  uint32_t xg[KT], dg[NTN], zg[BNA ? NTN : 1], og[BNA ? NTN : 1];
  int xl[KT], dl[NTN];
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int f = min(l + 64 * i, nx - 1);
    const int r = f / k4, c = f - r * k4;
    xrow[i] = (l + 64 * i < nx) ? r : 16;          // 16 = never valid
    xl[i] = r * XP + c * 4;
    xg[i] = ((uint32_t)r * (uint32_t)p.ldx + (uint32_t)c * 4u) * 4u;
  }
#pragma unroll
  for (int i = 0; i < NTN; ++i) {
    const int f = min(l + 64 * i, nd - 1);
    const int r = f / n4, c = f - r * n4;
    drow[i] = (l + 64 * i < nd) ? r : 16;
    dl[i] = r * DP + c * 4;
    dg[i] = ((uint32_t)r * (uint32_t)p.lddy + (uint32_t)c * 4u) * 4u;
    if (BNA) {
      zg[i] = ((uint32_t)r * (uint32_t)p.ldz + (uint32_t)c * 4u) * 4u;
      og[i] = ((uint32_t)r * (uint32_t)p.lddz + (uint32_t)c * 4u) * 4u;
    }
  }
  const float act_lo = p.act == DL3P_ACT_NONE ? -DL3P_INF : 0.f;
  const float act_hi = (p.act == DL3P_ACT_NONE || p.act == DL3P_ACT_RELU) ? DL3P_INF : 6.f;

  f32x4 acc[KT][NTN];
#pragma unroll
  for (int a = 0; a < KT; ++a)
#pragma unroll
    for (int b = 0; b < NTN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ntiles = (p.M + 15) >> 4;
  const int nwaves = gridDim.x * 4;
  const int gw = blockIdx.x * 4 + w;
  const char* Xb = reinterpret_cast<const char*>(p.X);
  const char* Db = reinterpret_cast<const char*>(p.DY);
  const char* Zb = reinterpret_cast<const char*>(p.Z);
  char* Ob = reinterpret_cast<char*>(p.DZ);
  float4 rx[KT], rd[NTN], rz[BNA ? NTN : 1];
  // (a macro, not a lambda: hipcc keeps a by-reference captured float4[] in scratch here)
#define WS_PREFETCH(tile_)                                                                          \
  {                                                                                                 \
    const int pm0 = (tile_) << 4;                                                                   \
    /* rows past M: the tile is loaded shifted up so every row is in bounds; see `back` below */    \
    const int pback = max(0, pm0 + 16 - p.M);                                                       \
    const uint32_t xb0 = (uint32_t)(pm0 - pback) * (uint32_t)p.ldx * 4u;                            \
    const uint32_t db0 = (uint32_t)(pm0 - pback) * (uint32_t)p.lddy * 4u;                           \
    _Pragma("unroll") for (int i = 0; i < KT; ++i) rx[i] = *reinterpret_cast<const float4*>(Xb + (xb0 + xg[i]));   \
    _Pragma("unroll") for (int i = 0; i < NTN; ++i) rd[i] = *reinterpret_cast<const float4*>(Db + (db0 + dg[i]));  \
    if (BNA) {                                                                                      \
      const uint32_t zb0 = (uint32_t)(pm0 - pback) * (uint32_t)p.ldz * 4u;                          \
      _Pragma("unroll") for (int i = 0; i < NTN; ++i) rz[i] = *reinterpret_cast<const float4*>(Zb + (zb0 + zg[i])); \
    }                                                                                               \
  }
  WS_PREFETCH(min(gw, ntiles - 1))
  for (int tile = gw; tile < ntiles; tile += nwaves) {
    const int m0 = tile << 4;
    const int back = max(0, m0 + 16 - p.M);        // the tile was loaded shifted up by `back` rows
    // stage: rows [0, back) of the shifted tile belong to the previous tile -> zero (X only: 0 * dy = 0)
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      if (xrow[i] < 16) {
        const float4 s4 = *reinterpret_cast<const float4*>(&sc_s[xl[i] - xrow[i] * XP]);
        const float4 h4 = *reinterpret_cast<const float4*>(&sh_s[xl[i] - xrow[i] * XP]);
        float4 v = fma4(rx[i], s4, h4);
        if (p.act >= DL3P_ACT_HSWISH) v = act_apply4(v, p.act);
        else v = make_float4(__builtin_amdgcn_fmed3f(v.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.y, act_lo, act_hi),
                             __builtin_amdgcn_fmed3f(v.z, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.w, act_lo, act_hi));
        *reinterpret_cast<float4*>(&Xs[xl[i]]) = xrow[i] >= back ? v : zero4();
      }
    }
#pragma unroll
    for (int i = 0; i < NTN; ++i)
      if (drow[i] < 16) {
        float4 v = make_float4(rd[i].x, rd[i].y, rd[i].z, rd[i].w);
        if (BNA) {
          const int cf = dl[i] - drow[i] * DP;       // channel of this float4
          const float4 a4 = *reinterpret_cast<const float4*>(&cf_s[cf]);
          const float4 c4 = *reinterpret_cast<const float4*>(&cf_s[NP + cf]);
          const float4 d4 = *reinterpret_cast<const float4*>(&cf_s[2 * NP + cf]);
          const float4 s4 = *reinterpret_cast<const float4*>(&cf_s[3 * NP + cf]);
          const float4 h4 = *reinterpret_cast<const float4*>(&cf_s[4 * NP + cf]);
          const float4 z = rz[i];
          const float4 u = fma4(z, s4, h4);
          const int act = p.b_act;
          v = make_float4(fmaf(a4.x, v.x * act_grad(u.x, act), fmaf(-c4.x, z.x, d4.x)),
                          fmaf(a4.y, v.y * act_grad(u.y, act), fmaf(-c4.y, z.y, d4.y)),
                          fmaf(a4.z, v.z * act_grad(u.z, act), fmaf(-c4.z, z.z, d4.z)),
                          fmaf(a4.w, v.w * act_grad(u.w, act), fmaf(-c4.w, z.w, d4.w)));
          // (rows [0, back) of a shifted last tile were written by the tile before it)
          if (p.DZ && drow[i] >= back)
            st4(reinterpret_cast<float*>(Ob + ((uint32_t)(m0 - back) * (uint32_t)p.lddz * 4u + og[i])), v);
        }
        *reinterpret_cast<float4*>(&Ds[dl[i]]) = v;
      }
    WS_PREFETCH(min(tile + nwaves, ntiles - 1))   // unconditional (the last one is a harmless re-read)
    // fragments: reduction index m = 4q + j; lane l15 = channel within the 16-wide tile
    float b[NTN][4];
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) b[nt][j] = Ds[(4 * q + j) * DP + nt * 16 + l15];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      float a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = Xs[(4 * q + j) * XP + kt * 16 + l15];
#pragma unroll
      for (int nt = 0; nt < NTN; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nt][j], a[j], acc[kt][nt], 0, 0, 0);
    }
  }
  // sum the four waves (fixed order 0+1+2+3) and write this workgroup's slab
  __syncthreads();
  float4* red = reinterpret_cast<float4*>(ws_lds);
  if (w > 0) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int nt = 0; nt < NTN; ++nt)
        red[((w - 1) * KT * NTN + kt * NTN + nt) * 64 + l] =
            make_float4(acc[kt][nt][0], acc[kt][nt][1], acc[kt][nt][2], acc[kt][nt][3]);
  }
  __syncthreads();
  if (w == 0) {
    float* slab = p.slabs + (size_t)blockIdx.x * p.K * p.N;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int nt = 0; nt < NTN; ++nt) {
        float4 v = make_float4(acc[kt][nt][0], acc[kt][nt][1], acc[kt][nt][2], acc[kt][nt][3]);
#pragma unroll
        for (int ww = 0; ww < 3; ++ww) v = add4(v, red[(ww * KT * NTN + kt * NTN + nt) * 64 + l]);
        const int k = kt * 16 + l15, n = nt * 16 + q * 4;
        if (k < p.K && n < p.N) st4(slab + (size_t)k * p.N + n, v);
      }
  }
}

template <int KT, int NTN, bool BNA = false>
static constexpr size_t wgrad_small_lds() {
  constexpr size_t stage = sizeof(float) * (size_t)(2 * 16 * KT + (BNA ? 5 * 16 * NTN : 0) + 4 * 16 * (16 * KT + 4 + 16 * NTN + 4));
  constexpr size_t red = 16 * (size_t)(3 * KT * NTN * 64);
  return stage > red ? stage : red;
}
