// 2x2 stride-2 transposed convolution (Conv2DTranspose(filters, 2, strides=(2, 2)) + bias) on the MFMA f32 path
// (v_mfma_f32_16x16x4_f32) for gfx950: the up-path of the U-Net family.
//
// Replaces Conv2DTranspose(512 / 256 / 128 / 64, 2, strides=(2, 2)) at the reference's unet/models/unet.py:47,53,59,65
// (unet_standard) and :116-134 (unet_lite).
//
// With k == stride == 2 and no padding every output pixel has exactly ONE tap, so nothing is masked and nothing overlaps:
//   fwd    Y[pix(m,q)][co] = sum_ci act(X[m][ci]*scale+shift) W[q][co][ci] + bias[co]     a GEMM [M][Cin] x [Cin][4 Cout], scattered rows
//   dgrad  GX[m][ci] (+)= sum_{q,co} DY[pix(m,q)][co] W[q][co][ci]                        a GEMM [M][4 Cout] x [4 Cout][Cin], gathered rows
//   wgrad  GW[q][co][ci] = sum_m act(X[m][ci]) DY[pix(m,q)][co]; GB[co] = sum DY         split over M, slab reduce, gathered DY
// m = (n, y, x) over the N x H x W input map, q = 2 dy + dx, pix(m, q) = (n, 2y + dy, 2x + dx) = pixel 4m - 2x + dy 2W + dx of the output.
// The Keras kernel as stored, (2, 2, Cout, Cin), IS the B operand of both GEMMs with no re-laid copy: read as [4 Cout][Cin] it is the
// forward's [Nout][Kred] operand, read as [4 Cout][Cin] = [Kred][Nout] it is the data gradient's.
//
// The structure is pwconv.hip's tiled kernel (128-row x 64-column tile, 32-deep K steps, operands swapped in the MFMA so a lane ends
// up with 4 consecutive channels of one pixel, A tile through LDS at pitch 36, register double buffering, persistent workgroups
// over M tiles, every global load of the K loop unconditional on a clamped 32-bit byte offset with invalid lanes selected to zero).
// What differs is WHERE rows live: the forward's epilogue computes the destination pixel of each 16-byte store from (m, column / Cout)
// -- a 4-channel group never straddles a quadrant because Cout % 4 == 0 -- and the gradients gather their dY operand from the four
// output pixels of each input row while it is staged.
#include "common.h"
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

struct DeconvParams {
  const float* A; int lda;                 // fwd: x [M][lda]; dgrad: dY [4 M pixels][lda]
  const float* scale; const float* shift; int act;   // fwd prologue on x
  const float* B;                          // the Keras kernel (2, 2, Cout, Cin)
  const float* bias;
  float* Y; int ldy;                       // fwd: y [4 M pixels][ldy]; dgrad: gx [M][ldy]
  int M, K, N;                             // GEMM sizes: fwd K = Cin, N = 4 Cout; dgrad K = 4 Cout, N = Cin
  int W, Cout;                             // width of the INPUT map; filters
  int accumulate;
  int num_m_tiles;
};

// quadrant q = c / Cout for 0 <= c < 4 Cout without a division; *co = c % Cout
__device__ __forceinline__ int quadrant(int c, int Cout, int* co) {
  const int q = (c >= Cout ? 1 : 0) + (c >= 2 * Cout ? 1 : 0) + (c >= 3 * Cout ? 1 : 0);
  *co = c - q * Cout;
  return q;
}
// output pixel index of tap q of input row m (x = m % W): (n, 2y + dy, 2x + dx) flattened over [N][2H][2W]
__device__ __forceinline__ uint32_t out_pixel(uint32_t m, uint32_t W, int q) {
  const uint32_t x = m % W;
  return 4u * m - 2u * x + (uint32_t)(q >> 1) * 2u * W + (uint32_t)(q & 1);
}

constexpr int BKT = 32;           // K step
constexpr int AP = BKT + 4;       // A pitch: rows 4 apart land 16 banks apart -> ds_read_b128 conflict-free
constexpr int MI = 2, NT = 4;     // 4 waves x MI tiles of 16 rows; NT tiles of 16 columns: 8 independent accumulators per wave
constexpr int BM = 64 * MI, BN = 16 * NT;

// DG = false: forward (B read as [Nout][Kred], scatter epilogue + bias);  DG = true: data gradient (A gathered, B read as [Kred][Nout])
template <bool DG>
__global__ __launch_bounds__(256, 2) void deconv_gemm_kernel(DeconvParams p) {
  constexpr int KQ = BKT / 4;       // float4 per K-tile row
  constexpr int RP = 256 / KQ;      // A rows staged per pass of the 256 threads
  constexpr int NA = BM / RP;
  constexpr int BPITCH = DG ? (BN + 4) : AP;
  constexpr int BS_FLOATS = DG ? BKT * BPITCH : BN * AP;
  constexpr int NB4 = (KQ * BN) / 256;      // float4 per thread for the B tile (exact)
  constexpr int EPITCH = BN + 4;
  constexpr int RW = 16 * MI;               // rows per wave
  __shared__ __attribute__((aligned(16))) float As[BM * AP];
  __shared__ __attribute__((aligned(16))) float Bs[BS_FLOATS];
  __shared__ __attribute__((aligned(16))) float Es[4 * RW * EPITCH];   // epilogue transpose buffer, wave-private slices

  const int t = threadIdx.x;
  const int l = t & 63;
  const int w = t >> 6;
  const int l15 = l & 15;
  const int q = l >> 4;
  const int n0 = blockIdx.y * BN;
  const int nk = (p.K + BKT - 1) / BKT;
  const int my_tiles = (p.num_m_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int it_total = my_tiles * nk;

  const int ar = t / KQ;         // A row within a pass of RP rows
  const int akq = (t % KQ) * 4;  // A k offset within the K tile
  const char* Ab = reinterpret_cast<const char*>(p.A);
  const char* Bb = reinterpret_cast<const char*>(p.B);
  const uint32_t ldb = DG ? (uint32_t)p.N : (uint32_t)p.K;

  float4 ra[NA];
  float4 rb[NB4];
  float4 rsc = make_float4(1.f, 1.f, 1.f, 1.f), rsh = zero4();
  uint32_t a_row[NA];        // fwd: byte offset of this thread's A rows; dgrad: output pixel of tap 0 of this thread's rows
  uint32_t b_off[NB4];
  bool b_nok[NB4];
  int pf_m0 = -1;
#pragma unroll
  for (int i = 0; i < NB4; ++i) {
    const int idx = t + 256 * i;
    if (DG) {
      const int kk = idx / (BN / 4), nq = idx - kk * (BN / 4);
      const int n = n0 + nq * 4;
      b_nok[i] = n < p.N;
      b_off[i] = (uint32_t)min(n, p.N - 4) * 4u;            // + k * ldb * 4 per K-step
    } else {
      const int n = n0 + idx / KQ;
      b_nok[i] = n < p.N;
      b_off[i] = (uint32_t)min(n, p.N - 1) * ldb * 4u;      // + k * 4 per K-step
    }
  }

  // Every global load of the K loop is UNCONDITIONAL on a clamped 32-bit byte offset (rows >= M re-read row M-1, columns >= K
  // re-read the last float4); invalid lanes are zeroed by a select when the tile is written to LDS.  Hosts reject operands of 4 GiB.
  auto prefetch = [&](int it) {
    const int kt = it % nk;
    const int mt = blockIdx.x + (it / nk) * gridDim.x;
    const int m0 = mt * BM;
    const int k0 = kt * BKT;
    const int k = min(k0 + akq, p.K - 4);
    if (m0 != pf_m0) {
      pf_m0 = m0;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const uint32_t m = (uint32_t)min(m0 + ar + RP * i, p.M - 1);
        a_row[i] = DG ? out_pixel(m, (uint32_t)p.W, 0) : m * (uint32_t)p.lda * 4u;
      }
    }
    if (DG) {
      // four consecutive k are four channels of one tap (Cout % 4 == 0): the gather keeps the 16-byte loads
      int co;
      const int tap = quadrant(k, p.Cout, &co);
      const uint32_t poff = (uint32_t)(tap >> 1) * 2u * (uint32_t)p.W + (uint32_t)(tap & 1);
#pragma unroll
      for (int i = 0; i < NA; ++i)
        ra[i] = *reinterpret_cast<const float4*>(Ab + (((a_row[i] + poff) * (uint32_t)p.lda + (uint32_t)co) * 4u));
    } else {
      const uint32_t kb = (uint32_t)k * 4u;
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[i] = *reinterpret_cast<const float4*>(Ab + (a_row[i] + kb));
      if (p.scale) {
        rsc = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.scale) + kb);
        rsh = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.shift) + kb);
      }
    }
#pragma unroll
    for (int i = 0; i < NB4; ++i) {
      const int idx = t + 256 * i;
      if (DG) {
        const int kk = idx / (BN / 4);
        rb[i] = *reinterpret_cast<const float4*>(Bb + (b_off[i] + (uint32_t)min(k0 + kk, p.K - 1) * ldb * 4u));
      } else {
        const int kq = (idx % KQ) * 4;
        rb[i] = *reinterpret_cast<const float4*>(Bb + (b_off[i] + (uint32_t)min(k0 + kq, p.K - 4) * 4u));
      }
    }
  };

  const float act_lo = p.act == DL3P_ACT_NONE ? -DL3P_INF : 0.f;
  const float act_hi = (p.act == DL3P_ACT_NONE || p.act == DL3P_ACT_RELU) ? DL3P_INF : 6.f;
  auto prologue4 = [&](float4 v) {
    v = fma4(v, rsc, rsh);
    if (p.act >= DL3P_ACT_HSWISH) return act_apply4(v, p.act);
    return make_float4(__builtin_amdgcn_fmed3f(v.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.y, act_lo, act_hi),
                       __builtin_amdgcn_fmed3f(v.z, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.w, act_lo, act_hi));
  };
  const bool has_pro = !DG && (p.scale != nullptr || p.act != DL3P_ACT_NONE);
  const bool n_edge = n0 + BN > p.N;
  auto stage = [&](int it) {
    const int kt = it % nk;
    const int mt = blockIdx.x + (it / nk) * gridDim.x;
    const int m0 = mt * BM;
    const int k0 = kt * BKT;
    const bool a_edge = m0 + BM > p.M || k0 + BKT > p.K;
    const bool b_edge = n_edge || k0 + BKT > p.K;
    const bool kok = k0 + akq < p.K;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int r = ar + RP * i;
      float4 v = ra[i];
      if (has_pro) v = prologue4(v);
      if (a_edge) v = (kok && m0 + r < p.M) ? v : zero4();     // zero rows / columns stay exactly zero
      *reinterpret_cast<float4*>(&As[r * AP + akq]) = v;
    }
#pragma unroll
    for (int i = 0; i < NB4; ++i) {
      const int idx = t + 256 * i;
      float4 v = rb[i];
      if (DG) {
        const int kk = idx / (BN / 4), nq = idx - kk * (BN / 4);
        if (b_edge) v = (b_nok[i] && k0 + kk < p.K) ? v : zero4();
        *reinterpret_cast<float4*>(&Bs[kk * BPITCH + nq * 4]) = v;
      } else {
        const int r = idx / KQ, kq = (idx % KQ) * 4;
        if (b_edge) v = (b_nok[i] && k0 + kq < p.K) ? v : zero4();
        *reinterpret_cast<float4*>(&Bs[r * AP + kq]) = v;
      }
    }
  };

  f32x4 acc[MI][NT];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (it_total > 0) prefetch(0);
  for (int it = 0; it < it_total; ++it) {
    stage(it);
    __syncthreads();
    if (it + 1 < it_total) prefetch(it + 1);
#pragma unroll
    for (int g = 0; g < BKT / 16; ++g) {
      const int kc = g * 16 + q * 4;      // lane quarter q supplies k = kc + j at step j, for both operands
      float4 a[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        a[mi] = *reinterpret_cast<const float4*>(&As[(w * RW + mi * 16 + l15) * AP + kc]);
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        float b[4];
        if (DG) {
#pragma unroll
          for (int j = 0; j < 4; ++j) b[j] = Bs[(kc + j) * BPITCH + ni * 16 + l15];
        } else {
          const float4 bv = *reinterpret_cast<const float4*>(&Bs[(ni * 16 + l15) * AP + kc]);
          b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[0], a[mi].x, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[1], a[mi].y, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[2], a[mi].z, acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[3], a[mi].w, acc[mi][ni], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    if (it % nk == nk - 1) {
      // Epilogue of this M tile.  A lane holds 4 consecutive channels of row l15 per accumulator; the tile is transposed
      // through a wave-private LDS slice so that one store instruction covers 4 rows x 256 B.  Forward: each row is one input
      // pixel and the lane's 4 columns lie in ONE quadrant, so the store goes to output pixel (n, 2y + dy, 2x + dx) and stays
      // 16 bytes; with Cout a multiple of 64 (or 64 a multiple of Cout) the 16 lanes of a row still write whole contiguous
      // segments of one output pixel.
      const int mt = blockIdx.x + (it / nk) * gridDim.x;
      const int m0 = mt * BM;
      float* es = Es + w * RW * EPITCH;
      const int rr = l >> 4, cq = l & 15;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const f32x4 v = acc[mi][ni];
          acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<float4*>(&es[(mi * 16 + l15) * EPITCH + ni * 16 + q * 4]) = make_float4(v[0], v[1], v[2], v[3]);
        }
      const int n = n0 + cq * 4;
      const int row_lim = p.M - (m0 + w * RW);     // valid rows of this wave's slice (wave-uniform)
      if (n < p.N) {
        int co = n, tap = 0;
        if (!DG) tap = quadrant(n, p.Cout, &co);
        float4 bias4 = zero4();
        if (!DG && p.bias) bias4 = ld4(p.bias + co);
        char* yb = reinterpret_cast<char*>(p.Y);
        auto rows = [&](auto full) {
#pragma unroll
          for (int r0 = 0; r0 < RW; r0 += 4) {
            const int row = r0 + rr;
            if (decltype(full)::value || row < row_lim) {
              const uint32_t m = (uint32_t)(m0 + w * RW + row);
              const uint32_t orow = DG ? m : out_pixel(m, (uint32_t)p.W, tap);
              float* yp = reinterpret_cast<float*>(yb + (orow * (uint32_t)p.ldy + (uint32_t)co) * 4u);
              float4 o = add4(*reinterpret_cast<const float4*>(&es[row * EPITCH + cq * 4]), bias4);
              if (DG && p.accumulate) o = add4(o, ld4(yp));
              st4(yp, o);
            }
          }
        };
        if (row_lim >= RW) rows(std::true_type{});
        else rows(std::false_type{});
      }
    }
  }
}

// ------------------------------------------------------------------------------ weight gradient
// One workgroup = one 64 (n = (q, co)) x 64 (ci) tile of GW over one slice of M; slices are summed by dl3p_reduce_rows in slice
// order (deterministic).  Both operands are staged in [m][channel] layout (pitch 68: rows 4 apart land 16 banks apart) and read as
// ds_read_b32 fragments; the dY rows are GATHERED from the four output pixels of each input row while they are staged, the
// prologue goes on x.  The MFMA operands are ordered so that a lane ends with 4 consecutive ci of one n: GW is [4 Cout][Cin].
struct DeconvWgradParams {
  const float* X; int ldx; const float* scale; const float* shift; int act;
  const float* DY; int lddy;
  float* slabs;
  int M, K, N;               // K = Cin, N = 4 Cout
  int W, Cout;
  int ktiles, ntiles, mchunk;
};
constexpr int WT = 64, WPITCH = WT + 4, WQ = WT / 4, WNL = (32 * WQ) / 256;

__global__ __launch_bounds__(256, 2) void deconv_wgrad_kernel(DeconvWgradParams p) {
  __shared__ __attribute__((aligned(16))) float Xs[32 * WPITCH];
  __shared__ __attribute__((aligned(16))) float Ds[32 * WPITCH];
  const int t = threadIdx.x, l = t & 63, w = t >> 6, l15 = l & 15, q = l >> 4;
  const int tile = blockIdx.x;
  const int kt = tile / p.ntiles, nt = tile - kt * p.ntiles;
  const int k0 = kt * WT, n0 = nt * WT;
  const int m_begin = blockIdx.y * p.mchunk;
  const int m_end = min(p.M, m_begin + p.mchunk);
  int sr[WNL];                       // staged row of this thread's float4 (the same for both operands)
  uint32_t xo[WNL], dco[WNL], dpo[WNL];
  bool xok[WNL], dok[WNL];
  float4 xsc[WNL], xsh[WNL];
#pragma unroll
  for (int i = 0; i < WNL; ++i) {
    const int idx = t + 256 * i;
    sr[i] = idx / WQ;
    const int c4 = (idx - sr[i] * WQ) * 4;
    const int c = min(k0 + c4, p.K - 4);
    xok[i] = k0 + c4 < p.K;
    xo[i] = (uint32_t)c * 4u;
    xsc[i] = make_float4(1.f, 1.f, 1.f, 1.f); xsh[i] = zero4();
    if (p.scale) { xsc[i] = ld4(p.scale + c); xsh[i] = ld4(p.shift + c); }
    // this thread's dY columns never change: tap offset and channel, once
    const int n = min(n0 + c4, p.N - 4);
    int co;
    const int tap = quadrant(n, p.Cout, &co);
    dok[i] = n0 + c4 < p.N;
    dco[i] = (uint32_t)co;
    dpo[i] = (uint32_t)(tap >> 1) * 2u * (uint32_t)p.W + (uint32_t)(tap & 1);
  }
  const float act_lo = p.act == DL3P_ACT_NONE ? -DL3P_INF : 0.f;
  const float act_hi = (p.act == DL3P_ACT_NONE || p.act == DL3P_ACT_RELU) ? DL3P_INF : 6.f;
  const char* Xb = reinterpret_cast<const char*>(p.X);
  const char* Db = reinterpret_cast<const char*>(p.DY);
  float4 rx[WNL], rd[WNL];
  // unconditional loads on clamped rows; rows past the slice are zeroed by the select below
  auto prefetch = [&](int m0) {
#pragma unroll
    for (int i = 0; i < WNL; ++i) {
      const uint32_t m = (uint32_t)min(m0 + sr[i], m_end - 1);
      rx[i] = *reinterpret_cast<const float4*>(Xb + (m * (uint32_t)p.ldx * 4u + xo[i]));
      const uint32_t pix = out_pixel(m, (uint32_t)p.W, 0) + dpo[i];
      rd[i] = *reinterpret_cast<const float4*>(Db + ((pix * (uint32_t)p.lddy + dco[i]) * 4u));
    }
  };
  f32x4 acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (m_begin < m_end) prefetch(m_begin);
  for (int m0 = m_begin; m0 < m_end; m0 += 32) {
#pragma unroll
    for (int i = 0; i < WNL; ++i) {
      const int col = (t + 256 * i - sr[i] * WQ) * 4;
      const bool rok = m0 + sr[i] < m_end;
      float4 v = fma4(rx[i], xsc[i], xsh[i]);
      if (p.act >= DL3P_ACT_HSWISH) v = act_apply4(v, p.act);
      else v = make_float4(__builtin_amdgcn_fmed3f(v.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.y, act_lo, act_hi),
                           __builtin_amdgcn_fmed3f(v.z, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.w, act_lo, act_hi));
      *reinterpret_cast<float4*>(&Xs[sr[i] * WPITCH + col]) = (xok[i] && rok) ? v : zero4();
      *reinterpret_cast<float4*>(&Ds[sr[i] * WPITCH + col]) = (dok[i] && rok) ? rd[i] : zero4();
    }
    __syncthreads();
    if (m0 + 32 < m_end) prefetch(m0 + 32);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = Xs[(g * 16 + q * 4 + j) * WPITCH + w * 16 + l15];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = Ds[(g * 16 + q * 4 + j) * WPITCH + ni * 16 + l15];
#pragma unroll
        for (int j = 0; j < 4; ++j)   // D[ci][n]: lane ends with 4 consecutive ci for n = l15; four independent accumulators
          acc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[ni], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  float* slab = p.slabs + (size_t)blockIdx.y * p.K * p.N;
  const int k = k0 + w * 16 + q * 4;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + ni * 16 + l15;
    if (k < p.K && n < p.N) st4(slab + (size_t)n * p.K + k, make_float4(acc[ni][0], acc[ni][1], acc[ni][2], acc[ni][3]));
  }
}

// column sums of dY over all output pixels (bias gradient): one partial row per workgroup
__global__ __launch_bounds__(256) void deconv_colsum_kernel(const float* dy, int lddy, long long rows, int C, int c4s, int px, int nbx,
                                                            float* partials) {
  const int b = blockIdx.x;
  const int slab = b / nbx;
  const int bx = b - slab * nbx;
  const int pl = threadIdx.x / c4s;
  const int cl = threadIdx.x - pl * c4s;
  const bool active = pl < px;
  const int cbase4 = slab * c4s;
  const int c = (cbase4 + cl) * 4;
  float4 acc[1] = {zero4()};
  if (active)
    for (long long m = (long long)bx * px + pl; m < rows; m += (long long)nbx * px) acc[0] = add4(acc[0], ld4(dy + (size_t)m * lddy + c));
  block_reduce_store<1>(acc, active, pl, cl, c4s, px, cbase4, C, partials + (size_t)bx * C);
}

int g_max_workgroups = 0;     // dl3p_deconv2x2_set_plan

int check_view(const char* fn, const char* what, const void* ptr, int ld, int cols) {
  DL3P_CHECK_ARG(ptr != nullptr, "%s: %s is a null pointer", fn, what);
  DL3P_CHECK_ARG(ld % 4 == 0 && ld >= cols && aligned16(ptr), "%s: bad layout of %s (ld=%d, %d channels)", fn, what, ld, cols);
  return DL3P_OK;
}

// shape, and the offset guard of the kernels' 32-bit byte offsets: both activations below 4 GiB
int check_geometry(const char* fn, int N, int H, int W, int Cin, int Cout, int ld_in, int ld_out) {
  DL3P_CHECK_ARG(dl3p_deconv2x2_supported(Cin, Cout), "%s: Cin=%d and Cout=%d must be positive multiples of 4", fn, Cin, Cout);
  DL3P_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: bad geometry (N=%d H=%d W=%d)", fn, N, H, W);
  const unsigned long long M = (unsigned long long)N * (unsigned long long)H * (unsigned long long)W;
  const unsigned long long lim = 1ull << 32;
  DL3P_CHECK_ARG(M < lim && ld_in > 0 && ld_out > 0 && M * (unsigned long long)ld_in * 4ull < lim &&
                     4ull * M * (unsigned long long)ld_out * 4ull < lim && 16ull * Cin * Cout < lim,
                 "%s: operands of 4 GiB or more are not supported (N=%d H=%d W=%d)", fn, N, H, W);
  return DL3P_OK;
}

void gemm_grid(int M, int N, int* gx, int* gy, int* num_m_tiles) {
  const int nb = ceil_div(N, BN);
  const int mt = ceil_div(M, BM);
  int gx_max = (DL3P_NUM_CUS * 2) / nb;           // two resident workgroups per CU (62 KB of LDS each)
  if (gx_max < 8) gx_max = 8;
  if (g_max_workgroups > 0) gx_max = g_max_workgroups;
  int g = mt;
  if (mt > gx_max) g = ceil_div(mt, ceil_div(mt, gx_max));
  *gx = g; *gy = nb; *num_m_tiles = mt;
}

void wgrad_split(int M, int K, int N, int* ktiles, int* ntiles, int* splits, int* mchunk) {
  *ktiles = ceil_div(K, WT);
  *ntiles = ceil_div(N, WT);
  int s = (DL3P_NUM_CUS * 4) / (*ktiles * *ntiles);
  if (s < 1) s = 1;
  const int max_s = ceil_div(M, 256);          // at least 256 rows per slice
  if (s > max_s) s = max_s;
  if (s > DL3P_MAX_STAT_ROWS) s = DL3P_MAX_STAT_ROWS;
  const int chunk = ceil_div(ceil_div(M, s), 32) * 32;
  *splits = ceil_div(M, chunk);
  *mchunk = chunk;
}

}  // namespace

extern "C" int dl3p_deconv2x2_supported(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 4 == 0 && Cout % 4 == 0; }

extern "C" int dl3p_deconv2x2_set_plan(int max_workgroups) {
  DL3P_CHECK_ARG(max_workgroups >= 0, "dl3p_deconv2x2_set_plan: max_workgroups must be >= 0");
  g_max_workgroups = max_workgroups;
  return DL3P_OK;
}

extern "C" int dl3p_deconv2x2_fwd(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act, const float* w,
                                  const float* bias, float* y, int ldy, int N, int H, int W, int Cin, int Cout, void* stream) {
  const char* fn = "dl3p_deconv2x2_fwd";
  int rc = check_geometry(fn, N, H, W, Cin, Cout, ldx, ldy);
  if (rc) return rc;
  if ((rc = check_view(fn, "x", x, ldx, Cin))) return rc;
  if ((rc = check_view(fn, "y", y, ldy, Cout))) return rc;
  DL3P_CHECK_ARG(w && aligned16(w) && (!bias || aligned16(bias)), "%s: bad kernel / bias pointer", fn);
  DL3P_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr) && in_act >= DL3P_ACT_NONE && in_act <= DL3P_ACT_HSIGMOID,
                 "%s: bad prologue", fn);
  DeconvParams p = {};
  p.A = x; p.lda = ldx; p.scale = in_scale; p.shift = in_shift; p.act = in_act;
  p.B = w; p.bias = bias; p.Y = y; p.ldy = ldy;
  p.M = N * H * W; p.K = Cin; p.N = 4 * Cout; p.W = W; p.Cout = Cout;
  int gx, gy;
  gemm_grid(p.M, p.N, &gx, &gy, &p.num_m_tiles);
  dl3p_launch(deconv_gemm_kernel<false>, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_deconv2x2_bwd_data(const float* dy, int lddy, const float* w, float* gx, int ldgx, int accumulate, int N, int H,
                                       int W, int Cin, int Cout, void* stream) {
  const char* fn = "dl3p_deconv2x2_bwd_data";
  int rc = check_geometry(fn, N, H, W, Cin, Cout, ldgx, lddy);
  if (rc) return rc;
  if ((rc = check_view(fn, "dy", dy, lddy, Cout))) return rc;
  if ((rc = check_view(fn, "gx", gx, ldgx, Cin))) return rc;
  DL3P_CHECK_ARG(w && aligned16(w), "%s: bad kernel pointer", fn);
  DeconvParams p = {};
  p.A = dy; p.lda = lddy; p.act = DL3P_ACT_NONE;
  p.B = w; p.Y = gx; p.ldy = ldgx; p.accumulate = accumulate;
  p.M = N * H * W; p.K = 4 * Cout; p.N = Cin; p.W = W; p.Cout = Cout;
  int gxs, gys;
  gemm_grid(p.M, p.N, &gxs, &gys, &p.num_m_tiles);
  dl3p_launch(deconv_gemm_kernel<true>, dim3(gxs, gys), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" size_t dl3p_deconv2x2_bwd_weight_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || !dl3p_deconv2x2_supported(Cin, Cout)) return 0;
  const unsigned long long M = (unsigned long long)N * (unsigned long long)H * (unsigned long long)W;
  if (M >= (1ull << 31)) return 0;
  int kt, nt, s, mc;
  wgrad_split((int)M, Cin, 4 * Cout, &kt, &nt, &s, &mc);
  const size_t a = (size_t)s * Cin * 4 * Cout;
  const size_t b = (size_t)512 * Cout;      // bias column-sum partial rows
  return (a > b ? a : b) * sizeof(float);
}

extern "C" int dl3p_deconv2x2_bwd_weight(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                         const float* dy, int lddy, float* gw, float* gb, float* workspace, size_t workspace_bytes,
                                         int N, int H, int W, int Cin, int Cout, void* stream) {
  const char* fn = "dl3p_deconv2x2_bwd_weight";
  int rc = check_geometry(fn, N, H, W, Cin, Cout, ldx, lddy);
  if (rc) return rc;
  if ((rc = check_view(fn, "x", x, ldx, Cin))) return rc;
  if ((rc = check_view(fn, "dy", dy, lddy, Cout))) return rc;
  DL3P_CHECK_ARG(gw && aligned16(gw) && (!gb || aligned16(gb)) && workspace && aligned16(workspace), "%s: bad arguments", fn);
  DL3P_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr) && in_act >= DL3P_ACT_NONE && in_act <= DL3P_ACT_HSIGMOID,
                 "%s: bad prologue", fn);
  const size_t need = dl3p_deconv2x2_bwd_weight_workspace(N, H, W, Cin, Cout);
  if (workspace_bytes < need) {
    dl3p_set_error("%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    return DL3P_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  DeconvWgradParams p = {};
  p.X = x; p.ldx = ldx; p.scale = in_scale; p.shift = in_shift; p.act = in_act;
  p.DY = dy; p.lddy = lddy; p.slabs = workspace;
  p.M = N * H * W; p.K = Cin; p.N = 4 * Cout; p.W = W; p.Cout = Cout;
  int splits;
  wgrad_split(p.M, p.K, p.N, &p.ktiles, &p.ntiles, &splits, &p.mchunk);
  dl3p_launch(deconv_wgrad_kernel, dim3(p.ktiles * p.ntiles, splits), dim3(256), 0, st, p);
  DL3P_CHECK_LAUNCH(fn);
  rc = dl3p_reduce_rows_impl(workspace, splits, (size_t)p.K * p.N, gw, 0, st);
  if (rc) return rc;
  if (gb) {
    int c4s, px, nslab;
    pick_lanes(Cout, &c4s, &px, &nslab);
    const long long rows = 4ll * p.M;
    const long long need_b = ceil_div_ll(rows, px);
    const int nbx = (int)(need_b < 512 ? need_b : 512);
    hipLaunchKernelGGL(deconv_colsum_kernel, dim3(nbx * nslab), dim3(256), 0, st, dy, lddy, rows, Cout, c4s, px, nbx, workspace);
    DL3P_CHECK_LAUNCH("dl3p_deconv2x2_bwd_weight(colsum)");
    rc = dl3p_reduce_rows_impl(workspace, nbx, (size_t)Cout, gb, 0, st);
  }
  return rc;
}
