// The fp32 MFMA kernels of the pointwise / implicit GEMM (forward and data gradient): the tiled kernel and the streaming
// small-K.N kernel.  Included and instantiated by pwconv.hip only.
#pragma once
#include "pw_gemm.h"
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// B_KN: B is [Kred][Nout] row-major (forward: the Keras kernel as stored);
// !B_KN: B is [Nout][Kred] row-major (dgrad: the same kernel read as its transpose).
#ifndef DL3P_GEMM_PIN_B
#define DL3P_GEMM_PIN_B 1      // 0 builds the unpinned loop for A/B runs (scripts/micro/build_variant.sh)
#endif
template <int NT, bool B_KN, bool STATS, int MI, int BKT, bool BNB = false, bool GA = false>
__global__ __launch_bounds__(256, 2) void pw_gemm_kernel(GemmParams p_in) {
  GemmParams p = p_in;
  int block_y = blockIdx.y;
#ifndef DL3P_NO_SPLITK
  if constexpr (!B_KN && !STATS && !BNB && !GA) {
    if (p.ksplit > 1) {                     // split-K forward: this workgroup's slice of the reduction and its slab of the output
      const int nbn = (int)gridDim.y / p.ksplit;
      const int z = block_y / nbn;
      block_y -= z * nbn;
      const int k_lo = z * p.kchunk;
      p.A += k_lo;
      if (p.scale) { p.scale += k_lo; p.shift += k_lo; }
      p.B += k_lo;
      p.K = min(p.kchunk, p.K - k_lo);
      p.Y += (size_t)z * p.M * p.ldy;
      p.bias = nullptr;
    }
  }
#endif
  constexpr int AP = BKT + 4;   // A pitch: rows 4 apart land 16 banks apart -> ds_read_b128 conflict-free
  constexpr int KQ = BKT / 4;   // float4 per K-tile row
  constexpr int RP = 256 / KQ;  // A rows staged per pass of the 256 threads
  constexpr int NA = (64 * MI) / RP;
  constexpr int BM = 64 * MI;   // 4 waves x MI tiles of 16 rows
  constexpr int BN = 16 * NT;
  constexpr int BPITCH = B_KN ? (BN + 4) : AP;
  constexpr int BS_FLOATS = B_KN ? BKT * BPITCH : BN * AP;
  constexpr int NB4 = (KQ * BN + 255) / 256;  // float4 per thread for the B tile
  // epilogue transpose buffer (wave-private slices): accumulators go out as whole 256-B row segments
  constexpr int TPP = NT < 4 ? NT : 4;            // 16-column tiles per epilogue pass
  constexpr int NPASS = (NT + TPP - 1) / TPP;
  constexpr int CH = 16 * TPP;
  constexpr int EPITCH = CH + 4;
  constexpr int RW = 16 * MI;                      // rows per wave
  // one dynamic LDS object.  BKT = 64: the epilogue buffer overlays the operand tiles (one extra barrier per
  // M tile) so that two workgroups still fit a CU
  constexpr int AS_FLOATS = BM * AP;
  constexpr int ES_FLOATS = 4 * RW * EPITCH;
  constexpr int OPER_FLOATS = AS_FLOATS + BS_FLOATS;
  constexpr bool OVERLAY = BKT > 32;
  constexpr int RED_OFF = OVERLAY ? (OPER_FLOATS > ES_FLOATS ? OPER_FLOATS : ES_FLOATS) : OPER_FLOATS + ES_FLOATS;
  extern __shared__ __attribute__((aligned(16))) float g_lds[];
  float* As = g_lds;
  float* Bs = g_lds + AS_FLOATS;
  float* Es = OVERLAY ? g_lds : g_lds + OPER_FLOATS;
  float* red = g_lds + RED_OFF;

  const int t = threadIdx.x;
  const int l = t & 63;
  const int w = t >> 6;
  const int l15 = l & 15;
  const int q = l >> 4;
  const int n0 = block_y * BN;
  const int nk = (p.K + BKT - 1) / BKT;
  const int my_tiles = (p.num_m_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int it_total = my_tiles * nk;

  // staging roles.  Every global load of the K loop is UNCONDITIONAL on a clamped 32-bit byte offset
  // (rows >= M re-read row M-1, columns >= K re-read the last float4) and invalid lanes are zeroed by a
  // select when the tile is written to LDS: no exec-masked branch per load (13 of them per K-step
  // before), one v_add per address.  Hosts reject operands of 4 GiB or more.
  const int ar = t / KQ;         // A row within a pass of RP rows
  const int akq = (t % KQ) * 4;  // A k offset within the K tile
  const char* Ab = reinterpret_cast<const char*>(p.A);
  const char* Bb = reinterpret_cast<const char*>(p.B);

  float4 ra[NA];
  float4 rb[NB4];
  float4 rsc = make_float4(1.f, 1.f, 1.f, 1.f), rsh = zero4();
  uint32_t a_row[NA];        // byte offset of this thread's A rows in the current M tile
  int g_by[GA ? NA : 1], g_bx[GA ? NA : 1];   // GA: source coordinates of tap (0, 0) of this thread's rows
  uint32_t g_ok = 0;                          // GA: which of the NA loads in flight hit the source tensor
  uint32_t b_off[NB4];           // byte offset of this thread's B float4s at k0 = 0
  bool b_nok[NB4];               // column (B_KN) / row (!B_KN) of the B tile inside the matrix
  int pf_m0 = -1;
#pragma unroll
  for (int i = 0; i < NB4; ++i) {
    const int idx = min(t + 256 * i, KQ * BN - 1);
    if (B_KN) {
      const int kk = idx / (BN / 4), nq = idx - kk * (BN / 4);
      const int n = n0 + nq * 4;
      b_nok[i] = (t + 256 * i < KQ * BN) && n < p.N;
      b_off[i] = (uint32_t)(min(n, p.N - 4)) * 4u;    // + k * ldb * 4 per K-step
    } else {
      const int r = idx / KQ;
      const int n = n0 + r;
      b_nok[i] = (t + 256 * i < KQ * BN) && n < p.N;
      b_off[i] = (uint32_t)min(n, p.N - 1) * (uint32_t)p.ldb * 4u;   // + k * 4 per K-step
    }
  }

  auto prefetch = [&](int it) {
    const int kt = it % nk;
    const int mt = blockIdx.x + (it / nk) * gridDim.x;
    const int m0 = mt * BM;
    const int k0 = kt * BKT;
    if (GA) {
      if (m0 != pf_m0) {
        pf_m0 = m0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
          const int m = m0 + ar + RP * i;
          const int mc = min(m, p.M - 1);
          const int row = mc / p.g_RW, x = mc - row * p.g_RW;
          const int n = row / p.g_RH, y = row - n * p.g_RH;
          // rows past M get a base far outside the source: every tap fails the bounds check
          g_by[i] = m < p.M ? y * p.g_mul + p.g_ay : -(1 << 20);
          g_bx[i] = x * p.g_mul + p.g_ax;
          a_row[i] = (uint32_t)n * (uint32_t)(p.g_SH * p.g_SW);      // pixel index of the image in the source
        }
      }
      const int k = min(k0 + akq, p.K - 4);
      const int tap = (int)__umulhi((uint32_t)k, p.g_cmagic);
      const int c = k - tap * p.g_C;
      const int ky = (tap * p.g_kwmagic) >> 16, kx = tap - ky * p.g_kw;
      const int dyo = ky * p.g_d, dxo = kx * p.g_d;
      const int par = (1 << p.g_shift) - 1;
      g_ok = 0;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int ty = g_by[i] + dyo, tx = g_bx[i] + dxo;
        const int sy = ty >> p.g_shift, sx = tx >> p.g_shift;
        const bool ok = ty >= 0 && tx >= 0 && ((ty | tx) & par) == 0 && sy < p.g_SH && sx < p.g_SW && k0 + akq < p.K;
        const uint32_t off = ok ? ((a_row[i] + (uint32_t)(sy * p.g_SW + sx)) * (uint32_t)p.lda + (uint32_t)c) * 4u : 0u;
        ra[i] = *reinterpret_cast<const float4*>(Ab + off);
        g_ok |= ok ? (1u << i) : 0u;
      }
      if (p.scale) {
        rsc = *reinterpret_cast<const float4*>(p.scale + c);
        rsh = *reinterpret_cast<const float4*>(p.shift + c);
      }
    } else {
    if (m0 != pf_m0) {
      pf_m0 = m0;
#pragma unroll
      for (int i = 0; i < NA; ++i) a_row[i] = (uint32_t)min(m0 + ar + RP * i, p.M - 1) * (uint32_t)p.lda * 4u;
    }
    const uint32_t kb = (uint32_t)min(k0 + akq, p.K - 4) * 4u;
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = *reinterpret_cast<const float4*>(Ab + (a_row[i] + kb));
    if (p.scale) {
      rsc = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.scale) + kb);
      rsh = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.shift) + kb);
    }
    }
#pragma unroll
    for (int i = 0; i < NB4; ++i) {
      const int idx = min(t + 256 * i, KQ * BN - 1);
      if (B_KN) {
        const int kk = idx / (BN / 4);
        rb[i] = *reinterpret_cast<const float4*>(Bb + (b_off[i] + (uint32_t)min(k0 + kk, p.K - 1) * (uint32_t)p.ldb * 4u));
      } else {
        const int kq = (idx % KQ) * 4;
        rb[i] = *reinterpret_cast<const float4*>(Bb + (b_off[i] + (uint32_t)min(k0 + kq, p.K - 4) * 4u));
      }
    }
  };

  // producer's BatchNormalization + activation on the way into LDS.  relu / relu6 / none are one
  // fma + one v_med3 per element; the hard-swish family takes the general form (wave-uniform branch).
  const float act_lo = p.act == DL3P_ACT_NONE ? -DL3P_INF : 0.f;
  const float act_hi = (p.act == DL3P_ACT_NONE || p.act == DL3P_ACT_RELU) ? DL3P_INF : 6.f;
  auto prologue4 = [&](float4 v) {
    v = fma4(v, rsc, rsh);
    if (p.act >= DL3P_ACT_HSWISH) return act_apply4(v, p.act);
    return make_float4(__builtin_amdgcn_fmed3f(v.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.y, act_lo, act_hi),
                       __builtin_amdgcn_fmed3f(v.z, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.w, act_lo, act_hi));
  };

  const bool has_pro = p.scale != nullptr || p.act != DL3P_ACT_NONE;   // data gradient / im2col input: raw operand
  const bool n_edge = n0 + BN > p.N;
  auto stage = [&](int it) {
    const int kt = it % nk;
    const int mt = blockIdx.x + (it / nk) * gridDim.x;
    const int m0 = mt * BM;
    const int k0 = kt * BKT;
    // interior K-steps (the common case, wave-uniform) skip the zero-fill selects of the M / K / N tails
    const bool a_edge = m0 + BM > p.M || k0 + BKT > p.K;
    const bool b_edge = n_edge || k0 + BKT > p.K;
    const bool kok = k0 + akq < p.K;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int r = ar + RP * i;
      float4 v = ra[i];
      if (has_pro) v = prologue4(v);
      // zero rows/cols stay exactly zero (padding of the M and K tails; GA: taps outside the source)
      if (GA) v = ((g_ok >> i) & 1u) ? v : zero4();
      else if (a_edge) v = (kok && m0 + r < p.M) ? v : zero4();
      *reinterpret_cast<float4*>(&As[r * AP + akq]) = v;
    }
#pragma unroll
    for (int i = 0; i < NB4; ++i) {
      const int idx = t + 256 * i;
#if DL3P_GEMM_PIN_B
      // An empty asm that reads rb[i] right before its LDS store.  Without it clang hoists the B stores' address math
      // and, in 64 of the 80 instantiations, ends up with an s_waitcnt vmcnt(5)/(6) INSIDE the next K-step's prefetch
      // burst (right after the barrier): every wave then sits out a full memory latency before its first MFMA.  With
      // the pin none of the 80 has that wait; the decoder GEMMs run 4-12 % faster ("stage phase").
      asm volatile("" :: "v"(rb[i].x), "v"(rb[i].y), "v"(rb[i].z), "v"(rb[i].w));
#endif
      if (idx < KQ * BN) {
        if (B_KN) {
          const int kk = idx / (BN / 4), nq = idx - kk * (BN / 4);
          float4 v = make_float4(rb[i].x, rb[i].y, rb[i].z, rb[i].w);
          if (b_edge) v = (b_nok[i] && k0 + kk < p.K) ? v : zero4();
          *reinterpret_cast<float4*>(&Bs[kk * BPITCH + nq * 4]) = v;
        } else {
          const int r = idx / KQ, kq = (idx % KQ) * 4;
          float4 v = make_float4(rb[i].x, rb[i].y, rb[i].z, rb[i].w);
          if (b_edge) v = (b_nok[i] && k0 + kq < p.K) ? v : zero4();
          *reinterpret_cast<float4*>(&Bs[r * AP + kq]) = v;
        }
      }
    }
  };

  f32x4 acc[MI][NT];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 st_s[STATS ? NPASS : 1], st_q[STATS ? NPASS : 1];   // per lane: 4 columns of each epilogue pass
  if (STATS) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) { st_s[i] = zero4(); st_q[i] = zero4(); }
  }

  if (it_total > 0) prefetch(0);
  for (int it = 0; it < it_total; ++it) {
    stage(it);
    __syncthreads();
    if (it + 1 < it_total) prefetch(it + 1);
#pragma unroll
    for (int g = 0; g < BKT / 16; ++g) {
      const int kc = g * 16 + q * 4;
      float4 a[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        a[mi] = *reinterpret_cast<const float4*>(&As[(w * 16 * MI + mi * 16 + l15) * AP + kc]);
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        float b[4];
        if (B_KN) {
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
      // epilogue of this M tile.  After the MFMAs a lane holds 4 consecutive channels of pixel l15 per
      // accumulator; stored directly that is 16 rows x 64 B per store instruction (half cache lines,
      // measured: 13.6k cycles per tile, and the next tile's staging waits behind those stores).  The tile
      // is therefore transposed through a wave-private LDS slice and leaves as 4 rows x 256 B per
      // instruction; bias / accumulate / BN statistics are applied on the way out.
      const int mt = blockIdx.x + (it / nk) * gridDim.x;
      const int m0 = mt * BM;
      float* es = Es + w * RW * EPITCH;
      const int rr = l >> 4, cq = l & 15;
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int ni0 = ps * TPP;
#pragma unroll
        for (int nl = 0; nl < TPP; ++nl) {
          if (ni0 + nl < NT) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
              const f32x4 v = acc[mi][ni0 + nl];
              acc[mi][ni0 + nl] = (f32x4){0.f, 0.f, 0.f, 0.f};
              *reinterpret_cast<float4*>(&es[(mi * 16 + l15) * EPITCH + nl * 16 + q * 4]) = make_float4(v[0], v[1], v[2], v[3]);
            }
          }
        }
        const int n = n0 + ni0 * 16 + cq * 4;
        const bool col_ok = (ni0 * 16 + cq * 4 < BN) && (cq * 4 < CH) && n < p.N && (ni0 + cq / 4 < NT);
        const int row_lim = p.M - (m0 + w * RW);     // valid rows of this wave's slice (wave-uniform)
        if (col_ok) {
          float4 bias4 = zero4();
          if (p.bias) bias4 = ld4(p.bias + n);
          char* yb = reinterpret_cast<char*>(p.Y) + ((uint32_t)(m0 + w * RW + rr) * (uint32_t)p.ldy + (uint32_t)n) * 4u;
          const uint32_t ystep = (uint32_t)p.ldy * 16u;   // 4 rows
          // fused BN-backward statistics: per-channel constants of this lane's 4 columns
          constexpr bool bnb = STATS && BNB;    // (a template flag: the z prefetch registers must not burden the forward)
          float4 bsc = zero4(), bsh = zero4(), bmu = zero4(), bis = zero4();
          float4 zpre[RW / 4];          // all z rows of the pass are requested before the first one is used
          if (bnb) {
            bsc = ld4(p.bb_scale + n); bsh = ld4(p.bb_shift + n); bmu = ld4(p.bb_mean + n); bis = ld4(p.bb_invstd + n);
            const char* zbase = reinterpret_cast<const char*>(p.bb_z) + (uint32_t)n * 4u;
#pragma unroll
            for (int i = 0; i < RW / 4; ++i) {
              const int mrow = min(m0 + w * RW + 4 * i + rr, p.M - 1);       // rows past M re-read the last one (unused)
              zpre[i] = *reinterpret_cast<const float4*>(zbase + (uint32_t)mrow * (uint32_t)p.bb_ldz * 4u);
            }
          }
          auto rows = [&](auto full) {
#pragma unroll
            for (int r0 = 0; r0 < RW; r0 += 4) {
              const int row = r0 + rr;
              if (decltype(full)::value || row < row_lim) {
                float4 o = add4(*reinterpret_cast<const float4*>(&es[row * EPITCH + cq * 4]), bias4);
                float* yp = reinterpret_cast<float*>(yb + (r0 / 4) * ystep);
                if (p.accumulate) o = add4(o, ld4(yp));
                st4(yp, o);
                if (STATS) {
                  if (bnb) {
                    const float4 zv = zpre[r0 / 4];
                    const float4 u = fma4(zv, bsc, bsh);
                    const float4 d = make_float4(o.x * act_grad(u.x, p.bb_act), o.y * act_grad(u.y, p.bb_act),
                                                 o.z * act_grad(u.z, p.bb_act), o.w * act_grad(u.w, p.bb_act));
                    const float4 xh = make_float4((zv.x - bmu.x) * bis.x, (zv.y - bmu.y) * bis.y, (zv.z - bmu.z) * bis.z,
                                                  (zv.w - bmu.w) * bis.w);
                    st_s[ps] = add4(st_s[ps], d);
                    st_q[ps] = fma4(d, xh, st_q[ps]);
                  } else {
                    st_s[ps] = add4(st_s[ps], o);
                    st_q[ps] = fma4(o, o, st_q[ps]);
                  }
                }
              }
            }
          };
          if (row_lim >= RW) rows(std::true_type{});
          else rows(std::false_type{});
        }
      }
      if (OVERLAY) __syncthreads();   // the next stage() overwrites the epilogue buffer
    }
  }

  if (STATS) {
    // reduce over the 4 row groups of the wave, then over the 4 waves; one partial row per workgroup
    const int rr = l >> 4, cq = l & 15;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      float sv[4] = {st_s[ps].x, st_s[ps].y, st_s[ps].z, st_s[ps].w};
      float qv[4] = {st_q[ps].x, st_q[ps].y, st_q[ps].z, st_q[ps].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s1 = sv[e], s2 = qv[e];
        s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        const int col = ps * CH + cq * 4 + e;
        if (rr == 0 && cq * 4 < CH && col < BN) {
          red[(0 * 4 + w) * BN + col] = s1;
          red[(1 * 4 + w) * BN + col] = s2;
        }
      }
    }
    __syncthreads();
    if (p.partials) {
      for (int i = t; i < 2 * BN; i += 256) {
        const int which = i / BN, nn = i - which * BN;
        if (n0 + nn < p.N) {
          float s = red[(which * 4 + 0) * BN + nn] + red[(which * 4 + 1) * BN + nn] +
                    red[(which * 4 + 2) * BN + nn] + red[(which * 4 + 3) * BN + nn];
          p.partials[((size_t)blockIdx.x * 2 + which) * p.N + n0 + nn] = s;
        }
      }
    }
  }
}

// (A barrier-enforced ping-pong of two half-workgroups -- 512 threads, waves 0-3 multiply while waves 4-7 stage and
// vice versa -- was built and measured twice this round: 510 us and 624 us against 471 us for two free-running
// workgroups per CU on 266256x304x256.  One wave per SIMD cannot keep the matrix pipe issuing back to back through
// its own LDS-read latencies; the free-running pair fills those bubbles.  Removed.)

// ------------------------------------------------------------------------------ forward / dgrad, small K x N
// Same idea as pw_wgrad_small_kernel for Y = act(X*scale+shift) @ W when the whole kernel matrix is a few
// KB (the 129x129 / 257x257 layers): W sits in LDS for the life of the workgroup, every wave walks its own
// 16-row tiles of M with no workgroup barrier, A fragments come straight from global memory (lane
// (row l15, quarter q) loads the float4 X[row][16 kt + 4q ..]: the k-permutation of the big kernel makes
// that exactly its MFMA operand), the 16 x N result is transposed through a wave-private LDS slice and
// leaves as whole rows; BN statistics are kept per lane in that row-major form and reduced once at the end.
template <int KT, int NTN, bool STATS, bool BNB = false>
__global__ __launch_bounds__(256, 2) void pw_small_kernel(GemmParams p) {
  constexpr int KP = 16 * KT, NP = 16 * NTN;
  constexpr int BP = NP + 4, TP = NP + 4;
  extern __shared__ __attribute__((aligned(16))) float sm_lds[];
  float* Bs = sm_lds;                         // [KP][BP], zero padded
  float* sc_s = Bs + KP * BP;
  float* sh_s = sc_s + KP;
  float* bq_s = sh_s + KP;                    // BNB: [scale | shift | mean | invstd][NP] of the BatchNorm whose sums ride along
  float* Tall = bq_s + (BNB ? 4 * NP : 0);    // 4 wave slices of [16][TP]
  const int t = threadIdx.x, l = t & 63, w = t >> 6, l15 = l & 15, q = l >> 4;
  float* Ts = Tall + w * 16 * TP;
  if (p.b_kn) {
    for (int idx = t; idx < KP * NP; idx += 256) {
      const int k = idx / NP, n = idx - k * NP;
      Bs[k * BP + n] = (k < p.K && n < p.N) ? p.B[(size_t)k * p.ldb + n] : 0.f;
    }
  } else {
    for (int idx = t; idx < KP * NP; idx += 256) {
      const int n = idx / KP, k = idx - n * KP;
      Bs[k * BP + n] = (k < p.K && n < p.N) ? p.B[(size_t)n * p.ldb + k] : 0.f;
    }
  }
  for (int i = t; i < KP; i += 256) {
    sc_s[i] = (p.scale && i < p.K) ? p.scale[i] : 1.f;
    sh_s[i] = (p.scale && i < p.K) ? p.shift[i] : 0.f;
  }
  if (BNB) {
    for (int i = t; i < NP; i += 256) {
      const bool in = i < p.N;
      bq_s[i] = in ? p.bb_scale[i] : 1.f;
      bq_s[NP + i] = in ? p.bb_shift[i] : 0.f;
      bq_s[2 * NP + i] = in ? p.bb_mean[i] : 0.f;
      bq_s[3 * NP + i] = in ? p.bb_invstd[i] : 0.f;
    }
  }
  __syncthreads();

  // A fragment loads: clamped 32-bit byte offsets, invalid lanes zeroed by select
  uint32_t a_k[KT];
  bool a_kok[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    const int k = kt * 16 + 4 * q;
    a_kok[kt] = k < p.K;
    a_k[kt] = (uint32_t)min(k, p.K - 4) * 4u;
  }
  // row-major output mapping of a 16 x N tile: float4 f = l + 64 i  ->  (row f / (N/4), column group f % (N/4))
  const int n4 = p.N >> 2, nf = 4 * p.N;
  int yrow[NTN], yl[NTN];
  uint32_t yg[NTN], zg[BNB ? NTN : 1];
#pragma unroll
  for (int i = 0; i < NTN; ++i) {
    const int f = min(l + 64 * i, nf - 1);
    const int r = f / n4, c = f - r * n4;
    yrow[i] = (l + 64 * i < nf) ? r : (1 << 20);
    yl[i] = r * TP + c * 4;
    yg[i] = ((uint32_t)r * (uint32_t)p.ldy + (uint32_t)c * 4u) * 4u;
    if (BNB) zg[i] = ((uint32_t)r * (uint32_t)p.bb_ldz + (uint32_t)c * 4u) * 4u;
  }
  const char* Zb = reinterpret_cast<const char*>(p.bb_z);
  const float act_lo = p.act == DL3P_ACT_NONE ? -DL3P_INF : 0.f;
  const float act_hi = (p.act == DL3P_ACT_NONE || p.act == DL3P_ACT_RELU) ? DL3P_INF : 6.f;

  f32x4 acc[NTN];
#pragma unroll
  for (int b = 0; b < NTN; ++b) acc[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 st_s[STATS ? NTN : 1], st_q[STATS ? NTN : 1];
  if (STATS) {
#pragma unroll
    for (int i = 0; i < NTN; ++i) { st_s[i] = zero4(); st_q[i] = zero4(); }
  }

  const int ntiles = (p.M + 15) >> 4;
  const int nwaves = gridDim.x * 4;
  const int gw = blockIdx.x * 4 + w;
  const char* Ab = reinterpret_cast<const char*>(p.A);
  char* Yb = reinterpret_cast<char*>(p.Y);
  float4 ra[KT];
#define SM_PREFETCH(tile_)                                                                                   \
  {                                                                                                          \
    const uint32_t arow = (uint32_t)min(((tile_) << 4) + l15, p.M - 1) * (uint32_t)p.lda * 4u;              \
    _Pragma("unroll") for (int kt = 0; kt < KT; ++kt) ra[kt] = *reinterpret_cast<const float4*>(Ab + (arow + a_k[kt])); \
  }
  SM_PREFETCH(min(gw, ntiles - 1))
  for (int tile = gw; tile < ntiles; tile += nwaves) {
    const int m0 = tile << 4;
    const bool row_ok = m0 + l15 < p.M;
    // BNB: the z rows this lane's outputs meet are requested now and used after the MFMAs
    float4 zpre[BNB ? NTN : 1];
    if (BNB) {
      const uint32_t zbase = (uint32_t)m0 * (uint32_t)p.bb_ldz * 4u;
#pragma unroll
      for (int i = 0; i < NTN; ++i) {
        const uint32_t off = (yrow[i] < p.M - m0) ? zg[i] : 0u;        // rows past M re-read the tile's first row (unused)
        zpre[i] = *reinterpret_cast<const float4*>(Zb + (zbase + off));
      }
    }
    float4 a[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const float4 s4 = *reinterpret_cast<const float4*>(&sc_s[kt * 16 + 4 * q]);
      const float4 h4 = *reinterpret_cast<const float4*>(&sh_s[kt * 16 + 4 * q]);
      float4 v = fma4(ra[kt], s4, h4);
      if (p.act >= DL3P_ACT_HSWISH) v = act_apply4(v, p.act);
      else v = make_float4(__builtin_amdgcn_fmed3f(v.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.y, act_lo, act_hi),
                           __builtin_amdgcn_fmed3f(v.z, act_lo, act_hi), __builtin_amdgcn_fmed3f(v.w, act_lo, act_hi));
      a[kt] = (row_ok && a_kok[kt]) ? v : zero4();
    }
    SM_PREFETCH(min(tile + nwaves, ntiles - 1))
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const float av[4] = {a[kt].x, a[kt].y, a[kt].z, a[kt].w};
#pragma unroll
      for (int nt = 0; nt < NTN; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Bs[(kt * 16 + 4 * q + j) * BP + nt * 16 + l15], av[j], acc[nt], 0, 0, 0);
    }
    // lane holds 4 consecutive channels (nt*16 + 4q ..) of pixel l15 -> wave-private transpose -> whole rows
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) {
      *reinterpret_cast<float4*>(&Ts[l15 * TP + nt * 16 + 4 * q]) = make_float4(acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
      acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const uint32_t ybase = (uint32_t)m0 * (uint32_t)p.ldy * 4u;
    const int rows_here = p.M - m0;
#pragma unroll
    for (int i = 0; i < NTN; ++i) {
      if (yrow[i] < rows_here) {
        float4 o = *reinterpret_cast<const float4*>(&Ts[yl[i]]);
        if (p.bias) o = add4(o, ld4(p.bias + (yl[i] - yrow[i] * TP)));
        float* yp = reinterpret_cast<float*>(Yb + (ybase + yg[i]));
        if (p.accumulate) o = add4(o, ld4(yp));
#ifdef DL3P_ABLATE_STORES
        if (o.x == 1234.5678f)
#endif
        st4(yp, o);
        if (STATS && BNB) {
          // (sum g', sum g' * xhat) of the BatchNorm behind this gradient, as dl3p_bn_bwd_reduce forms them
          const int cf = yl[i] - yrow[i] * TP;
          const float4 zv = zpre[i];
          const float4 u = fma4(zv, *reinterpret_cast<const float4*>(&bq_s[cf]), *reinterpret_cast<const float4*>(&bq_s[NP + cf]));
          const float4 mu = *reinterpret_cast<const float4*>(&bq_s[2 * NP + cf]), is = *reinterpret_cast<const float4*>(&bq_s[3 * NP + cf]);
          const float4 d = make_float4(o.x * act_grad(u.x, p.bb_act), o.y * act_grad(u.y, p.bb_act),
                                       o.z * act_grad(u.z, p.bb_act), o.w * act_grad(u.w, p.bb_act));
          const float4 xh = make_float4((zv.x - mu.x) * is.x, (zv.y - mu.y) * is.y, (zv.z - mu.z) * is.z, (zv.w - mu.w) * is.w);
          st_s[i] = add4(st_s[i], d);
          st_q[i] = fma4(d, xh, st_q[i]);
        } else if (STATS) {
          st_s[i] = add4(st_s[i], o);
          st_q[i] = fma4(o, o, st_q[i]);
        }
      }
    }
  }
#undef SM_PREFETCH
  if (STATS) {
    // per-lane sums are indexed by (row r, column group c) of the tile pattern: dump them and add the
    // 16 rows x 4 waves of every column group in a fixed order; one partial row per workgroup
    float4* S = reinterpret_cast<float4*>(Tall);
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NTN; ++i)
        if (l + 64 * i < nf) S[w * 4 * NP + l + 64 * i] = which ? st_q[i] : st_s[i];
      __syncthreads();
      if (p.partials && t < n4) {
        float4 s = zero4();
        for (int ww = 0; ww < 4; ++ww)
          for (int r = 0; r < 16; ++r) s = add4(s, S[ww * 4 * NP + r * n4 + t]);
        st4(p.partials + ((size_t)blockIdx.x * 2 + which) * p.N + 4 * t, s);
      }
    }
  }
}

template <int KT, int NTN, bool BNB = false>
static constexpr size_t pw_small_lds() {
  return sizeof(float) * (size_t)(16 * KT * (16 * NTN + 4) + 2 * 16 * KT + (BNB ? 4 * 16 * NTN : 0) + 4 * 16 * (16 * NTN + 4));
}
