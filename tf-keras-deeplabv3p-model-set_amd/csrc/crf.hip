// Fully connected CRF post-processing for gfx950: mean-field inference of the dense CRF of Kraehenbuehl & Koltun
// with the unary term of pydensecrf's unary_from_labels (a hard class mask, gt_prob), a Gaussian (position) and a bilateral
// (position + colour) Potts kernel, symmetric normalisation -- deeplabv3p/postprocess_np.py of the reference with zero_unsure=False.
// The reference filters with a permutohedral lattice on the CPU; here every message pass is the sum the lattice approximates,
//   out_i[l] = sum_j k(f_i, f_j) V_j[l]      over ALL pixels j of the image (j == i included),
// computed exactly in fp32:
//   * the Gaussian kernel is separable: a row pass and a column pass over the full width / height (VALU, 1-D tables in LDS);
//   * the bilateral kernel is attention without the softmax: each lane forms k(i, j) from exact integer-valued coordinate and colour
//     differences and one v_exp_f32; that value is the A operand of v_mfma_f32_32x32x2_f32, the V rows are the B operand, the
//     32 x 32 accumulator (32 pixels i x 32 label columns) stays in registers for the whole walk over j.
// Class vectors are rows of Lp = 32 floats (C <= 32): columns of absent classes and columns >= C hold exactly 0 and stay 0
// through every product (k * 0 = 0).  Batch is grid dimension y (z for the Gaussian); buffer offsets are 64-bit, pixel indices
// 32-bit.  Everything runs on the caller's stream, nothing synchronises.
#include "head_common.h"

#define CRF_LP 32              // label columns of a class-vector row = the MFMA's column count
#define CRF_TILE 128           // pixels i per workgroup of the bilateral kernel: 4 waves x 32 rows
#define CRF_CHUNK 256          // pixels j staged in LDS per step of the walk
#define CRF_MAX_SIDE 2048      // dx^2 + dy^2 and the colour distance stay exact integers in fp32 (< 2^24)

typedef float crf_f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------ census, unary term, update
// present classes of one image as a bit mask, found by every workgroup for itself (the mask is n int32 and stays in L2)
__device__ __forceinline__ unsigned int crf_census(const int32_t* mask, int n, int C, unsigned int* lds_bits) {
  if (threadIdx.x == 0) *lds_bits = 0u;
  __syncthreads();
  unsigned int bits = 0u;
  for (int t = threadIdx.x; t < n; t += 256) {
    const int m = mask[t];
    if (m >= 0 && m < C) bits |= 1u << m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off);
  if ((threadIdx.x & 63) == 0 && bits) atomicOr(lds_bits, bits);
  __syncthreads();
  return *lds_bits;
}

struct CrfUpdateParams {
  const int32_t* mask; int* census_out; const int* census;
  const float* fg; const float* ng; const float* fb; const float* nb;
  float wg, wb, log_own, one_minus_gt;
  float* q; int ldq; int32_t* mask_out;
  int n, C;
};

// 32 lanes per pixel, lane = class column:  Q = softmax over the present classes of  -U + wg ng_i Fg_i + wb nb_i Fb_i;
// absent classes and columns >= C get exactly 0.  mask_out: argmax, lowest class id on ties; an image with fewer than two
// present classes keeps its mask as it came.
template <bool CENSUS>
__global__ __launch_bounds__(256) void crf_update_kernel(CrfUpdateParams p) {
  __shared__ unsigned int lds_bits;
  const int img = blockIdx.y;
  const int32_t* mask = p.mask + (size_t)img * p.n;
  unsigned int bits;
  if (CENSUS) {
    bits = crf_census(mask, p.n, p.C, &lds_bits);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      p.census_out[img * 2] = (int)bits;
      p.census_out[img * 2 + 1] = __popc(bits);
    }
  } else {
    bits = (unsigned int)p.census[img * 2];
  }
  const int nl = __popc(bits);
  const int c = threadIdx.x & 31;
  const bool present = (bits >> c) & 1u;
  const float log_other = nl > 1 ? logf(p.one_minus_gt / (float)(nl - 1)) : 0.f;
  const size_t row0 = (size_t)img * p.n;
  for (int px = blockIdx.x * 8 + (threadIdx.x >> 5); px < p.n; px += gridDim.x * 8) {
    const int m = mask[px];
    const size_t row = row0 + px;
    float logit = c == m ? p.log_own : log_other;
    if (p.fg) logit = logit + (p.wg * p.ng[px]) * p.fg[row * CRF_LP + c];
    if (p.fb) logit = logit + (p.wb * p.nb[row]) * p.fb[row * CRF_LP + c];
    float mx = present ? logit : -DL3P_INF;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float e = present ? __expf(logit - mx) : 0.f;
    float sum = e;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const float q = present ? e / sum : 0.f;
    if (p.q) p.q[row * p.ldq + c] = q;
    if (p.mask_out) {
      float best = present ? q : -1.f;
      int arg = c;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
      }
      if (c == 0) p.mask_out[row] = nl > 1 ? arg : m;
    }
  }
}

static int crf_update_launch(const char* fn, bool census, CrfUpdateParams p, float gt_prob, int N, hipStream_t st) {
  DL3P_CHECK_ARG(N > 0 && p.n > 0, "%s: bad dims N=%d n=%d", fn, N, p.n);
  DL3P_CHECK_ARG(p.C >= 1 && p.C <= CRF_LP, "%s: C=%d is outside [1, %d]", fn, p.C, CRF_LP);
  DL3P_CHECK_ARG(gt_prob > 0.f && gt_prob < 1.f, "%s: gt_prob=%g is outside (0, 1)", fn, (double)gt_prob);
  DL3P_CHECK_ARG(p.mask && (p.q || p.mask_out), "%s: needs a mask and something to produce", fn);
  DL3P_CHECK_ARG(!p.q || p.ldq >= CRF_LP, "%s: Q rows hold %d columns (ldq=%d)", fn, CRF_LP, p.ldq);
  DL3P_CHECK_ARG((p.fg != nullptr) == (p.ng != nullptr) && (p.fb != nullptr) == (p.nb != nullptr),
                 "%s: a message comes with its normaliser", fn);
  p.log_own = logf(gt_prob);
  p.one_minus_gt = 1.f - gt_prob;
  // the census walks the whole mask in every workgroup: few workgroups per image then
  int blocks = ceil_div(p.n, 8);
  const int cap = census ? 64 : DL3P_NUM_CUS * 8;
  if (blocks > cap) blocks = cap;
  if (census) hipLaunchKernelGGL(crf_update_kernel<true>, dim3(blocks, N), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(crf_update_kernel<false>, dim3(blocks, N), dim3(256), 0, st, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_crf_unary(const int* mask, int32_t* census, float* q, int ldq, float gt_prob, int N, int n, int C,
                              void* stream) {
  const char* fn = "dl3p_crf_unary";
  DL3P_CHECK_ARG(census && q, "%s: needs the census and the Q buffer", fn);
  CrfUpdateParams p = {};
  p.mask = mask; p.census_out = census; p.q = q; p.ldq = ldq; p.n = n; p.C = C;
  return crf_update_launch(fn, true, p, gt_prob, N, (hipStream_t)stream);
}

extern "C" int dl3p_crf_update(const int* mask, const int* census, const float* fg, const float* norm_g, const float* fb,
                               const float* norm_b, float weight_g, float weight_b, float gt_prob, float* q, int ldq,
                               int32_t* mask_out, int N, int n, int C, void* stream) {
  const char* fn = "dl3p_crf_update";
  DL3P_CHECK_ARG(census, "%s: needs the census dl3p_crf_unary left", fn);
  CrfUpdateParams p = {};
  p.mask = mask; p.census = census; p.fg = fg; p.ng = norm_g; p.fb = fb; p.nb = norm_b; p.wg = weight_g; p.wb = weight_b;
  p.q = q; p.ldq = ldq; p.mask_out = mask_out; p.n = n; p.C = C;
  return crf_update_launch(fn, false, p, gt_prob, N, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------ Gaussian message (separable, exact)
// table[d] = exp(-d^2 / (2 s^2)) for the d in [0, L) of one axis
__device__ __forceinline__ void crf_axis_table(float* tab, int L, float inv2s2) {
  for (int d = threadIdx.x; d < L; d += 256) tab[d] = expf(-(float)(d * d) * inv2s2);
  __syncthreads();
}

// norm[p] = 1 / sqrt(sum_j k(p, j) + 1e-20) with the sum as the product of its two 1-D sums; the same for every image
__global__ __launch_bounds__(256) void crf_gauss_norm_kernel(float* norm, int H, int W, float inv2sx2, float inv2sy2) {
  extern __shared__ float crf_tab[];          // [W] then [H]
  float* tx = crf_tab;
  float* ty = crf_tab + W;
  for (int d = threadIdx.x; d < W; d += 256) tx[d] = expf(-(float)(d * d) * inv2sx2);
  for (int d = threadIdx.x; d < H; d += 256) ty[d] = expf(-(float)(d * d) * inv2sy2);
  __syncthreads();
  const int n = H * W;
  for (int px = blockIdx.x * 256 + threadIdx.x; px < n; px += gridDim.x * 256) {
    const int x = px % W, y = px / W;
    float sx = 0.f, sy = 0.f;
    for (int xx = 0; xx < W; ++xx) sx += tx[abs(x - xx)];
    for (int yy = 0; yy < H; ++yy) sy += ty[abs(y - yy)];
    norm[px] = 1.f / sqrtf(sx * sy + 1e-20f);
  }
}

struct CrfAxisParams {
  const float* v; int ldv; const float* scale;      // scale: one factor per pixel of the image (the same for every image), or NULL
  float* out; int ldo;
  int L, lines, base_step, pos_step, n;             // pixel of position t on line l: l * base_step + t * pos_step
  float inv2s2;
};

// one axis of the separable filter: out[line][o][c] = sum_t table[|o - t|] * scale * v[line][t][c] over the WHOLE line.
// A workgroup owns 32 consecutive output positions of one line (8 groups of 4) x 32 columns and walks the line in chunks of 64
// source positions staged in LDS.
__global__ __launch_bounds__(256) void crf_gauss_axis_kernel(CrfAxisParams p) {
  extern __shared__ float crf_tab[];          // [L] table, then [64][32] staged rows
  float* tab = crf_tab;
  float* vs = crf_tab + (p.L + 3) / 4 * 4;
  crf_axis_table(tab, p.L, p.inv2s2);
  const int line = blockIdx.y;
  const size_t img0 = (size_t)blockIdx.z * p.n;
  const int base = line * p.base_step;
  const int c = threadIdx.x & 31, og = threadIdx.x >> 5;
  const int o0 = blockIdx.x * 32 + og * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < p.L; s0 += 64) {
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 8; e += 256) {
      const int s = e >> 3, c4 = e & 7, pos = s0 + s;
      float4 q = zero4();
      if (pos < p.L) {
        const int px = base + pos * p.pos_step;
        q = ld4(p.v + (img0 + px) * p.ldv + c4 * 4);
        if (p.scale) {
          const float f = p.scale[px];
          q = make_float4(q.x * f, q.y * f, q.z * f, q.w * f);
        }
      }
      st4(vs + s * CRF_LP + c4 * 4, q);
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 64; ++s) {
      const float vv = vs[s * CRF_LP + c];
      const int t = s0 + s;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = min(abs(o0 + k - t), p.L - 1);        // (positions past the line: staged as 0, any table entry serves)
        acc[k] = fmaf(tab[d], vv, acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int o = o0 + k;
    if (o < p.L) p.out[(img0 + base + o * p.pos_step) * p.ldo + c] = acc[k];
  }
}

static bool crf_side_ok(int H, int W) { return H > 0 && W > 0 && H <= CRF_MAX_SIDE && W <= CRF_MAX_SIDE; }

extern "C" int dl3p_crf_gauss_norm(float* norm, int H, int W, float sx, float sy, void* stream) {
  const char* fn = "dl3p_crf_gauss_norm";
  DL3P_CHECK_ARG(norm && crf_side_ok(H, W), "%s: bad arguments (H=%d W=%d, sides up to %d)", fn, H, W, CRF_MAX_SIDE);
  DL3P_CHECK_ARG(sx > 0.f && sy > 0.f, "%s: the standard deviations must be positive (sx=%g sy=%g)", fn, (double)sx, (double)sy);
  int blocks = ceil_div(H * W, 256);
  if (blocks > DL3P_NUM_CUS * 8) blocks = DL3P_NUM_CUS * 8;
  hipLaunchKernelGGL(crf_gauss_norm_kernel, dim3(blocks), dim3(256), (size_t)(H + W) * sizeof(float), (hipStream_t)stream, norm, H,
                     W, (float)(0.5 / ((double)sx * sx)), (float)(0.5 / ((double)sy * sy)));
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_crf_gauss_message(const float* v, int ldv, const float* scale, float* tmp, float* out, int ldo, int N, int H,
                                      int W, float sx, float sy, void* stream) {
  const char* fn = "dl3p_crf_gauss_message";
  DL3P_CHECK_ARG(v && tmp && out && N > 0 && crf_side_ok(H, W), "%s: bad arguments (N=%d H=%d W=%d, sides up to %d)", fn, N, H, W,
                 CRF_MAX_SIDE);
  DL3P_CHECK_ARG(N <= 65535, "%s: N=%d is past the grid's z range", fn, N);
  DL3P_CHECK_ARG(sx > 0.f && sy > 0.f, "%s: the standard deviations must be positive (sx=%g sy=%g)", fn, (double)sx, (double)sy);
  DL3P_CHECK_ARG(aligned16(v) && ldv % 4 == 0 && ldv >= CRF_LP && aligned16(tmp) && ldo >= CRF_LP,
                 "%s: V and the scratch rows are 16-byte aligned, strides >= %d and (V) a multiple of 4 (ldv=%d ldo=%d)", fn, CRF_LP,
                 ldv, ldo);
  hipStream_t st = (hipStream_t)stream;
  CrfAxisParams p = {};
  p.n = H * W;
  // rows: tmp (N, n, 32) dense
  p.v = v; p.ldv = ldv; p.scale = scale; p.out = tmp; p.ldo = CRF_LP;
  p.L = W; p.lines = H; p.base_step = W; p.pos_step = 1; p.inv2s2 = (float)(0.5 / ((double)sx * sx));
  size_t lds = ((size_t)(p.L + 3) / 4 * 4 + 64 * CRF_LP) * sizeof(float);
  hipLaunchKernelGGL(crf_gauss_axis_kernel, dim3(ceil_div(p.L, 32), p.lines, N), dim3(256), lds, st, p);
  DL3P_CHECK_LAUNCH(fn);
  // columns
  p.v = tmp; p.ldv = CRF_LP; p.scale = nullptr; p.out = out; p.ldo = ldo;
  p.L = H; p.lines = W; p.base_step = 1; p.pos_step = W; p.inv2s2 = (float)(0.5 / ((double)sy * sy));
  lds = ((size_t)(p.L + 3) / 4 * 4 + 64 * CRF_LP) * sizeof(float);
  hipLaunchKernelGGL(crf_gauss_axis_kernel, dim3(ceil_div(p.L, 32), p.lines, N), dim3(256), lds, st, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// ------------------------------------------------------------------------------ bilateral message (fp32 MFMA)
struct CrfBilateralParams {
  const unsigned char* img;      // (N, n, 3)
  const float* v; int ldv;       // (N, n, ldv), or NULL: V is the unit column 0 (the normaliser's run)
  const float* scale;            // (N, n) factor per pixel j, or NULL
  float* out; int ldo;           // (N, n, ldo), columns [0, 32) written
  float* norm_out;               // (N, n): 1 / sqrt(column 0 + 1e-20), or NULL
  int n, W;
  float ca, cc;                  // -0.5 log2(e) / sxy^2, -0.5 log2(e) / srgb^2
};

// Workgroup: 128 pixels i (wave w: rows 32 w .. 32 w + 31), all pixels j in chunks of 256.  v_mfma_f32_32x32x2_f32 takes
// A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][col = lane & 31]: lane l of a step that covers the chunk rows jj, jj + 1
// forms k(i, jj + (l >> 5)) and reads V[jj + (l >> 5)][l & 31].  The coordinates and colours are small integers held as floats,
// so the squared distances are exact; the only roundings before the exp are the two scalings and their sum.
__global__ __launch_bounds__(256) void crf_bilateral_kernel(CrfBilateralParams p) {
  __shared__ float vs[CRF_CHUNK * CRF_LP];          // 32 KiB
  __shared__ float4 fa[CRF_CHUNK];                  // x, y, r, g
  __shared__ float fb[CRF_CHUNK];                   // b
  const int img = blockIdx.y;
  const unsigned char* im = p.img + (size_t)img * p.n * 3;
  const float* v = p.v ? p.v + (size_t)img * p.n * p.ldv : nullptr;
  const float* scale = p.scale ? p.scale + (size_t)img * p.n : nullptr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = lane >> 5, r = lane & 31;
  const int i0 = blockIdx.x * CRF_TILE + wave * 32;
  const int ic = min(i0 + r, p.n - 1);              // rows past n compute on the last pixel and are not stored
  const float xi = (float)(ic % p.W), yi = (float)(ic / p.W);
  const float ri = (float)im[(size_t)ic * 3], gi = (float)im[(size_t)ic * 3 + 1], bi = (float)im[(size_t)ic * 3 + 2];
  crf_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int j0 = 0; j0 < p.n; j0 += CRF_CHUNK) {
    __syncthreads();
    {
      const int jc = min(j0 + (int)threadIdx.x, p.n - 1);
      fa[threadIdx.x] = make_float4((float)(jc % p.W), (float)(jc / p.W), (float)im[(size_t)jc * 3], (float)im[(size_t)jc * 3 + 1]);
      fb[threadIdx.x] = (float)im[(size_t)jc * 3 + 2];
    }
    for (int e = threadIdx.x; e < CRF_CHUNK * 8; e += 256) {
      const int row = e >> 3, c4 = e & 7, j = j0 + row;
      float4 q = zero4();                            // rows past n contribute 0
      if (j < p.n) {
        if (v) {
          q = ld4(v + (size_t)j * p.ldv + c4 * 4);
          if (scale) {
            const float f = scale[j];
            q = make_float4(q.x * f, q.y * f, q.z * f, q.w * f);
          }
        } else if (c4 == 0) {
          q.x = 1.f;
        }
      }
      st4(vs + row * CRF_LP + c4 * 4, q);
    }
    __syncthreads();
#pragma unroll 8
    for (int jj = 0; jj < CRF_CHUNK; jj += 2) {
      const float4 f = fa[jj + h];
      const float fbj = fb[jj + h];
      const float dx = xi - f.x, dy = yi - f.y, dr = ri - f.z, dg = gi - f.w, db = bi - fbj;
      const float d2 = fmaf(dy, dy, dx * dx);
      const float c2 = fmaf(db, db, fmaf(dg, dg, dr * dr));
      const float k = __builtin_amdgcn_exp2f(fmaf(c2, p.cc, d2 * p.ca));
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k, vs[(jj + h) * CRF_LP + r], acc, 0, 0, 0);
    }
  }
  // C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const size_t row0 = (size_t)img * p.n;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (i < p.n) {
      if (p.out) p.out[(row0 + i) * p.ldo + r] = acc[e];
      if (p.norm_out && r == 0) p.norm_out[row0 + i] = 1.f / sqrtf(acc[e] + 1e-20f);
    }
  }
}

extern "C" int dl3p_crf_bilateral_message(const unsigned char* img, const float* v, int ldv, const float* scale, float* out, int ldo,
                                          float* norm_out, int N, int H, int W, float sxy, float srgb, void* stream) {
  const char* fn = "dl3p_crf_bilateral_message";
  DL3P_CHECK_ARG(img && N > 0 && crf_side_ok(H, W), "%s: bad arguments (N=%d H=%d W=%d, sides up to %d)", fn, N, H, W, CRF_MAX_SIDE);
  DL3P_CHECK_ARG(N <= 65535, "%s: N=%d is past the grid's y range", fn, N);
  DL3P_CHECK_ARG(sxy > 0.f && srgb > 0.f, "%s: the standard deviations must be positive (sxy=%g srgb=%g)", fn, (double)sxy,
                 (double)srgb);
  DL3P_CHECK_ARG(out || norm_out, "%s: nothing to produce", fn);
  DL3P_CHECK_ARG(v || !scale, "%s: a scale comes with a V", fn);
  DL3P_CHECK_ARG(!v || (aligned16(v) && ldv % 4 == 0 && ldv >= CRF_LP),
                 "%s: V rows are 16-byte aligned with a stride that is a multiple of 4 and >= %d (ldv=%d)", fn, CRF_LP, ldv);
  DL3P_CHECK_ARG(!out || ldo >= CRF_LP, "%s: output rows hold %d columns (ldo=%d)", fn, CRF_LP, ldo);
  CrfBilateralParams p = {};
  p.img = img; p.v = v; p.ldv = ldv; p.scale = scale; p.out = out; p.ldo = ldo; p.norm_out = norm_out;
  p.n = H * W; p.W = W;
  const double log2e = 1.4426950408889634;
  p.ca = (float)(-0.5 * log2e / ((double)sxy * sxy));
  p.cc = (float)(-0.5 * log2e / ((double)srgb * srgb));
  hipLaunchKernelGGL(crf_bilateral_kernel, dim3(ceil_div(p.n, CRF_TILE), N), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// ------------------------------------------------------------------------------ front-end helpers
// confusion[label][mask] += 1 for a mask that is already there (dl3p_argmax_confusion's counting half)
__global__ __launch_bounds__(256) void crf_mask_confusion_kernel(const int32_t* pred, const float* labels, unsigned long long* cm,
                                                                 long long total, int C) {
  extern __shared__ unsigned int crf_hist[];
  const ConfusionHist hist = confusion_begin(crf_hist, cm, C, true);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < total; s += (long long)gridDim.x * 256) {
    const int arg = pred[s];
    if (arg >= 0 && arg < C) hist.count((int)labels[s], arg);
  }
  hist.flush();
}

extern "C" int dl3p_mask_confusion(const int* pred_mask, const float* labels, unsigned long long* confusion, size_t total, int C,
                                   void* stream) {
  const char* fn = "dl3p_mask_confusion";
  DL3P_CHECK_ARG(pred_mask && labels && confusion && total > 0, "%s: needs a mask, labels and the counters", fn);
  DL3P_CHECK_ARG(C >= 1 && C <= 64, "%s: C=%d is outside [1, 64]", fn, C);
  long long blocks = ceil_div_ll((long long)total, 256);
  if (blocks > DL3P_NUM_CUS * 8) blocks = DL3P_NUM_CUS * 8;
  hipLaunchKernelGGL(crf_mask_confusion_kernel, dim3((unsigned)blocks), dim3(256), (size_t)C * C * sizeof(unsigned int),
                     (hipStream_t)stream, pred_mask, labels, confusion, (long long)total, C);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// the reference's denormalize_image: (x * 127.5 + 127.5) truncated to uint8 (values outside [0, 255] are clamped first)
__global__ __launch_bounds__(256) void crf_denormalize_kernel(const float* x, unsigned char* out, size_t total) {
  for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < total; s += (size_t)gridDim.x * 256)
    out[s] = (unsigned char)fminf(fmaxf(x[s] * 127.5f + 127.5f, 0.f), 255.f);
}

extern "C" int dl3p_denormalize_u8(const float* x, unsigned char* out, size_t total, void* stream) {
  const char* fn = "dl3p_denormalize_u8";
  DL3P_CHECK_ARG(x && out && total > 0, "%s: needs an input, an output and a size", fn);
  long long blocks = ceil_div_ll((long long)total, 256);
  if (blocks > DL3P_NUM_CUS * 8) blocks = DL3P_NUM_CUS * 8;
  hipLaunchKernelGGL(crf_denormalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, out, total);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
