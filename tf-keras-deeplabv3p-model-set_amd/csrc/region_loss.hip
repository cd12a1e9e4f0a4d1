// Region losses (soft Dice, soft Jaccard, Tversky) behind the bilinear head.  A region loss is not a sum of
// per-pixel terms: its gradient at a pixel needs per-class sums over the whole batch.  Three stages:
//   sums      one pass over the full-resolution pixels: I_c = sum p_ic [y_i == c], P_c = sum p_ic, Y_c = |{y_i == c}| over the valid
//             pixels, reduced thread -> wave (__shfl_xor) -> workgroup (LDS, fixed order) into one partial row [3][Cpad] per workgroup
//   finalize  one workgroup adds the rows in fixed order in float64 and leaves the record {rho R, |S|, 0, 0, T[Cpad], A[Cpad], B[Cpad]}
//   gradient  the head once more: base_weight * (the per-pixel loss' gradient) + p (g - p.g), g_c = B_c - [y == c] A_c, in one store
// No floating-point atomics (Y_c is counted in integers in LDS), no (N,H,W,C) probability tensor, the same bits on every run.  The
// bilinear rule, the softmax, the label rule and the per-pixel loss term are the training heads': csrc/head_common.h.
#include "head_common.h"
#include <math.h>

namespace {

constexpr int REC_HEAD = 4;                                   // record words in front of T / A / B
constexpr int SUMS_BLOCK_CAP = DL3P_NUM_CUS * 4 < DL3P_MAX_STAT_ROWS ? DL3P_NUM_CUS * 4 : DL3P_MAX_STAT_ROWS;

struct SumsParams {
  const float* z; int ldz; const float* labels; int ignore_index;
  float* rows;                                                // [gridDim.x][3][cpad]: float I, float P, int32 Y
  int N, h, w, C, H, W, cpad;
  long long total;
};

// CP > 0: one thread per pixel with the padded class vector and both accumulator sets in registers
template <int CP>
__global__ __launch_bounds__(256) void region_sums_kernel(SumsParams p) {
  __shared__ float part[4][2 * CP];
  __shared__ unsigned hist[CP];
  if (threadIdx.x < CP) hist[threadIdx.x] = 0u;
  __syncthreads();
  float ai[CP], ap[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) ai[c] = ap[c] = 0.f;
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    const int lab = (int)p.labels[s];
    if (!label_valid(lab, p.ignore_index, p.C)) continue;
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
    float v[CP];
    tap_logits<CP>(v, Taps(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W));
    const float inv = softmax_exp<CP>(v, p.C);
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float pr = v[c] * inv;
      ap[c] += pr;
      ai[c] += c == lab ? pr : 0.f;
    }
    atomicAdd(&hist[lab], 1u);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float si = wave_sum(ai[c]), sp = wave_sum(ap[c]);
    if (lane == 0) { part[wave][c] = si; part[wave][CP + c] = sp; }
  }
  __syncthreads();
  float* row = p.rows + (size_t)blockIdx.x * 3 * CP;          // (CP == cpad here)
  if (threadIdx.x < 2 * CP)
    row[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
  if (threadIdx.x < CP) reinterpret_cast<int*>(row)[2 * CP + threadIdx.x] = (int)hist[threadIdx.x];
}

// More than 32 classes: the classes are walked (softmax_walk); a wave adds each class' 64 probabilities with shuffles and its first
// lane keeps the wave's running sums in LDS.  Whole waves stay in the loop, lanes without a valid pixel add zeros.
__global__ __launch_bounds__(256) void region_sums_walk_kernel(SumsParams p) {
  __shared__ float part[4][2][256];
  __shared__ unsigned hist[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  hist[threadIdx.x] = 0u;
  for (int c = lane; c < 256; c += 64) part[wave][0][c] = part[wave][1][c] = 0.f;
  __syncthreads();
  for (long long sw = (long long)blockIdx.x * 256 + threadIdx.x; sw - lane < p.total; sw += (long long)gridDim.x * 256) {
    const bool live = sw < p.total;
    const long long s = live ? sw : p.total - 1;
    const int lab = (int)p.labels[s];
    const bool on = live && label_valid(lab, p.ignore_index, p.C);
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
    const SoftmaxWalk k = softmax_walk(Taps(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W), p.C);
    if (on) atomicAdd(&hist[lab], 1u);
    for (int c = 0; c < p.C; ++c) {
      const float pr = on ? k.prob(c) : 0.f;
      const float sp = wave_sum(pr), si = wave_sum(c == lab ? pr : 0.f);
      if (lane == 0) { part[wave][0][c] += si; part[wave][1][c] += sp; }
    }
  }
  __syncthreads();
  float* row = p.rows + (size_t)blockIdx.x * 3 * p.cpad;
  for (int i = threadIdx.x; i < 2 * p.cpad; i += 256) {
    const int q = i / p.cpad, c = i - q * p.cpad;
    row[i] = (part[0][q][c] + part[1][q][c]) + (part[2][q][c] + part[3][q][c]);
  }
  for (int c = threadIdx.x; c < p.cpad; c += 256) reinterpret_cast<int*>(row)[2 * p.cpad + c] = (int)hist[c];
}

// ------------------------------------------------------------------------------ finalize
// 256 threads: column j of the [3][cpad] rows is added by G = 256 / (3 cpad) threads, each over the rows g, g + G, ... in order, then
// their G sums in order (more than 256 columns: one thread per column, over all rows).  All in float64; the counts are exact.
__global__ __launch_bounds__(256) void region_finalize_kernel(const float* rows, int nrows, int C, int cpad, double alpha, double beta,
                                                              double smooth, double rho, float* record) {
  __shared__ double slice[256];
  __shared__ double tot[3 * 256];
  __shared__ double term[256];
  __shared__ int present;
  const int t = threadIdx.x, ncol = 3 * cpad;
  if (ncol <= 256) {
    const int G = 256 / ncol, g = t / ncol, j = t - g * ncol;
    double acc = 0.0;
    if (g < G) {
      for (int r = g; r < nrows; r += G) {
        const float* row = rows + (size_t)r * ncol;
        acc += j < 2 * cpad ? (double)row[j] : (double)reinterpret_cast<const int*>(row)[j];
      }
      slice[t] = acc;
    }
    __syncthreads();
    if (t < ncol) {
      double sum = 0.0;
      for (int k = 0; k < G; ++k) sum += slice[k * ncol + t];
      tot[t] = sum;
    }
  } else {
    for (int j = t; j < ncol; j += 256) {
      double acc = 0.0;
      for (int r = 0; r < nrows; ++r) {
        const float* row = rows + (size_t)r * ncol;
        acc += j < 2 * cpad ? (double)row[j] : (double)reinterpret_cast<const int*>(row)[j];
      }
      tot[j] = acc;
    }
  }
  __syncthreads();
  if (t == 0) {
    int n = 0;
    for (int c = 0; c < C; ++c) n += tot[2 * cpad + c] > 0.0 ? 1 : 0;
    present = n;
  }
  __syncthreads();
  const int ns = present;
  float* T = record + REC_HEAD;
  float* A = T + cpad;
  float* B = A + cpad;
  for (int c = t; c < cpad; c += 256) {
    const bool in = c < C && tot[2 * cpad + c] > 0.0;
    float tc = __uint_as_float(0x7fc00000u), a = 0.f, b = 0.f;
    double one_minus = 0.0;
    if (in) {
      const double I = tot[c], Pc = tot[cpad + c], Y = tot[2 * cpad + c];
      const double rest = 1.0 - alpha - beta;
      const double D = rest * I + alpha * Pc + beta * Y + smooth;
      const double num = I + smooth;
      const double score = num / D;
      tc = (float)score;
      one_minus = 1.0 - score;
      a = (float)(rho * (1.0 / D - rest * num / (D * D)) / (double)ns);
      b = (float)(rho * (alpha * num / (D * D)) / (double)ns);
    }
    T[c] = tc; A[c] = a; B[c] = b;
    term[c] = one_minus;
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += term[c];
    record[0] = ns > 0 ? (float)(rho * sum / (double)ns) : 0.f;
    reinterpret_cast<int*>(record)[1] = ns;
    record[2] = record[3] = 0.f;
  }
}

// ------------------------------------------------------------------------------ gradient
struct GradParams {
  const float* z; int ldz; const float* labels; int ignore_index; float inv_count;
  int base_kind; const float* class_w; float focal_gamma, focal_alpha; const float* pixel_w; float base_weight;
  const float* rec_a; const float* rec_b; const float* rec_loss;
  float* dlogits; float* loss_partials;
  int N, h, w, C, H, W, ld_big;
  long long total;
};

// base_weight * l and base_weight * f * w_i * inv_count of the base term at one pixel (0, 0 without one)
__device__ __forceinline__ void base_term(const GradParams& p, float pt, bool valid, int lab, long long s, float* l, float* gs) {
  *l = 0.f; *gs = 0.f;
  if (p.base_kind == DL3P_REGION_BASE_NONE) return;
  float li, f;
  loss_term(p.base_kind, pt, valid, lab, p.class_w, p.focal_gamma, p.focal_alpha, &li, &f);
  if (p.pixel_w) {
    const float sw = p.pixel_w[s];
    li *= sw;
    f *= sw;
  }
  if (valid) { *l = p.base_weight * li; *gs = p.base_weight * f * p.inv_count; }
}

__device__ __forceinline__ void write_loss_rows(const GradParams& p, float loss) {
  __shared__ float wsum[4];
  loss = wave_sum(loss);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    p.loss_partials[blockIdx.x] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * p.inv_count;
    if (blockIdx.x == 0) p.loss_partials[gridDim.x] = *p.rec_loss;      // the last row: rho R
  }
}

template <int CP>
__global__ __launch_bounds__(256) void region_grad_kernel(GradParams p) {
  // a wave's 64 rows leave through a wave-private LDS slice as 1 KB-contiguous stores, like head_kernel's
  __shared__ __attribute__((aligned(16))) float tr_s[4][64 * (CP + 4)];
  float* trw = tr_s[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  const bool vec = p.ld_big == CP;
  float loss = 0.f;
  for (long long sw = (long long)blockIdx.x * 256 + threadIdx.x; sw - lane < p.total; sw += (long long)gridDim.x * 256) {
    const bool live = sw < p.total;
    const long long s = live ? sw : p.total - 1;
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
    float e[CP];
    tap_logits<CP>(e, Taps(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W));
    const float inv = softmax_exp<CP>(e, p.C);
    const int lab = (int)p.labels[s];
    const bool valid = label_valid(lab, p.ignore_index, p.C);
    float pt = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) if (c == lab) pt = e[c] * inv;
    float li, gs;
    base_term(p, pt, valid, lab, s, &li, &gs);
    if (live) loss += li;
    if (!p.dlogits) continue;
    // g_c = B_c - [c == y] A_c;  dot = sum_c p_c g_c
    const float pa = valid ? pt * p.rec_a[lab] : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) dot += c < p.C ? e[c] * inv * p.rec_b[c] : 0.f;
    dot -= pa;
    float d[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float pr = e[c] * inv, oh = c == lab ? 1.f : 0.f;
      d[c] = (valid && c < p.C) ? gs * (pr - oh) + (pr * (p.rec_b[c] - dot) - oh * pa) : 0.f;
    }
    if (vec) {
#pragma unroll
      for (int c4 = 0; c4 < CP / 4; ++c4)
        *reinterpret_cast<float4*>(&trw[lane * (CP + 4) + c4 * 4]) = make_float4(d[c4 * 4], d[c4 * 4 + 1], d[c4 * 4 + 2], d[c4 * 4 + 3]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // other lanes' rows are read next
      const long long s0 = sw - lane;
      const int npx = (int)(p.total - s0 < 64 ? p.total - s0 : 64);
#pragma unroll
      for (int k = 0; k < CP / 4; ++k) {
        const int f = lane + 64 * k;
        const int r = f / (CP / 4), cc = f - r * (CP / 4);
        if (r < npx) st4(p.dlogits + (size_t)s0 * CP + (size_t)f * 4, *reinterpret_cast<const float4*>(&trw[r * (CP + 4) + cc * 4]));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // ... before the next pixel's writes
    } else if (live) {
      float* o = p.dlogits + (size_t)s * p.ld_big;
#pragma unroll
      for (int c = 0; c < CP; ++c) if (c < p.C) o[c] = d[c];
      for (int c = p.C; c < p.ld_big; ++c) o[c] = 0.f;
    }
  }
  write_loss_rows(p, loss);
}

__global__ __launch_bounds__(256) void region_grad_walk_kernel(GradParams p) {
  float loss = 0.f;
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
    const SoftmaxWalk k = softmax_walk(Taps(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W), p.C);
    const int lab = (int)p.labels[s];
    const bool valid = label_valid(lab, p.ignore_index, p.C);
    const float pt = valid ? k.prob(lab) : 0.f;
    float li, gs;
    base_term(p, pt, valid, lab, s, &li, &gs);
    loss += li;
    if (!p.dlogits) continue;
    float* o = p.dlogits + (size_t)s * p.ld_big;
    const float pa = valid ? pt * p.rec_a[lab] : 0.f;
    float dot = 0.f;
    if (valid) {
      for (int c = 0; c < p.C; ++c) dot += k.prob(c) * p.rec_b[c];
      dot -= pa;
    }
    for (int c = 0; c < p.ld_big; ++c) {
      float d = 0.f;
      if (valid && c < p.C) {
        const float pr = k.prob(c), oh = c == lab ? 1.f : 0.f;
        d = gs * (pr - oh) + (pr * (p.rec_b[c] - dot) - oh * pa);
      }
      o[c] = d;
    }
  }
  write_loss_rows(p, loss);
}

int check_shape(const char* fn, const float* z, int ldz, const float* labels, int N, int h, int w, int C, int H, int W) {
  DL3P_CHECK_ARG(z && aligned16(z) && ldz % 4 == 0, "%s: logits must be 16-byte aligned, ld %% 4 == 0", fn);
  DL3P_CHECK_ARG(C > 0 && C <= 256 && ldz >= (C + 3) / 4 * 4, "%s: C=%d (ld=%d) unsupported", fn, C, ldz);
  DL3P_CHECK_ARG(labels, "%s: labels are required", fn);
  DL3P_CHECK_ARG(N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1ll << 31), "%s: N*H*W = %lld must lie in [1, 2^31)", fn,
                 (long long)N * H * W);
  DL3P_CHECK_ARG(h > 0 && w > 0 && h <= H && w <= W, "%s: (h, w) = (%d, %d) must lie in [1, (H, W) = (%d, %d)]", fn, h, w, H, W);
  return DL3P_OK;
}

bool finite_f(float v) { return isfinite(v); }

}  // namespace

extern "C" size_t dl3p_region_workspace(int C) {
  if (C < 1 || C > 256) return 0;
  return (size_t)DL3P_MAX_STAT_ROWS * 3 * ((C + 3) / 4 * 4) * sizeof(float);
}

extern "C" int dl3p_region_sums(const float* z, int ldz, const float* labels, int ignore_index, void* workspace, int* rows_out, int N,
                                int h, int w, int C, int H, int W, void* stream) {
  const char* fn = "dl3p_region_sums";
  const int rc = check_shape(fn, z, ldz, labels, N, h, w, C, H, W);
  if (rc) return rc;
  DL3P_CHECK_ARG(workspace && aligned16(workspace) && rows_out, "%s: a 16-byte aligned workspace and rows_out are required", fn);
  SumsParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels; p.ignore_index = ignore_index; p.rows = (float*)workspace;
  p.N = N; p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.cpad = (C + 3) / 4 * 4;
  p.total = (long long)N * H * W;
  long long blocks = ceil_div_ll(p.total, 256);
  if (blocks > SUMS_BLOCK_CAP) blocks = SUMS_BLOCK_CAP;
  *rows_out = (int)blocks;
  hipStream_t st = (hipStream_t)stream;
  switch (C > 32 ? 0 : p.cpad) {
    case 0: hipLaunchKernelGGL(region_sums_walk_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p); break;
#define DL3P_SUMS_CASE(CP) case CP: hipLaunchKernelGGL((region_sums_kernel<CP>), dim3((unsigned)blocks), dim3(256), 0, st, p); break;
    DL3P_SUMS_CASE(4) DL3P_SUMS_CASE(8) DL3P_SUMS_CASE(12) DL3P_SUMS_CASE(16) DL3P_SUMS_CASE(20) DL3P_SUMS_CASE(24)
    DL3P_SUMS_CASE(28) DL3P_SUMS_CASE(32)
#undef DL3P_SUMS_CASE
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_region_finalize(const void* workspace, int rows, int C, float alpha, float beta, float smooth, float region_weight,
                                    void* record, void* stream) {
  const char* fn = "dl3p_region_finalize";
  DL3P_CHECK_ARG(workspace && aligned16(workspace) && record && aligned16(record),
                 "%s: the workspace and the record must be 16-byte aligned", fn);
  DL3P_CHECK_ARG(C > 0 && C <= 256, "%s: C=%d unsupported", fn, C);
  DL3P_CHECK_ARG(rows >= 1 && rows <= DL3P_MAX_STAT_ROWS, "%s: rows = %d must lie in [1, %d]", fn, rows, DL3P_MAX_STAT_ROWS);
  DL3P_CHECK_ARG(finite_f(alpha) && finite_f(beta) && finite_f(smooth) && finite_f(region_weight) && alpha > 0.f && beta > 0.f &&
                 smooth >= 0.f && region_weight > 0.f,
                 "%s: alpha = %g and beta = %g must be > 0, smooth = %g >= 0, region_weight = %g > 0, all finite", fn, alpha, beta,
                 smooth, region_weight);
  hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, rows, C,
                     (C + 3) / 4 * 4, (double)alpha, (double)beta, (double)smooth, (double)region_weight, (float*)record);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_region_head_grad(const float* z, int ldz, const float* labels, int ignore_index, float inv_count, int base_kind,
                                     const float* class_weights, float focal_gamma, float focal_alpha, const float* pixel_weights,
                                     float base_weight, const void* record, float* dlogits_big, int ld_big, float* loss_partials,
                                     int* rows_out, int N, int h, int w, int C, int H, int W, void* stream) {
  const char* fn = "dl3p_region_head_grad";
  const int rc = check_shape(fn, z, ldz, labels, N, h, w, C, H, W);
  if (rc) return rc;
  DL3P_CHECK_ARG(base_kind == DL3P_REGION_BASE_NONE || base_kind == DL3P_LOSS_CE || base_kind == DL3P_LOSS_FOCAL ||
                 (base_kind == DL3P_LOSS_WEIGHTED_CE && class_weights),
                 "%s: bad base kind %d (weighted CE needs class_weights[C])", fn, base_kind);
  DL3P_CHECK_ARG(finite_f(base_weight) && base_weight >= 0.f, "%s: base_weight = %g must be finite and >= 0", fn, base_weight);
  DL3P_CHECK_ARG(record && aligned16(record) && loss_partials && rows_out,
                 "%s: a 16-byte aligned record, loss_partials and rows_out are required", fn);
  DL3P_CHECK_ARG(!dlogits_big || (ld_big >= C && (ld_big % 4 || aligned16(dlogits_big))), "%s: bad ld_big=%d", fn, ld_big);
  const int cpad = (C + 3) / 4 * 4;
  GradParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels; p.ignore_index = ignore_index; p.inv_count = inv_count;
  p.base_kind = base_kind; p.class_w = class_weights; p.focal_gamma = focal_gamma; p.focal_alpha = focal_alpha;
  p.pixel_w = pixel_weights; p.base_weight = base_weight;
  p.rec_loss = (const float*)record;
  p.rec_a = p.rec_loss + REC_HEAD + cpad;
  p.rec_b = p.rec_a + cpad;
  p.dlogits = dlogits_big; p.loss_partials = loss_partials;
  p.N = N; p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.ld_big = ld_big;
  // the value of a pure region loss is in the record already: no pixel is visited
  p.total = (!dlogits_big && base_kind == DL3P_REGION_BASE_NONE) ? 0 : (long long)N * H * W;
  long long blocks = ceil_div_ll(p.total, 256);
  if (blocks < 1) blocks = 1;
  if (blocks > DL3P_MAX_STAT_ROWS - 1) blocks = DL3P_MAX_STAT_ROWS - 1;      // one more row holds rho R
  *rows_out = (int)blocks + 1;
  hipStream_t st = (hipStream_t)stream;
  if (C > 32) {
    hipLaunchKernelGGL(region_grad_walk_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p);
    DL3P_CHECK_LAUNCH(fn);
    return DL3P_OK;
  }
  int cp = cpad;
  // rows padded further (the bf16 graphs pad 19 classes to 24): the instantiation that matches the row, so that it leaves as vectors
  if (dlogits_big && ld_big % 4 == 0 && ld_big > cp && ld_big <= 32 && ldz >= ld_big) cp = ld_big;
  switch (cp) {
#define DL3P_GRAD_CASE(CP) case CP: hipLaunchKernelGGL((region_grad_kernel<CP>), dim3((unsigned)blocks), dim3(256), 0, st, p); break;
    DL3P_GRAD_CASE(4) DL3P_GRAD_CASE(8) DL3P_GRAD_CASE(12) DL3P_GRAD_CASE(16) DL3P_GRAD_CASE(20) DL3P_GRAD_CASE(24)
    DL3P_GRAD_CASE(28) DL3P_GRAD_CASE(32)
#undef DL3P_GRAD_CASE
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
