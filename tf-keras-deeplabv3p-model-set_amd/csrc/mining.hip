// Hard-example mining (DeepLab's top_k_percent_pixels / hard_example_mining_step): the loss and its gradient
// come from the k pixels of the batch whose loss is highest.  Three stages in front of the weighted training heads:
//   map      the forward of the head into a compact per-pixel loss map l[N*H*W] (and the first radix histogram of its keys)
//   select   an exact radix select of the k-th largest value: 4 passes of 8 bits over an order-preserving 32-bit key, each pass a
//            histogram launch and a one-workgroup scan that narrows the prefix and the remaining rank
//   weights  w_i = (l_i >= theta) * base_i * scale, the pixel_weights buffer the head reads next
// Counting is done in integers only (workgroup-private LDS bins flushed with integer atomics, like argmax_confusion_kernel), so
// every result is the same bit for bit in any order.  Per-pixel loss definitions, clipping constants and masking are the training
// heads': loss_term and label_valid of csrc/head_common.h.
#include "head_common.h"

namespace {

// workspace words (uint32): hist[4][256], then the count of exact zeros and the select's running state
constexpr int WS_ZEROS = 1024, WS_PREFIX = 1025, WS_RANK = 1026, WS_ABOVE = 1027, WS_WORDS = 1028;
// record words: {int32 k, float theta, int32 m, int32 m_plus, float scale, 0, 0, 0}
constexpr int REC_K = 0, REC_THETA = 1, REC_M = 2, REC_MPLUS = 3, REC_SCALE = 4, REC_WORDS = 8;
constexpr int MAP_BLOCK_CAP = DL3P_NUM_CUS * 4;

// float order -> unsigned order: +inf above every finite value, -0.0 counted as +0.0
__device__ __forceinline__ unsigned key_of(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct Bins {
  unsigned* bins;      // LDS [256]
  unsigned* zeros;     // LDS [1]
  unsigned prefix, mask_hi;
  int shift;
  bool first;
  __device__ __forceinline__ void tally(float v) const {
    const unsigned k = key_of(v);
    if ((k & mask_hi) == prefix) atomicAdd(&bins[(k >> shift) & 255u], 1u);
    if (first && v == 0.f) atomicAdd(zeros, 1u);
  }
};

__device__ __forceinline__ Bins bins_begin(unsigned* lds, const unsigned* ws, int pass) {
  lds[threadIdx.x] = 0u;                       // 256 threads
  if (threadIdx.x == 0) lds[256] = 0u;
  __syncthreads();
  Bins b;
  b.bins = lds; b.zeros = lds + 256;
  b.shift = 24 - 8 * pass;
  b.first = pass == 0;
  b.prefix = pass ? ws[WS_PREFIX] : 0u;
  b.mask_hi = pass ? (0xffffffffu << (b.shift + 8)) : 0u;
  return b;
}
__device__ __forceinline__ void bins_flush(const unsigned* lds, unsigned* ws, int pass) {
  __syncthreads();
  const unsigned c = lds[threadIdx.x];
  if (c) atomicAdd(&ws[pass * 256 + threadIdx.x], c);
  if (pass == 0 && threadIdx.x == 0 && lds[256]) atomicAdd(&ws[WS_ZEROS], lds[256]);
}

// ------------------------------------------------------------------------------ the per-pixel loss
struct MapParams {
  const float* z; int ldz; const float* labels; int ignore_index;
  int loss_kind; const float* class_w; float focal_gamma, focal_alpha; const float* pixel_w;
  float* map; unsigned* ws;
  int N, h, w, C, H, W, r, cp;
  long long total;
};

// loss_term's l(p_t) times the pixel weight, 0 for a pixel the head leaves out of its sum; -0.0 becomes +0.0
__device__ __forceinline__ float pixel_loss(const MapParams& p, float pt, bool valid, int lab, float sw) {
  float li, f;
  loss_term(p.loss_kind, pt, valid, lab, p.class_w, p.focal_gamma, p.focal_alpha, &li, &f);
  li *= sw;
  if (!valid || li == 0.f) li = 0.f;
  return li;
}

// one thread per full-resolution pixel; CP > 0: the padded class vector in registers (head_kernel), CP == 0: three walks over the
// classes (head_kernel_big)
template <int CP>
__global__ __launch_bounds__(256) void loss_map_kernel(MapParams p) {
  __shared__ unsigned lds[257];
  const Bins b = bins_begin(lds, p.ws, 0);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
    const Taps t(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W);
    const int lab = (int)p.labels[s];
    const bool valid = label_valid(lab, p.ignore_index, p.C);
    float pt = 0.f;
    if constexpr (CP > 0) {
      float v[CP];
      tap_logits<CP>(v, t);
      const float inv = softmax_exp<CP>(v, p.C);
#pragma unroll
      for (int c = 0; c < CP; ++c) if (c == lab) pt = v[c] * inv;
    } else {
      const SoftmaxWalk k = softmax_walk(t, p.C);
      pt = valid ? k.prob(lab) : 0.f;
    }
    const float l = pixel_loss(p, pt, valid, lab, p.pixel_w ? p.pixel_w[s] : 1.f);
    p.map[s] = l;
    b.tally(l);
  }
  bins_flush(lds, p.ws, 0);
}

// behind a nearest upsampling: a wave owns a logit pixel, lane l holds the classes [4 l, 4 l + 4) and the label l of the r x r block
__global__ __launch_bounds__(256) void nearest_loss_map_kernel(MapParams p) {
  __shared__ unsigned lds[257];
  const Bins b = bins_begin(lds, p.ws, 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rr = p.r * p.r;
  const int li = lane / p.r, lj = lane - li * p.r;
  for (long long s = (long long)blockIdx.x * 4 + wave; s < p.total; s += (long long)gridDim.x * 4) {   // wave-uniform
    int x, y;
    long long n;
    pixel_of(s, p.w, p.h, &x, &y, &n);
    const float4 pr = wave_softmax(p.z + (size_t)s * p.ldz, lane, p.C, p.cp);
    int lab = -1;
    float swt = 1.f;
    size_t f = 0;
    if (lane < rr) {
      f = ((size_t)n * p.H + (size_t)y * p.r + li) * p.W + (size_t)x * p.r + lj;
      lab = (int)p.labels[f];
      if (p.pixel_w) swt = p.pixel_w[f];
    }
    const bool valid = lane < rr && label_valid(lab, p.ignore_index, p.C);
    if (!valid) lab = -1;
    const float pt = wave_label_prob(pr, valid, lab);
    const float l = pixel_loss(p, pt, valid, valid ? lab : 0, swt);
    if (lane < rr) {
      p.map[f] = l;
      b.tally(l);
    }
  }
  bins_flush(lds, p.ws, 0);
}

// ------------------------------------------------------------------------------ radix select
// one pass' histogram over a map that is already there: 16-byte loads, the last P % 4 entries one by one
__global__ __launch_bounds__(256) void mining_hist_kernel(const float* map, long long P, unsigned* ws, int pass) {
  __shared__ unsigned lds[257];
  const Bins b = bins_begin(lds, ws, pass);
  const long long P4 = P >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P4; i += (long long)gridDim.x * 256) {
    const float4 v = ld4(map + i * 4);
    b.tally(v.x); b.tally(v.y); b.tally(v.z); b.tally(v.w);
  }
  if (blockIdx.x == 0 && P4 * 4 + threadIdx.x < P) b.tally(map[P4 * 4 + threadIdx.x]);
  bins_flush(lds, ws, pass);
}

// k of the rule, float64 in the order written (no contraction: the host oracle rounds every product and sum)
__device__ long long kept_count(long long P, double p, int M, long long s) {
#pragma clang fp contract(off)
  double kd;
  if (M == 0) {
    kd = p * (double)P;
  } else {
    const double r = fmin(1.0, (double)s / (double)M);
    const double a = r * p;
    const double c = 1.0 - r;
    kd = (a + c) * (double)P;
  }
  long long k = (long long)kd;
  return k < 1 ? 1 : (k > P ? P : k);
}

// one workgroup: the bin that holds the rank-th largest key of this pass' histogram; the last pass writes the record.  Every pass
// leaves its own histogram zeroed again, so a workspace that was zero before the map launch is zero after the select.
__global__ __launch_bounds__(256) void mining_scan_kernel(unsigned* ws, unsigned* record, int pass, long long P, double p, int M,
                                                          const long long* step_counter, int step_bias) {
  __shared__ unsigned hs[256];
  const int t = threadIdx.x;
  const unsigned hcount = ws[pass * 256 + t];
  hs[t] = hcount;
  unsigned rank, prefix, above_total;
  long long k = 0;
  if (pass == 0) {
    long long s = step_counter ? *step_counter + step_bias : 0;
    if (s < 0) s = 0;
    k = kept_count(P, p, M, s);
    rank = (unsigned)k; prefix = 0u; above_total = 0u;
  } else {
    rank = ws[WS_RANK]; prefix = ws[WS_PREFIX]; above_total = ws[WS_ABOVE];
  }
  const unsigned zeros = ws[WS_ZEROS];
  __syncthreads();
  ws[pass * 256 + t] = 0u;
  unsigned above = 0u;
  for (int u = t + 1; u < 256; ++u) above += hs[u];
  if (above < rank && rank <= above + hcount) {          // exactly one thread: the bins partition the keys under the prefix
    const int shift = 24 - 8 * pass;
    prefix |= (unsigned)t << shift;
    above_total += above;
    if (pass < 3) {
      ws[WS_PREFIX] = prefix; ws[WS_RANK] = rank - above; ws[WS_ABOVE] = above_total;
      if (pass == 0) record[REC_K] = (unsigned)k;
    } else {
      const float theta = value_of(prefix);
      const unsigned m = above_total + hcount;
      const unsigned mplus = theta <= 0.f ? m - zeros : m;      // every zero is kept once the threshold is at or below it
      record[REC_THETA] = __float_as_uint(theta);
      record[REC_M] = m;
      record[REC_MPLUS] = mplus;
      record[REC_SCALE] = __float_as_uint((float)((double)P / (double)(mplus > 1u ? mplus : 1u)));
      record[5] = record[6] = record[7] = 0u;
      ws[WS_ZEROS] = 0u;
    }
  }
}

// ------------------------------------------------------------------------------ weights
__global__ __launch_bounds__(256) void mining_weights_kernel(const float* map, const float* base, const unsigned* record, float* w,
                                                             long long P) {
  const float theta = __uint_as_float(record[REC_THETA]), scale = __uint_as_float(record[REC_SCALE]);
  const long long P4 = P >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P4; i += (long long)gridDim.x * 256) {
    const float4 l = ld4(map + i * 4);
    const float4 bw = base ? ld4(base + i * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
    st4(w + i * 4, make_float4(l.x >= theta ? bw.x * scale : 0.f, l.y >= theta ? bw.y * scale : 0.f,
                               l.z >= theta ? bw.z * scale : 0.f, l.w >= theta ? bw.w * scale : 0.f));
  }
  const long long j = P4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && j < P) w[j] = map[j] >= theta ? (base ? base[j] : 1.f) * scale : 0.f;
}

int check_map(const char* fn, const float* z, int ldz, const float* labels, int loss_kind, const float* class_weights,
              const float* loss_map, const void* workspace, int N, int C, int H, int W) {
  DL3P_CHECK_ARG(z && aligned16(z) && ldz % 4 == 0, "%s: logits must be 16-byte aligned, ld %% 4 == 0", fn);
  DL3P_CHECK_ARG(C > 0 && C <= 256 && ldz >= (C + 3) / 4 * 4, "%s: C=%d (ld=%d) unsupported", fn, C, ldz);
  DL3P_CHECK_ARG(loss_kind == DL3P_LOSS_CE || loss_kind == DL3P_LOSS_FOCAL || (loss_kind == DL3P_LOSS_WEIGHTED_CE && class_weights),
                 "%s: bad loss kind %d (weighted CE needs class_weights[C])", fn, loss_kind);
  DL3P_CHECK_ARG(labels && loss_map && aligned16(loss_map) && workspace && aligned16(workspace),
                 "%s: labels, a 16-byte aligned loss map and a 16-byte aligned workspace are required", fn);
  DL3P_CHECK_ARG(N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1ll << 31), "%s: N*H*W = %lld must lie in [1, 2^31)", fn,
                 (long long)N * H * W);
  return DL3P_OK;
}

long long stream_blocks(long long P) {
  long long blocks = ceil_div_ll((P >> 2) > 0 ? (P >> 2) : 1, 256);
  return blocks > MAP_BLOCK_CAP ? MAP_BLOCK_CAP : blocks;
}

}  // namespace

extern "C" size_t dl3p_mining_workspace(void) { return (size_t)WS_WORDS * sizeof(unsigned); }

extern "C" int dl3p_pixel_loss_map(const float* z, int ldz, const float* labels, int ignore_index, int loss_kind,
                                   const float* class_weights, float focal_gamma, float focal_alpha, const float* pixel_weights,
                                   float* loss_map, void* workspace, int N, int h, int w, int C, int H, int W, void* stream) {
  const char* fn = "dl3p_pixel_loss_map";
  const int rc = check_map(fn, z, ldz, labels, loss_kind, class_weights, loss_map, workspace, N, C, H, W);
  if (rc) return rc;
  DL3P_CHECK_ARG(h > 0 && w > 0 && h <= H && w <= W, "%s: (h, w) = (%d, %d) must lie in [1, (H, W) = (%d, %d)]", fn, h, w, H, W);
  MapParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels; p.ignore_index = ignore_index; p.loss_kind = loss_kind; p.class_w = class_weights;
  p.focal_gamma = focal_gamma; p.focal_alpha = focal_alpha; p.pixel_w = pixel_weights; p.map = loss_map;
  p.ws = (unsigned*)workspace;
  p.N = N; p.h = h; p.w = w; p.C = C; p.H = H; p.W = W;
  p.total = (long long)N * H * W;
  long long blocks = ceil_div_ll(p.total, 256);
  if (blocks > MAP_BLOCK_CAP) blocks = MAP_BLOCK_CAP;
  hipStream_t st = (hipStream_t)stream;
  switch (C > 32 ? 0 : (C + 3) / 4 * 4) {
#define DL3P_MAP_CASE(CP) case CP: hipLaunchKernelGGL((loss_map_kernel<CP>), dim3((unsigned)blocks), dim3(256), 0, st, p); break;
    DL3P_MAP_CASE(0) DL3P_MAP_CASE(4) DL3P_MAP_CASE(8) DL3P_MAP_CASE(12) DL3P_MAP_CASE(16) DL3P_MAP_CASE(20) DL3P_MAP_CASE(24)
    DL3P_MAP_CASE(28) DL3P_MAP_CASE(32)
#undef DL3P_MAP_CASE
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_nearest_pixel_loss_map(const float* z, int ldz, const float* labels, int ignore_index, int loss_kind,
                                           const float* class_weights, float focal_gamma, float focal_alpha,
                                           const float* pixel_weights, float* loss_map, void* workspace, int N, int h, int w, int C,
                                           int H, int W, void* stream) {
  const char* fn = "dl3p_nearest_pixel_loss_map";
  const int rc = check_map(fn, z, ldz, labels, loss_kind, class_weights, loss_map, workspace, N, C, H, W);
  if (rc) return rc;
  const int r = (h > 0 && w > 0 && H % h == 0 && W % w == 0 && H / h == W / w) ? H / h : 0;
  DL3P_CHECK_ARG(r >= 1 && r <= 8, "%s: (H, W) = (%d, %d) must be r in 1..8 times (h, w) = (%d, %d)", fn, H, W, h, w);
  MapParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels; p.ignore_index = ignore_index; p.loss_kind = loss_kind; p.class_w = class_weights;
  p.focal_gamma = focal_gamma; p.focal_alpha = focal_alpha; p.pixel_w = pixel_weights; p.map = loss_map;
  p.ws = (unsigned*)workspace;
  p.N = N; p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.r = r; p.cp = (C + 3) / 4 * 4;
  p.total = (long long)N * h * w;
  long long blocks = ceil_div_ll(p.total, 4);
  if (blocks > MAP_BLOCK_CAP) blocks = MAP_BLOCK_CAP;
  hipLaunchKernelGGL(nearest_loss_map_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_topk_threshold(const float* loss_map, size_t P, double top_k_percent, int mining_step,
                                   const int64_t* step_counter, int step_bias, int first_histogram_ready, void* workspace,
                                   void* record, void* stream) {
  const char* fn = "dl3p_topk_threshold";
  DL3P_CHECK_ARG(loss_map && aligned16(loss_map) && workspace && aligned16(workspace) && record && aligned16(record),
                 "%s: the loss map, the workspace and the record must be 16-byte aligned", fn);
  DL3P_CHECK_ARG(P >= 1 && P < ((size_t)1 << 31), "%s: P = %zu must lie in [1, 2^31)", fn, P);
  DL3P_CHECK_ARG(top_k_percent > 0.0 && top_k_percent <= 1.0 && mining_step >= 0,
                 "%s: top_k_percent = %g must lie in (0, 1], mining_step = %d must be >= 0", fn, top_k_percent, mining_step);
  hipStream_t st = (hipStream_t)stream;
  unsigned* ws = (unsigned*)workspace;
  const unsigned blocks = (unsigned)stream_blocks((long long)P);
  for (int pass = 0; pass < 4; ++pass) {
    if (pass > 0 || !first_histogram_ready)
      hipLaunchKernelGGL(mining_hist_kernel, dim3(blocks), dim3(256), 0, st, loss_map, (long long)P, ws, pass);
    hipLaunchKernelGGL(mining_scan_kernel, dim3(1), dim3(256), 0, st, ws, (unsigned*)record, pass, (long long)P, top_k_percent, mining_step,
                       (const long long*)step_counter, step_bias);
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_mining_weights(const float* loss_map, const float* base, const void* record, float* weights, size_t P,
                                   void* stream) {
  const char* fn = "dl3p_mining_weights";
  DL3P_CHECK_ARG(loss_map && aligned16(loss_map) && weights && aligned16(weights) && record && aligned16(record) &&
                 aligned16(base), "%s: the loss map, the base weights, the record and the weights must be 16-byte aligned", fn);
  DL3P_CHECK_ARG(P >= 1 && P < ((size_t)1 << 31), "%s: P = %zu must lie in [1, 2^31)", fn, P);
  hipLaunchKernelGGL(mining_weights_kernel, dim3((unsigned)stream_blocks((long long)P)), dim3(256), 0, (hipStream_t)stream, loss_map, base,
                     (const unsigned*)record, weights, (long long)P);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
