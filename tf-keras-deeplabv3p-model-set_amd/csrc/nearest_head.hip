// The head behind a nearest UpSampling2D((r, r)) (fast_scnn/models/fast_scnn.py:143-149): the r x r pixels of a block share ONE logit
// vector, so one softmax per logit pixel serves the whole block and the gradient of that vector is the sum over the block's labels.
// A wave owns a logit pixel: lane l holds the classes [4 l, 4 l + 4) (256 classes at most) and, in the training kernel, the label
// k = l of the block (r * r <= 64).  Per-pixel loss definitions, clipping constants and masking are loss_term's and
// label_valid's (csrc/head_common.h).  Every sum has a fixed order: graph replay equals eager bit for bit.
#include "head_common.h"

namespace {

struct NHeadParams {
  const float* z; int ldz; const float* labels; int ignore_index; float inv_count;
  int loss_kind; const float* class_w; float focal_gamma, focal_alpha; const float* pixel_w;
  float* probs; float* gz; int ldgz; int accumulate; float* loss_partials;
  int h, w, C, H, W, r, cp;
  long long total;                   // N * h * w logit pixels
};

// ------------------------------------------------------------------------------ loss and d loss / d z
__global__ __launch_bounds__(256) void nearest_head_train_kernel(NHeadParams p) {
  __shared__ float wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rr = p.r * p.r;
  const int li = lane / p.r, lj = lane - li * p.r;          // this lane's label inside the block
  const int c0 = lane * 4;
  float loss = 0.f;
  for (long long s = (long long)blockIdx.x * 4 + wave; s < p.total; s += (long long)gridDim.x * 4) {   // wave-uniform
    int x, y;
    long long n;
    pixel_of(s, p.w, p.h, &x, &y, &n);
    const float4 pr = wave_softmax(p.z + (size_t)s * p.ldz, lane, p.C, p.cp);
    int lab = -1;
    float swt = 1.f;
    if (lane < rr) {
      const size_t f = ((size_t)n * p.H + (size_t)y * p.r + li) * p.W + (size_t)x * p.r + lj;
      lab = (int)p.labels[f];
      if (p.pixel_w) swt = p.pixel_w[f];
    }
    const bool valid = lane < rr && label_valid(lab, p.ignore_index, p.C);
    if (!valid) lab = -1;
    const float pt = wave_label_prob(pr, valid, lab);
    float l, f;
    loss_term(p.loss_kind, pt, valid, lab, p.class_w, p.focal_gamma, p.focal_alpha, &l, &f);
    l *= swt;
    f *= swt;
    loss += wave_sum(valid ? l : 0.f);
    if (p.gz) {
      // d/dz_c = sum_k gs_k (p_c - [c == y_k]) = (sum_k gs_k) p_c - sum_k gs_k [c == y_k], k in block order
      const float gs = valid ? f * p.inv_count : 0.f;
      float G = 0.f;
      float4 hit = zero4();
      for (int k = 0; k < rr; ++k) {
        const float gk = __shfl(gs, k);
        const int lk = __shfl(lab, k);
        G += gk;
        hit.x += lk == c0 ? gk : 0.f;
        hit.y += lk == c0 + 1 ? gk : 0.f;
        hit.z += lk == c0 + 2 ? gk : 0.f;
        hit.w += lk == c0 + 3 ? gk : 0.f;
      }
      if (c0 < p.cp) {
        float4 d = make_float4(c0 < p.C ? G * pr.x - hit.x : 0.f, c0 + 1 < p.C ? G * pr.y - hit.y : 0.f,
                               c0 + 2 < p.C ? G * pr.z - hit.z : 0.f, c0 + 3 < p.C ? G * pr.w - hit.w : 0.f);
        float* o = p.gz + (size_t)s * p.ldgz + c0;
        if (p.accumulate) d = add4(d, ld4(o));
        st4(o, d);
      }
    }
  }
  if (lane == 0) wsum[wave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) p.loss_partials[blockIdx.x] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * p.inv_count;
}

// ------------------------------------------------------------------------------ probabilities (predict)
// the r pixels of a block row are r * C contiguous floats of the compact (N,H,W,C) output: the wave writes them as one run
__global__ __launch_bounds__(256) void nearest_probs_kernel(NHeadParams p) {
  __shared__ __attribute__((aligned(16))) float ps[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long base = (long long)blockIdx.x * 4; base < p.total; base += (long long)gridDim.x * 4) {   // workgroup-uniform
    const bool live = base + wave < p.total;
    const long long s = live ? base + wave : p.total - 1;
    int x, y;
    long long n;
    pixel_of(s, p.w, p.h, &x, &y, &n);
    const float4 pr = wave_softmax(p.z + (size_t)s * p.ldz, lane, p.C, p.cp);
    __syncthreads();
    *reinterpret_cast<float4*>(&ps[wave][lane * 4]) = pr;
    __syncthreads();
    if (live) {
      const int run = p.r * p.C;
      for (int i = 0; i < p.r; ++i) {
        float* row = p.probs + (((size_t)n * p.H + (size_t)y * p.r + i) * p.W + (size_t)x * p.r) * p.C;
        for (int e = lane; e < run; e += 64) row[e] = ps[wave][e % p.C];
      }
    }
  }
}

// ------------------------------------------------------------------------------ argmax, confusion matrix, class counts
struct NEvalParams {
  const float* z; int ldz; const float* labels; int* pred; unsigned long long* cm;
  int h, w, C, H, W, r, cp;
  long long total;
};

// first maximum over the classes, like np.argmax
__device__ __forceinline__ int argmax_of(const float* zp, int C, int cp) {
  float best = -3.0e38f;
  int arg = 0;
  for (int c = 0; c < cp; c += 4) {
    const float4 v = ld4(zp + c);
    if (v.x > best) { best = v.x; arg = c; }
    if (c + 1 < C && v.y > best) { best = v.y; arg = c + 1; }
    if (c + 2 < C && v.z > best) { best = v.z; arg = c + 2; }
    if (c + 3 < C && v.w > best) { best = v.w; arg = c + 3; }
  }
  return arg;
}

// one thread per logit pixel; integer counts (LDS histogram for C <= 64, 64-bit atomics otherwise): any order gives the same matrix
__global__ __launch_bounds__(256) void nearest_argmax_confusion_kernel(NEvalParams p) {
  extern __shared__ unsigned int hist[];                 // [C][C], only with labels and C <= 64
  const ConfusionHist cm = confusion_begin(hist, p.cm, p.C, p.labels && p.cm && p.C <= 64);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    int x, y;
    long long n;
    pixel_of(s, p.w, p.h, &x, &y, &n);
    const int arg = argmax_of(p.z + (size_t)s * p.ldz, p.C, p.cp);
    for (int i = 0; i < p.r; ++i)
      for (int j = 0; j < p.r; ++j) {
        const size_t f = ((size_t)n * p.H + (size_t)y * p.r + i) * p.W + (size_t)x * p.r + j;
        if (p.pred) p.pred[f] = arg;
        if (p.labels && p.cm) cm.count((int)p.labels[f], arg);
      }
  }
  cm.flush();
}

// counts[n][3][C] (see dl3p_class_counts): workgroups stay inside one image and keep an LDS histogram
__global__ __launch_bounds__(256) void nearest_class_counts_kernel(NEvalParams p, int* counts, int blocks_per_image) {
  extern __shared__ unsigned int hist[];                 // [3][C]
  const ClassCountHist cc = class_counts_begin(hist, p.C);
  const int n = blockIdx.x / blocks_per_image, b = blockIdx.x - n * blocks_per_image;
  const int hw = p.h * p.w;
  for (int s = b * 256 + threadIdx.x; s < hw; s += blocks_per_image * 256) {
    const int x = s % p.w, y = s / p.w;
    const int arg = argmax_of(p.z + ((size_t)n * hw + s) * p.ldz, p.C, p.cp);
    cc.predicted(arg, (unsigned int)(p.r * p.r));
    for (int i = 0; i < p.r; ++i)
      for (int j = 0; j < p.r; ++j)
        cc.labelled((int)p.labels[((size_t)n * p.H + (size_t)y * p.r + i) * p.W + (size_t)x * p.r + j], arg);
  }
  cc.flush(counts + (size_t)n * 3 * p.C);
}

// the scale r with (H, W) = r (h, w), or 0
int scale_of(int h, int w, int H, int W) {
  if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || H % h || W % w || H / h != W / w) return 0;
  return H / h;
}

int check_head(const char* fn, const float* z, int ldz, int N, int h, int w, int C, int H, int W, int* r) {
  DL3P_CHECK_ARG(z && aligned16(z) && ldz % 4 == 0, "%s: logits must be 16-byte aligned, ld %% 4 == 0", fn);
  DL3P_CHECK_ARG(C > 0 && C <= 256 && ldz >= (C + 3) / 4 * 4, "%s: C=%d (ld=%d) unsupported", fn, C, ldz);
  *r = scale_of(h, w, H, W);
  DL3P_CHECK_ARG(N > 0 && *r >= 1 && *r <= 8, "%s: (H, W) = (%d, %d) must be r in 1..8 times (h, w) = (%d, %d)", fn, H, W, h, w);
  return DL3P_OK;
}

}  // namespace

extern "C" int dl3p_nearest_softmax_probs(const float* z, int ldz, float* probs, int N, int h, int w, int C, int H, int W,
                                          void* stream) {
  const char* fn = "dl3p_nearest_softmax_probs";
  int r;
  const int rc = check_head(fn, z, ldz, N, h, w, C, H, W, &r);
  if (rc) return rc;
  DL3P_CHECK_ARG(probs != nullptr, "%s: probs is null", fn);
  NHeadParams p = {};
  p.z = z; p.ldz = ldz; p.probs = probs;
  p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.r = r; p.cp = (C + 3) / 4 * 4;
  p.total = (long long)N * h * w;
  long long blocks = ceil_div_ll(p.total, 4);
  const long long cap = (long long)DL3P_NUM_CUS * 16;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(nearest_probs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_nearest_head_train(const float* z, int ldz, const float* labels, int ignore_index, float inv_count,
                                       int loss_kind, const float* class_weights, float focal_gamma, float focal_alpha,
                                       const float* pixel_weights, float* gz, int ldgz, int accumulate, float* loss_partials,
                                       int* rows_out, int N, int h, int w, int C, int H, int W, void* stream) {
  const char* fn = "dl3p_nearest_head_train";
  int r;
  const int rc = check_head(fn, z, ldz, N, h, w, C, H, W, &r);
  if (rc) return rc;
  DL3P_CHECK_ARG(loss_kind == DL3P_LOSS_CE || loss_kind == DL3P_LOSS_FOCAL || (loss_kind == DL3P_LOSS_WEIGHTED_CE && class_weights),
                 "%s: bad loss kind %d (weighted CE needs class_weights[C])", fn, loss_kind);
  DL3P_CHECK_ARG(labels && loss_partials, "%s: labels and loss_partials are required", fn);
  DL3P_CHECK_ARG(!gz || (aligned16(gz) && ldgz % 4 == 0 && ldgz >= (C + 3) / 4 * 4), "%s: bad gradient layout (ld=%d)", fn, ldgz);
  NHeadParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels; p.ignore_index = ignore_index; p.inv_count = inv_count;
  p.loss_kind = loss_kind; p.class_w = class_weights; p.focal_gamma = focal_gamma; p.focal_alpha = focal_alpha;
  p.pixel_w = pixel_weights; p.gz = gz; p.ldgz = ldgz; p.accumulate = accumulate; p.loss_partials = loss_partials;
  p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.r = r; p.cp = (C + 3) / 4 * 4;
  p.total = (long long)N * h * w;
  long long blocks = ceil_div_ll(p.total, 4);
  if (blocks > DL3P_MAX_STAT_ROWS) blocks = DL3P_MAX_STAT_ROWS;
  if (rows_out) *rows_out = (int)blocks;
  hipLaunchKernelGGL(nearest_head_train_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_nearest_argmax_confusion(const float* z, int ldz, const float* labels, int32_t* pred_mask,
                                             unsigned long long* confusion, int N, int h, int w, int C, int H, int W,
                                             void* stream) {
  const char* fn = "dl3p_nearest_argmax_confusion";
  int r;
  const int rc = check_head(fn, z, ldz, N, h, w, C, H, W, &r);
  if (rc) return rc;
  DL3P_CHECK_ARG(pred_mask || (labels && confusion), "%s: nothing to produce", fn);
  DL3P_CHECK_ARG(!confusion || labels, "%s: a confusion matrix needs labels", fn);
  NEvalParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels; p.pred = pred_mask; p.cm = confusion;
  p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.r = r; p.cp = (C + 3) / 4 * 4;
  p.total = (long long)N * h * w;
  long long blocks = ceil_div_ll(p.total, 256);
  if (blocks > 4096) blocks = 4096;
  const size_t lds = (labels && confusion && C <= 64) ? (size_t)C * C * sizeof(unsigned int) : 0;
  hipLaunchKernelGGL(nearest_argmax_confusion_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_nearest_class_counts(const float* z, int ldz, const float* labels, int32_t* counts, int N, int h, int w,
                                         int C, int H, int W, void* stream) {
  const char* fn = "dl3p_nearest_class_counts";
  int r;
  const int rc = check_head(fn, z, ldz, N, h, w, C, H, W, &r);
  if (rc) return rc;
  DL3P_CHECK_ARG(labels && counts, "%s: labels and counts are required", fn);
  NEvalParams p = {};
  p.z = z; p.ldz = ldz; p.labels = labels;
  p.h = h; p.w = w; p.C = C; p.H = H; p.W = W; p.r = r; p.cp = (C + 3) / 4 * 4;
  int bpi = (h * w + 255) / 256;
  if (bpi > 256) bpi = 256;
  hipLaunchKernelGGL(nearest_class_counts_kernel, dim3((unsigned)(N * bpi)), dim3(256), (size_t)3 * C * sizeof(unsigned int),
                     (hipStream_t)stream, p, counts, bpi);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
