// Multi-scale / mirrored evaluation head for gfx950: one pass's (or one scale's plain and mirrored pass's) low-resolution
// logits are upsampled to the base resolution, turned into class probabilities and added, weighted, into ONE running
// (N,H,W,ld) fp32 sum; the launch that adds the last pass skips the write and goes straight to argmax + confusion counts.
// No per-pass probability tensor exists.  The protocol (several input scales and the mirrored image, probabilities
// averaged before the argmax) is DeepLab's evaluation protocol; the reference repository has no counterpart.
//
// Arithmetic per output pixel, op for op that of head_kernel (resize_head.hip): half-pixel bilinear gather of the four
// neighbour logit rows in float32, softmax with the hardware exp of the max-shifted logits, p = e * (1 / sum).  The
// mirrored map contributes the probabilities of ITS column W - 1 - x at column x.  The sum is
//   acc = (acc + weight * p_plain) + weight * p_mirror          (-ffp-contract=off: two roundings per term)
// so one paired launch is, bit for bit, a plain-only launch followed by a mirror-only one.
// HBM-bound: the acc read and write are the traffic (the logits are small and stay in L2); 16-byte accesses on acc, one
// thread per output pixel, no floating-point atomics.  The confusion counters are integers: a workgroup-private LDS
// histogram (C <= 64) flushed with 64-bit atomics, as in argmax_confusion_kernel.
#include "common.h"

struct TtaLerp { int lo, hi; float t; };
__device__ __forceinline__ TtaLerp tta_lerp(int o, float scale, int in_size) {      // = lerp_coeff of resize_head.hip
  const float src = ((float)o + 0.5f) * scale - 0.5f;
  const float fl = floorf(src);
  TtaLerp r;
  r.lo = max((int)fl, 0);
  r.hi = min((int)ceilf(src), in_size - 1);
  r.t = src - fl;
  return r;
}

struct TtaParams {
  const float* z; int ldz; const float* zm; int ldzm;
  int h, w; float weight;
  const float* acc_in; float* acc_out; int ld_acc;
  const float* labels; int* pred; unsigned long long* cm;
  int N, C, H, W;
  long long total;
};

// the four neighbour rows of output pixel (n, oy, ox) in a (N,h,w,ld) logit map, and the two interpolation weights
struct TtaTaps { const float *tl, *tr, *bl, *br; float tx, ty; };
__device__ __forceinline__ TtaTaps tta_taps(const float* z, int ld, int n, int oy, int ox, const TtaParams& p) {
  const float sy = (float)p.h / (float)p.H, sx = (float)p.w / (float)p.W;
  const TtaLerp ly = tta_lerp(oy, sy, p.h), lx = tta_lerp(ox, sx, p.w);
  const float* img = z + (size_t)n * p.h * p.w * ld;
  TtaTaps t;
  t.tl = img + ((size_t)ly.lo * p.w + lx.lo) * ld;
  t.tr = img + ((size_t)ly.lo * p.w + lx.hi) * ld;
  t.bl = img + ((size_t)ly.hi * p.w + lx.lo) * ld;
  t.br = img + ((size_t)ly.hi * p.w + lx.hi) * ld;
  t.tx = lx.t; t.ty = ly.t;
  return t;
}
__device__ __forceinline__ float tta_lerp2(float tl, float tr, float bl, float br, float tx, float ty) {
  const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
  return top + (bot - top) * ty;
}

// a[c] += weight * softmax(upsampled logits)[c] for a class vector held in registers
template <int CP>
__device__ __forceinline__ void tta_add_pass(float (&a)[CP], const TtaTaps& t, int C, float weight) {
  float v[CP];
#pragma unroll
  for (int c4 = 0; c4 < CP / 4; ++c4) {
    const float4 tl = ld4(t.tl + c4 * 4), tr = ld4(t.tr + c4 * 4), bl = ld4(t.bl + c4 * 4), br = ld4(t.br + c4 * 4);
    v[c4 * 4 + 0] = tta_lerp2(tl.x, tr.x, bl.x, br.x, t.tx, t.ty);
    v[c4 * 4 + 1] = tta_lerp2(tl.y, tr.y, bl.y, br.y, t.tx, t.ty);
    v[c4 * 4 + 2] = tta_lerp2(tl.z, tr.z, bl.z, br.z, t.tx, t.ty);
    v[c4 * 4 + 3] = tta_lerp2(tl.w, tr.w, bl.w, br.w, t.tx, t.ty);
  }
  float mx = -3.0e38f;
#pragma unroll
  for (int c = 0; c < CP; ++c) if (c < C) mx = fmaxf(mx, v[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    v[c] = c < C ? __expf(v[c] - mx) : 0.f;
    sum += v[c];
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float pr = v[c] * inv;
    a[c] = a[c] + weight * pr;
  }
}

// confusion[label][prediction] += 1 for labels in [0, C): into the workgroup's LDS histogram where there is one
__device__ __forceinline__ void tta_count(const TtaParams& p, unsigned int* hist, bool use_lds, long long s, int arg) {
  const int lab = (int)p.labels[s];
  if (lab >= 0 && lab < p.C) {
    if (use_lds) atomicAdd(&hist[lab * p.C + arg], 1u);
    else atomicAdd(&p.cm[(size_t)lab * p.C + arg], 1ull);
  }
}

// up to 32 classes: a pixel's class vector (the running sum) stays in registers; CP = C rounded up to a multiple of 4
template <int CP>
__global__ __launch_bounds__(256) void tta_accumulate_kernel(TtaParams p) {
  extern __shared__ unsigned int tta_hist[];               // [C][C], only with a confusion matrix
  const bool use_lds = p.cm != nullptr;
  if (use_lds) {
    for (int i = threadIdx.x; i < p.C * p.C; i += 256) tta_hist[i] = 0u;
    __syncthreads();
  }
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    const int ox = (int)(s % p.W);
    const long long row = s / p.W;
    const int oy = (int)(row % p.H), n = (int)(row / p.H);
    float a[CP];
    if (p.acc_in) {
      const float* src = p.acc_in + (size_t)s * p.ld_acc;
#pragma unroll
      for (int c4 = 0; c4 < CP / 4; ++c4) {
        const float4 q = ld4(src + c4 * 4);
        a[c4 * 4] = q.x; a[c4 * 4 + 1] = q.y; a[c4 * 4 + 2] = q.z; a[c4 * 4 + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CP; ++c) a[c] = 0.f;
    }
    if (p.z) tta_add_pass<CP>(a, tta_taps(p.z, p.ldz, n, oy, ox, p), p.C, p.weight);
    if (p.zm) tta_add_pass<CP>(a, tta_taps(p.zm, p.ldzm, n, oy, p.W - 1 - ox, p), p.C, p.weight);
    if (p.acc_out) {
      float* dst = p.acc_out + (size_t)s * p.ld_acc;
#pragma unroll
      for (int c4 = 0; c4 < CP / 4; ++c4)        // pad channels leave as 0
        st4(dst + c4 * 4, make_float4(c4 * 4 + 0 < p.C ? a[c4 * 4 + 0] : 0.f, c4 * 4 + 1 < p.C ? a[c4 * 4 + 1] : 0.f,
                                      c4 * 4 + 2 < p.C ? a[c4 * 4 + 2] : 0.f, c4 * 4 + 3 < p.C ? a[c4 * 4 + 3] : 0.f));
    }
    if (p.pred || p.cm) {
      float best = a[0];
      int arg = 0;
#pragma unroll
      for (int c = 1; c < CP; ++c) if (c < p.C && a[c] > best) { best = a[c]; arg = c; }      // first index on ties
      if (p.pred) p.pred[s] = arg;
      if (p.cm) tta_count(p, tta_hist, use_lds, s, arg);
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < p.C * p.C; i += 256)
      if (tta_hist[i]) atomicAdd(&p.cm[i], (unsigned long long)tta_hist[i]);
  }
}

// More than 32 classes: the class vector no longer fits registers.  A thread walks the classes of its pixel three times per
// map (maximum, sum of exponentials, then four classes of the sum at a time), re-interpolating each logit from its four
// neighbours (L1 / L2 hits), like head_kernel_big; same arithmetic per class.
struct TtaWalk { TtaTaps t; float mx, inv; };
__device__ __forceinline__ float tta_logit(const TtaTaps& t, int c) {
  return tta_lerp2(t.tl[c], t.tr[c], t.bl[c], t.br[c], t.tx, t.ty);
}
__device__ __forceinline__ TtaWalk tta_walk(const TtaTaps& t, int C) {
  TtaWalk k;
  k.t = t;
  k.mx = -3.0e38f;
  for (int c = 0; c < C; ++c) k.mx = fmaxf(k.mx, tta_logit(t, c));
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += __expf(tta_logit(t, c) - k.mx);
  k.inv = 1.f / sum;
  return k;
}

__global__ __launch_bounds__(256) void tta_accumulate_big(TtaParams p) {
  extern __shared__ unsigned int tta_hist[];               // [C][C], only with a confusion matrix and C <= 64
  const bool use_lds = p.cm != nullptr && p.C <= 64;
  if (use_lds) {
    for (int i = threadIdx.x; i < p.C * p.C; i += 256) tta_hist[i] = 0u;
    __syncthreads();
  }
  const int cp = (p.C + 3) / 4 * 4;
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    const int ox = (int)(s % p.W);
    const long long row = s / p.W;
    const int oy = (int)(row % p.H), n = (int)(row / p.H);
    TtaWalk kp = {}, km = {};
    if (p.z) kp = tta_walk(tta_taps(p.z, p.ldz, n, oy, ox, p), p.C);
    if (p.zm) km = tta_walk(tta_taps(p.zm, p.ldzm, n, oy, p.W - 1 - ox, p), p.C);
    float best = 0.f;
    int arg = 0;
    for (int c0 = 0; c0 < cp; c0 += 4) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (p.acc_in) {
        const float4 q = ld4(p.acc_in + (size_t)s * p.ld_acc + c0);
        a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c0 + i;
        if (c < p.C) {
          if (p.z) { const float pr = __expf(tta_logit(kp.t, c) - kp.mx) * kp.inv; a[i] = a[i] + p.weight * pr; }
          if (p.zm) { const float pr = __expf(tta_logit(km.t, c) - km.mx) * km.inv; a[i] = a[i] + p.weight * pr; }
          if (c == 0 || a[i] > best) { best = a[i]; arg = c; }      // first index on ties
        } else {
          a[i] = 0.f;
        }
      }
      if (p.acc_out) st4(p.acc_out + (size_t)s * p.ld_acc + c0, make_float4(a[0], a[1], a[2], a[3]));
    }
    if (p.pred) p.pred[s] = arg;
    if (p.cm) tta_count(p, tta_hist, use_lds, s, arg);
  }
  if (use_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < p.C * p.C; i += 256)
      if (tta_hist[i]) atomicAdd(&p.cm[i], (unsigned long long)tta_hist[i]);
  }
}

extern "C" int dl3p_tta_accumulate(const float* z, int ldz, const float* z_mirror, int ldzm, int h, int w, float weight,
                                   const float* acc_in, float* acc_out, int ld_acc, const float* labels,
                                   int32_t* pred_mask, unsigned long long* confusion, int N, int C, int H, int W,
                                   void* stream) {
  const char* fn = "dl3p_tta_accumulate";
  DL3P_CHECK_ARG(C >= 1 && C <= 256, "%s: C=%d is outside [1, 256]", fn, C);
  DL3P_CHECK_ARG(N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "%s: bad dims N=%d h=%d w=%d H=%d W=%d", fn, N, h, w, H, W);
  DL3P_CHECK_ARG(h <= H && w <= W, "%s: the logits (%d x %d) must not be larger than the sum (%d x %d)", fn, h, w, H, W);
  DL3P_CHECK_ARG(z || z_mirror, "%s: needs a plain or a mirrored logit map", fn);
  const int cp = (C + 3) / 4 * 4;
  DL3P_CHECK_ARG(!z || (aligned16(z) && ldz % 4 == 0 && ldz >= cp),
                 "%s: logits must be 16-byte aligned with a stride that is a multiple of 4 and >= C (ldz=%d, C=%d)", fn, ldz, C);
  DL3P_CHECK_ARG(!z_mirror || (aligned16(z_mirror) && ldzm % 4 == 0 && ldzm >= cp),
                 "%s: mirrored logits must be 16-byte aligned with a stride that is a multiple of 4 and >= C (ldzm=%d, C=%d)", fn,
                 ldzm, C);
  DL3P_CHECK_ARG((!acc_in && !acc_out) || (aligned16(acc_in) && aligned16(acc_out) && ld_acc % 4 == 0 && ld_acc >= cp),
                 "%s: the sum must be 16-byte aligned with a stride that is a multiple of 4 and >= C (ld_acc=%d, C=%d)", fn, ld_acc, C);
  DL3P_CHECK_ARG(acc_out || pred_mask || confusion, "%s: nothing to produce", fn);
  DL3P_CHECK_ARG((labels != nullptr) == (confusion != nullptr), "%s: labels and a confusion matrix come together", fn);
  TtaParams p = {};
  p.z = z; p.ldz = ldz; p.zm = z_mirror; p.ldzm = ldzm; p.h = h; p.w = w; p.weight = weight;
  p.acc_in = acc_in; p.acc_out = acc_out; p.ld_acc = ld_acc;
  p.labels = labels; p.pred = pred_mask; p.cm = confusion;
  p.N = N; p.C = C; p.H = H; p.W = W;
  p.total = (long long)N * H * W;
  // a pixel per thread, grid-strided from 8 workgroups per CU: few histogram flushes, and the tail is short
  long long blocks = ceil_div_ll(p.total, 256);
  if (blocks > DL3P_NUM_CUS * 8) blocks = DL3P_NUM_CUS * 8;
  hipStream_t st = (hipStream_t)stream;
  if (C > 32) {
    const size_t lds = (confusion && C <= 64) ? (size_t)C * C * sizeof(unsigned int) : 0;
    hipLaunchKernelGGL(tta_accumulate_big, dim3((unsigned)blocks), dim3(256), lds, st, p);
    DL3P_CHECK_LAUNCH(fn);
    return DL3P_OK;
  }
  const size_t lds = confusion ? (size_t)C * C * sizeof(unsigned int) : 0;
  switch (cp) {
#define DL3P_TTA_CASE(CP) case CP: hipLaunchKernelGGL((tta_accumulate_kernel<CP>), dim3((unsigned)blocks), dim3(256), lds, st, p); break;
    DL3P_TTA_CASE(4) DL3P_TTA_CASE(8) DL3P_TTA_CASE(12) DL3P_TTA_CASE(16) DL3P_TTA_CASE(20) DL3P_TTA_CASE(24) DL3P_TTA_CASE(28)
    DL3P_TTA_CASE(32)
#undef DL3P_TTA_CASE
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
