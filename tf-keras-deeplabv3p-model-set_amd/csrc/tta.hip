// Multi-scale / mirrored evaluation head for gfx950: one pass's (or one scale's plain and mirrored pass's) low-resolution
// logits are upsampled to the base resolution, turned into class probabilities and added, weighted, into ONE running
// (N,H,W,ld) fp32 sum; the launch that adds the last pass skips the write and goes straight to argmax + confusion counts.
// No per-pass probability tensor exists.  The protocol (several input scales and the mirrored image, probabilities
// averaged before the argmax) is DeepLab's evaluation protocol; the reference repository has no counterpart.
//
// Arithmetic per output pixel, head_kernel's through the same calls (head_common.h): half-pixel bilinear gather of the four
// neighbour logit rows in float32, softmax with the hardware exp of the max-shifted logits, p = e * (1 / sum).  The
// mirrored map contributes the probabilities of ITS column W - 1 - x at column x.  The sum is
//   acc = (acc + weight * p_plain) + weight * p_mirror          (-ffp-contract=off: two roundings per term)
// so one paired launch is, bit for bit, a plain-only launch followed by a mirror-only one.
// HBM-bound: the acc read and write are the traffic (the logits are small and stay in L2); 16-byte accesses on acc, one
// thread per output pixel, no floating-point atomics.  The confusion counters are integers: a workgroup-private LDS
// histogram (C <= 64) flushed with 64-bit atomics, as in argmax_confusion_kernel.
#include "head_common.h"

struct TtaParams {
  const float* z; int ldz; const float* zm; int ldzm;
  int h, w; float weight;
  const float* acc_in; float* acc_out; int ld_acc;
  const float* labels; int* pred; unsigned long long* cm;
  int N, C, H, W;
  long long total;
};

// a[c] += weight * softmax(upsampled logits)[c] for a class vector held in registers
template <int CP>
__device__ __forceinline__ void tta_add_pass(float (&a)[CP], const Taps& t, int C, float weight) {
  float v[CP];
  tap_logits<CP>(v, t);
  const float inv = softmax_exp<CP>(v, C);
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float pr = v[c] * inv;
    a[c] = a[c] + weight * pr;
  }
}

// up to 32 classes: a pixel's class vector (the running sum) stays in registers; CP = C rounded up to a multiple of 4
template <int CP>
__global__ __launch_bounds__(256) void tta_accumulate_kernel(TtaParams p) {
  extern __shared__ unsigned int tta_hist[];               // [C][C], only with a confusion matrix
  const ConfusionHist cm = confusion_begin(tta_hist, p.cm, p.C, p.cm != nullptr);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
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
    if (p.z) tta_add_pass<CP>(a, Taps(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W), p.C, p.weight);
    if (p.zm) tta_add_pass<CP>(a, Taps(p.zm, p.ldzm, n, oy, p.W - 1 - ox, p.h, p.w, p.H, p.W), p.C, p.weight);
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
      if (p.cm) cm.count((int)p.labels[s], arg);
    }
  }
  cm.flush();
}

// More than 32 classes: a thread walks the classes of its pixel three times per map (softmax_walk: maximum, sum of exponentials,
// then four classes of the sum at a time).
__global__ __launch_bounds__(256) void tta_accumulate_big(TtaParams p) {
  extern __shared__ unsigned int tta_hist[];               // [C][C], only with a confusion matrix and C <= 64
  const ConfusionHist cm = confusion_begin(tta_hist, p.cm, p.C, p.cm != nullptr && p.C <= 64);
  const int cp = (p.C + 3) / 4 * 4;
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    int ox, oy;
    long long n;
    pixel_of(s, p.W, p.H, &ox, &oy, &n);
    SoftmaxWalk kp = {}, km = {};
    if (p.z) kp = softmax_walk(Taps(p.z, p.ldz, n, oy, ox, p.h, p.w, p.H, p.W), p.C);
    if (p.zm) km = softmax_walk(Taps(p.zm, p.ldzm, n, oy, p.W - 1 - ox, p.h, p.w, p.H, p.W), p.C);
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
          if (p.z) { const float pr = kp.prob(c); a[i] = a[i] + p.weight * pr; }
          if (p.zm) { const float pr = km.prob(c); a[i] = a[i] + p.weight * pr; }
          if (c == 0 || a[i] > best) { best = a[i]; arg = c; }      // first index on ties
        } else {
          a[i] = 0.f;
        }
      }
      if (p.acc_out) st4(p.acc_out + (size_t)s * p.ld_acc + c0, make_float4(a[0], a[1], a[2], a[3]));
    }
    if (p.pred) p.pred[s] = arg;
    if (p.cm) cm.count((int)p.labels[s], arg);
  }
  cm.flush();
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
