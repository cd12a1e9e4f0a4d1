// What the prediction-head kernels share (resize_head.hip, nearest_head.hip, mining.hip, tta.hip) and what the resize kernels share
// with them (bf16_ew.hip, dwconv.hip): the half-pixel bilinear rule, the softmax of a pixel's class vector, the label rule, the
// per-pixel loss term and the integer histograms.  The kernels promise each other's bits (predict + a host argmax gives
// evaluate_miou's class, one TTA pass is the softmax of the resize, the loss map's value is the head's loss at that pixel, the folded
// decoder resize equals the unfolded pair); they keep that promise by calling the same expression.  The build uses
// -ffp-contract=off: the order of operations written here is the contract.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------ bilinear rule
// TF's half-pixel source coordinate in float32 (tf.image.resize(method='bilinear')), op for op:
//   scale = in/out; src = (o + 0.5f)*scale - 0.5f; lo = max(floor(src),0); hi = min(ceil(src),in-1); t = src - floor(src)
struct Lerp { int lo, hi; float t; };
__host__ __device__ __forceinline__ Lerp lerp_coeff(int o, float scale, int in_size) {
  const float src = ((float)o + 0.5f) * scale - 0.5f;
  const float fl = floorf(src);
  Lerp r;
  r.lo = max((int)fl, 0);
  r.hi = min((int)ceilf(src), in_size - 1);
  r.t = src - fl;
  return r;
}

// TF: top = tl + (tr-tl)*tx; bottom = bl + (br-bl)*tx; out = top + (bottom-top)*ty
__device__ __forceinline__ float lerp2(float tl, float tr, float bl, float br, float tx, float ty) {
  const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
  return top + (bot - top) * ty;
}
__device__ __forceinline__ float4 lerp2(float4 tl, float4 tr, float4 bl, float4 br, float tx, float ty) {
  return make_float4(lerp2(tl.x, tr.x, bl.x, br.x, tx, ty), lerp2(tl.y, tr.y, bl.y, br.y, tx, ty),
                     lerp2(tl.z, tr.z, bl.z, br.z, tx, ty), lerp2(tl.w, tr.w, bl.w, br.w, tx, ty));
}

// flat index over (n, h, w) -> x, y, n
__device__ __forceinline__ void pixel_of(long long s, int w, int h, int* x, int* y, long long* n) {
  *x = (int)(s % w);
  const long long t = s / w;
  *y = (int)(t % h);
  *n = t / h;
}

// the four neighbour rows of output pixel (n, oy, ox) of an H x W map in a (N,h,w,ld) logit map, and the two interpolation weights
struct Taps {
  const float *tl, *tr, *bl, *br;
  float tx, ty;
  Taps() = default;
  __device__ __forceinline__ Taps(const float* z, int ld, size_t n, int oy, int ox, int h, int w, int H, int W) {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const Lerp ly = lerp_coeff(oy, sy, h), lx = lerp_coeff(ox, sx, w);
    const float* img = z + n * h * w * ld;
    tl = img + ((size_t)ly.lo * w + lx.lo) * ld;
    tr = img + ((size_t)ly.lo * w + lx.hi) * ld;
    bl = img + ((size_t)ly.hi * w + lx.lo) * ld;
    br = img + ((size_t)ly.hi * w + lx.hi) * ld;
    tx = lx.t; ty = ly.t;
  }
};
__device__ __forceinline__ float tap_logit(const Taps& t, int c) { return lerp2(t.tl[c], t.tr[c], t.bl[c], t.br[c], t.tx, t.ty); }
// the classes [4 c4, 4 c4 + 4) of the pixel with 16-byte loads (rows 16-byte aligned), and its padded class vector in registers
__device__ __forceinline__ float4 tap_logits4(const Taps& t, int c4) {
  return lerp2(ld4(t.tl + c4 * 4), ld4(t.tr + c4 * 4), ld4(t.bl + c4 * 4), ld4(t.br + c4 * 4), t.tx, t.ty);
}
template <int CP>
__device__ __forceinline__ void tap_logits(float (&v)[CP], const Taps& t) {
#pragma unroll
  for (int c4 = 0; c4 < CP / 4; ++c4) {
    const float4 o = tap_logits4(t, c4);
    v[c4 * 4] = o.x; v[c4 * 4 + 1] = o.y; v[c4 * 4 + 2] = o.z; v[c4 * 4 + 3] = o.w;
  }
}
// first maximum over the classes, like np.argmax: four classes at a time (the vector is never whole in registers), and class by
// class for more than 32 classes
template <int CP>
__device__ __forceinline__ int argmax_taps(const Taps& t, int C) {
  float best = -3.0e38f;
  int arg = 0;
#pragma unroll
  for (int c4 = 0; c4 < CP / 4; ++c4) {
    const float4 o = tap_logits4(t, c4);
    const float v[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) if (c4 * 4 + i < C && v[i] > best) { best = v[i]; arg = c4 * 4 + i; }
  }
  return arg;
}
__device__ __forceinline__ int argmax_walk(const Taps& t, int C) {
  float best = -3.0e38f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float v = tap_logit(t, c);
    if (v > best) { best = v; arg = c; }
  }
  return arg;
}

// ------------------------------------------------------------------------------ softmax
// exp of the max-shifted logits is the hardware v_exp_f32 (1 ulp on the [-87, 0] arguments a softmax sees); the
// full-range expf costs ~25 instructions x 21 classes per pixel and made the head kernels VALU-bound.
// In registers: v becomes the exponentials (0 for classes >= C); returns 1 / their sum, p_c = v[c] * that
template <int CP>
__device__ __forceinline__ float softmax_exp(float (&v)[CP], int C) {
  float mx = -3.0e38f;
#pragma unroll
  for (int c = 0; c < CP; ++c) if (c < C) mx = fmaxf(mx, v[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    v[c] = c < C ? __expf(v[c] - mx) : 0.f;
    sum += v[c];
  }
  return 1.f / sum;
}
// More than 32 classes (the reference allows up to 253: train.py:34): a pixel's class vector no longer fits registers.  The classes
// are walked three times (maximum, sum of exponentials, then whatever reads the probabilities), re-interpolating each logit from
// its four neighbours (L1 / L2 hits): the arithmetic of softmax_exp, class by class.
struct SoftmaxWalk {
  Taps t;
  float mx, inv;
  __device__ __forceinline__ float exp_of(float logit) const { return __expf(logit - mx); }
  __device__ __forceinline__ float prob(int c) const { return exp_of(tap_logit(t, c)) * inv; }
};
__device__ __forceinline__ SoftmaxWalk softmax_walk(const Taps& t, int C) {
  SoftmaxWalk k;
  k.t = t;
  k.mx = -3.0e38f;
  for (int c = 0; c < C; ++c) k.mx = fmaxf(k.mx, tap_logit(t, c));
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += k.exp_of(tap_logit(t, c));
  k.inv = 1.f / sum;
  return k;
}

// across a wave that owns one logit vector: lane l holds the classes [4 l, 4 l + 4) (256 classes at most)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// softmax of the logit vector at zp over the wave: this lane's four probabilities (0 for classes >= C)
__device__ __forceinline__ float4 wave_softmax(const float* zp, int lane, int C, int cp) {
  const int c0 = lane * 4;
  float4 v = make_float4(-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f);
  if (c0 < cp) v = ld4(zp + c0);
  const bool i0 = c0 < C, i1 = c0 + 1 < C, i2 = c0 + 2 < C, i3 = c0 + 3 < C;
  float mx = fmaxf(fmaxf(i0 ? v.x : -3.0e38f, i1 ? v.y : -3.0e38f), fmaxf(i2 ? v.z : -3.0e38f, i3 ? v.w : -3.0e38f));
  mx = wave_max(mx);
  const float4 e = make_float4(i0 ? __expf(v.x - mx) : 0.f, i1 ? __expf(v.y - mx) : 0.f, i2 ? __expf(v.z - mx) : 0.f,
                               i3 ? __expf(v.w - mx) : 0.f);
  const float inv = 1.f / wave_sum((e.x + e.y) + (e.z + e.w));
  return make_float4(e.x * inv, e.y * inv, e.z * inv, e.w * inv);
}
// the label's probability in such a wave: component lab & 3 of the lane lab >> 2; 1 for a pixel that does not count
__device__ __forceinline__ float wave_label_prob(float4 pr, bool valid, int lab) {
  const int src = valid ? (lab >> 2) : 0;
  const float q0 = __shfl(pr.x, src), q1 = __shfl(pr.y, src), q2 = __shfl(pr.z, src), q3 = __shfl(pr.w, src);
  const int comp = lab & 3;
  return valid ? (comp == 0 ? q0 : comp == 1 ? q1 : comp == 2 ? q2 : q3) : 1.f;
}

// ------------------------------------------------------------------------------ labels and the per-pixel loss
// a pixel counts towards the loss when its label is a class and is not the ignored one
__device__ __forceinline__ bool label_valid(int lab, int ignore_index, int C) {
  const bool masked = ignore_index != 0 && lab == ignore_index;   // loss.py:139 truthiness
  return !masked && lab >= 0 && lab < C;
}

// cross entropy of the reference (loss.py:121-156): p_t clipped to [1e-7, 1 - 1e-7], no gradient outside the clip range
__device__ __forceinline__ bool ce_unclipped(float pt) { return pt > 1e-7f && pt < 1.f - 1e-7f; }
__device__ __forceinline__ float ce_loss(float pt) { return -logf(fminf(fmaxf(pt, 1e-7f), 1.f - 1e-7f)); }

// per-pixel loss l(p_t) and the factor f with d l / d z_c = f * (p_c - [c == y]):
//   cross entropy (loss.py:121-156)   l = -log(clip(p_t, 1e-7, 1 - 1e-7)),  f = 1 inside the clip range, else 0
//   class-weighted  (loss.py:159-191) l = -w_y log(p_t)  (no clipping),      f = w_y
//   focal           (loss.py:63-118)  l = -alpha (1 - p_t)^gamma log(p_t),   p_t clipped to [1e-15, 1 - 1e-15];
//                                     f = alpha ((1 - p_t)^gamma - gamma (1 - p_t)^(gamma - 1) p_t log p_t)
// Neither is multiplied by a pixel weight, and the caller leaves an invalid pixel out of its sums.
__device__ __forceinline__ void loss_term(int kind, float pt, bool valid, int lab, const float* class_w, float gamma, float alpha,
                                          float* l, float* f) {
  if (kind == DL3P_LOSS_WEIGHTED_CE) {
    float wy = 0.f;
    if (valid) wy = class_w[lab];
    *l = -wy * logf(pt);
    *f = wy;
  } else if (kind == DL3P_LOSS_FOCAL) {
    const float pc = fmaxf(pt, 1e-15f);               // 1 - 1e-15 rounds to 1 in fp32: the upper clip is a no-op
    const float om = 1.f - pc, lp = logf(pc);
    const float pw1 = om > 0.f ? powf(om, gamma - 1.f) : (gamma == 1.f ? 1.f : 0.f);
    const float pw = pw1 * om;
    *l = -alpha * pw * lp;
    *f = pt >= 1e-15f ? alpha * (pw - gamma * pw1 * pc * lp) : 0.f;
  } else {
    *l = ce_loss(pt);
    *f = ce_unclipped(pt) ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------ integer histograms
// Counts are integers: a workgroup-private LDS histogram flushed with integer atomics gives the same result in any order.
// confusion[label][prediction] for labels in [0, C): LDS bins [C][C] where the caller has them (lds), else 64-bit atomics on cm
struct ConfusionHist {
  unsigned int* hist;
  unsigned long long* cm;
  int C;
  bool lds;
  __device__ __forceinline__ void count(int lab, int arg) const {
    if (lab >= 0 && lab < C) {
      if (lds) atomicAdd(&hist[lab * C + arg], 1u);
      else atomicAdd(&cm[(size_t)lab * C + arg], 1ull);
    }
  }
  __device__ __forceinline__ void flush() const {      // every thread of the workgroup (256)
    if (lds) {
      __syncthreads();
      for (int i = threadIdx.x; i < C * C; i += 256)
        if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
    }
  }
};
__device__ __forceinline__ ConfusionHist confusion_begin(unsigned int* hist, unsigned long long* cm, int C, bool lds) {
  if (lds) {
    for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0u;
    __syncthreads();
  }
  return ConfusionHist{hist, cm, C, lds};
}

// one image's [3][C] counts: |label == c & pred == c|, |label == c|, |pred == c| (see dl3p_class_counts), LDS bins [3][C]
struct ClassCountHist {
  unsigned int* hist;
  int C;
  __device__ __forceinline__ void predicted(int arg, unsigned int pixels) const { atomicAdd(&hist[2 * C + arg], pixels); }
  __device__ __forceinline__ void labelled(int lab, int arg) const {
    if (lab >= 0 && lab < C) {
      atomicAdd(&hist[C + lab], 1u);
      if (lab == arg) atomicAdd(&hist[lab], 1u);
    }
  }
  __device__ __forceinline__ void flush(int* counts) const {      // counts: the image's [3][C]
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C; i += 256)
      if (hist[i]) atomicAdd(&counts[i], (int)hist[i]);
  }
};
__device__ __forceinline__ ClassCountHist class_counts_begin(unsigned int* hist, int C) {
  for (int i = threadIdx.x; i < 3 * C; i += 256) hist[i] = 0u;
  __syncthreads();
  return ClassCountHist{hist, C};
}
