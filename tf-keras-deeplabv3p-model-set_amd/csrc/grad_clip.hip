// Gradient clipping on the flat gradient buffer: clipvalue, clipnorm, global_clipnorm of the Keras 2.11 legacy OptimizerV2
// (common/model_utils.py:117-123 spells the keywords out on every optimiser), in front of the unchanged optimiser entry points.
//
// The gradient that is clipped is the gradient of the WHOLE Keras loss, g' = fmaf(g, grad_scale, 2 * l2_elem * w) in float32 -- what
// sgd_kernel / adaptive_kernel (bn_elementwise.hip) form themselves when nothing is clipped: grad_scale = 1 / world under data
// parallelism (the caller has all-reduced g), the regulariser included.  Elements with lr_scale_elem == 0 (frozen layers, BatchNorm
// moving statistics, the padding between variables) are not trainable variables: they enter no norm and their g is not written.
//   1. clipvalue c:        g' <- g' < -c ? -c : (g' > c ? c : g')               (a NaN stays a NaN, as tf.clip_by_value leaves it)
//   2. clipnorm c:         per variable v, g' <- g' * s_v,  s_v = c / max(|g'_v|, c)
//   3. global_clipnorm c:  g' <- g' * s,  s = c / max(|g'|, c) over every trainable element of every variable
// in this order; 2 and 3 exclude each other (Keras raises).  Squares are accumulated in float64 (the square of a float32 is exact
// there), the norm, the comparison and the quotient are taken in float64 and the quotient is rounded ONCE to float32.  Consequences:
//   - a norm at or below the threshold gives s == 1.0f exactly (an all-zero or wholly frozen variable: norm 0, s = 1, never 0 / 0);
//   - the max propagates NaN: a NaN norm gives a NaN scale in both modes;
//   - an infinite per-variable norm gives s_v = 0: the finite elements of that variable become 0, the infinite ones inf * 0 = NaN,
//     and no other variable is touched;
//   - a non-finite GLOBAL norm gives s = NaN for every variable (tf.clip_by_global_norm documents this; we follow it);
//   - TensorFlow's float32 summation order is not reproduced: the promise is the float64 norm, rounded once.
// Every sum has a fixed order -- per thread in element order, the 64 lanes of a wave by a halving tree, the four waves in wave
// order, the blocks of a variable in block order (by one lane for a short variable; lane-strided, then the tree, for a long one), the
// variables lane-strided and by the tree -- and there are no atomics: two runs give the same bits.
//
// Three passes (dl3p.h): sumsq reads g, w, l2_elem, lr_scale_elem once and leaves one float64 partial per workgroup; finalize (one
// workgroup) turns them into norm[] and scale[]; apply forms g' again and writes g <- clip(g') * scale[v] in place, so that the
// optimiser launch behind it takes G as the finished gradient (grad_scale = 1, l2_elem = NULL) and none of its seven entry points
// changes.  With clipvalue alone only apply runs (scale = NULL); it can leave the partials of the clamped gradient for logging.
//
// Work split: a block map {variable, block within the variable}, as dl3p_reduce_rows_batched has one: a workgroup takes up to
// CLIP_BLOCK consecutive floats of ONE variable, four at a time per thread as 16-byte accesses (variables start on 16-byte
// boundaries and have lengths that are multiples of 4 floats: ParamStore pads them, and the padding is frozen).
#include "common.h"
#include <math.h>

#define CLIP_BLOCK 4096          // floats per workgroup: 256 threads x 4 float4
#define CLIP_MAX_VARS 65536      // what the one-workgroup finalize kernel is asked to serve

struct ClipArgs {
  float* g; const float* w; const float* l2e; const float* lre;
  float gscale, cval;
  const int64_t* vars;           // [nvars][3] = {offset, length, first block} (floats, floats, block index)
  const int2* map;               // [nblocks] = {variable, block within the variable}
  const float* scale;            // apply: [nvars] or NULL
  double* partials;              // sumsq: [nblocks]; apply: [nblocks] or NULL
};

__device__ __forceinline__ float clip_form(float g, float w, float d, float gscale, float c) {
  float v = fmaf(g, gscale, 2.f * d * w);
  if (c > 0.f) v = v < -c ? -c : (v > c ? c : v);
  return v;
}

// sum over the 64 lanes (result in lane 0), a fixed halving tree
__device__ __forceinline__ double clip_wave_sum(double a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  return a;
}

// all 256 threads call; thread 0 returns the workgroup's sum (waves added in wave order)
__device__ __forceinline__ double clip_block_sum(double a) {
  __shared__ double sm[4];
  a = clip_wave_sum(a);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  return threadIdx.x == 0 ? ((sm[0] + sm[1]) + sm[2]) + sm[3] : 0.0;
}

// APPLY 0: sum of squares of clip(g') over the trainable elements of the block -> partials[block]
// APPLY 1: g <- clip(g') * scale[v] in place (and, with partials, the same sums of the clamped, unscaled gradient)
template <int APPLY>
__global__ __launch_bounds__(256) void grad_clip_kernel(ClipArgs p) {
  const int2 m = p.map[blockIdx.x];
  const int64_t off = p.vars[3 * m.x], len = p.vars[3 * m.x + 1];
  const int64_t begin = (int64_t)m.y * CLIP_BLOCK;
  const int count = (int)(len - begin < CLIP_BLOCK ? len - begin : CLIP_BLOCK);     // a multiple of 4, > 0 (checked on the host)
  const size_t base = (size_t)(off + begin);
  const float s = (APPLY && p.scale) ? p.scale[m.x] : 1.f;
  const bool scaled = APPLY && p.scale;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < CLIP_BLOCK / 1024; ++j) {
    const int e = (j * 256 + (int)threadIdx.x) * 4;
    if (e >= count) continue;
    const size_t i = base + e;
    const float4 m4 = p.lre ? ld4(p.lre + i) : make_float4(1.f, 1.f, 1.f, 1.f);
    if (m4.x == 0.f && m4.y == 0.f && m4.z == 0.f && m4.w == 0.f) continue;
    const float4 g4 = ld4(p.g + i);
    const float4 d4 = p.l2e ? ld4(p.l2e + i) : zero4();
    const float4 w4 = p.l2e ? ld4(p.w + i) : zero4();
    const float g[4] = {g4.x, g4.y, g4.z, g4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
    const float on[4] = {m4.x, m4.y, m4.z, m4.w};
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = clip_form(g[k], w[k], d[k], p.gscale, p.cval);
      if (on[k] != 0.f) acc += (double)v * (double)v;
      out[k] = on[k] != 0.f ? (scaled ? v * s : v) : g[k];
    }
    if (APPLY) st4(p.g + i, make_float4(out[0], out[1], out[2], out[3]));
  }
  if (!APPLY || p.partials) {
    const double t = clip_block_sum(acc);
    if (threadIdx.x == 0) p.partials[blockIdx.x] = t;
  }
}

// one workgroup of 16 waves: per-variable sums, the sum over the variables, norms and scales.  A wave takes 64 variables at a time,
// one per lane: a variable of at most CLIP_SMALL_BLOCKS blocks (most are a BatchNorm vector or a depthwise kernel: one block) is
// added up by its lane in block order, a longer one by the whole wave (lane-strided in block order, then the tree)
#define CLIP_SMALL_BLOCKS 16
__global__ __launch_bounds__(1024) void grad_clip_finalize_kernel(const double* __restrict__ partials, const int64_t* __restrict__ vars,
                                                                  int nvars, int mode, double c, float* __restrict__ scale,
                                                                  double* norm) {
  __shared__ double total_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int v0 = wave * 64; v0 < nvars; v0 += nwaves * 64) {
    const int v = v0 + lane;
    long long first = 0;
    int nb = 0;
    if (v < nvars) {
      const int64_t len = vars[3 * v + 1];
      first = vars[3 * v + 2];
      nb = (int)((len + CLIP_BLOCK - 1) / CLIP_BLOCK);
    }
    if (v < nvars && nb <= CLIP_SMALL_BLOCKS) {
      double a = 0.0;
      for (int b = 0; b < nb; ++b) a += partials[first + b];
      norm[v] = a;                              // the sum of squares for now
    }
    unsigned long long big = __ballot(v < nvars && nb > CLIP_SMALL_BLOCKS);
    while (big) {
      const int l = __ffsll(big) - 1;
      big &= big - 1;
      const long long f = __shfl(first, l, 64);
      const int n = __shfl(nb, l, 64);
      double a = 0.0;
      for (int b = lane; b < n; b += 64) a += partials[f + b];
      a = clip_wave_sum(a);
      if (lane == 0) norm[v0 + l] = a;
    }
  }
  __syncthreads();
  if (wave == 0) {
    double a = 0.0;
    for (int v = lane; v < nvars; v += 64) a += norm[v];
    a = clip_wave_sum(a);
    if (lane == 0) total_s = a;
  }
  __syncthreads();
  const double gn = sqrt(total_s);
  // c / max(norm, c) with a max that propagates NaN: 1 exactly at or below the threshold
  const float gs = !(gn - gn == 0.0) ? __builtin_nanf("") : (gn <= c ? 1.f : (float)(c / gn));
  for (int v = threadIdx.x; v < nvars; v += blockDim.x) {
    const double nv = sqrt(norm[v]);
    norm[v] = nv;
    scale[v] = mode == 2 ? gs : (nv <= c ? 1.f : (float)(c / nv));
  }
  if (threadIdx.x == 0) norm[nvars] = gn;
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int dl3p_grad_clip_block_elements(void) { return CLIP_BLOCK; }

static inline int64_t clip_blocks_of(int64_t len) { return len / CLIP_BLOCK + (len % CLIP_BLOCK != 0); }     // (no overflow)

// the tables as the host sees them: every block inside its variable, every variable inside the buffer, the blocks of a variable
// consecutive and in order (partials[first block + b] is what finalize adds up)
static int clip_check_tables(const char* fn, size_t n, const int64_t* vars_host, int nvars, const int* map_host, int nblocks) {
  DL3P_CHECK_ARG(vars_host && map_host, "%s: null host table", fn);
  DL3P_CHECK_ARG(nvars > 0 && nvars <= CLIP_MAX_VARS, "%s: nvars %d outside 1..%d", fn, nvars, CLIP_MAX_VARS);
  DL3P_CHECK_ARG(nblocks > 0, "%s: no blocks", fn);
  int64_t next = 0;
  for (int v = 0; v < nvars; ++v) {
    const int64_t off = vars_host[3 * v], len = vars_host[3 * v + 1], first = vars_host[3 * v + 2];
    DL3P_CHECK_ARG(off >= 0 && len > 0 && off % 4 == 0 && len % 4 == 0 && (uint64_t)off + (uint64_t)len <= n,
                   "%s: variable %d (offset %lld, length %lld) is not a 16-byte aligned range of the %zu floats", fn, v,
                   (long long)off, (long long)len, n);
    DL3P_CHECK_ARG(first == next, "%s: variable %d starts at block %lld, expected %lld", fn, v, (long long)first, (long long)next);
    next += clip_blocks_of(len);
  }
  DL3P_CHECK_ARG(next == nblocks, "%s: the variables have %lld blocks, the block map %d", fn, (long long)next, nblocks);
  for (int b = 0; b < nblocks; ++b) {
    const int v = map_host[2 * b], k = map_host[2 * b + 1];
    DL3P_CHECK_ARG(v >= 0 && v < nvars, "%s: block %d names variable %d of %d", fn, b, v, nvars);
    DL3P_CHECK_ARG(k >= 0 && (int64_t)k * CLIP_BLOCK < vars_host[3 * v + 1], "%s: block %d runs past its variable %d", fn, b, v);
    DL3P_CHECK_ARG(vars_host[3 * v + 2] + k == b, "%s: block %d is not block %d of variable %d", fn, b, k, v);
  }
  return DL3P_OK;
}

static int clip_check_buffers(const char* fn, const float* g, const float* w, const float* l2e, const float* lre, float gscale,
                              float cval, const int64_t* vars, const int* map) {
  DL3P_CHECK_ARG(g && vars && map && (w || !l2e), "%s: null pointer", fn);
  DL3P_CHECK_ARG(aligned16(g) && aligned16(w) && aligned16(l2e) && aligned16(lre), "%s: buffers must be 16-byte aligned", fn);
  DL3P_CHECK_ARG((reinterpret_cast<uintptr_t>(vars) & 7u) == 0 && (reinterpret_cast<uintptr_t>(map) & 7u) == 0,
                 "%s: tables must be 8-byte aligned", fn);
  DL3P_CHECK_ARG(gscale == gscale && cval >= 0.f && cval - cval == 0.f, "%s: clip_value must be 0 (off) or positive and finite", fn);
  return DL3P_OK;
}

extern "C" int dl3p_grad_clip_sumsq(const float* g, const float* w, const float* l2_elem, const float* lr_scale_elem, size_t n,
                                    float grad_scale, float clip_value, const int64_t* vars, const int64_t* vars_host, int nvars,
                                    const int* blockmap, const int* blockmap_host, int nblocks, double* partials, void* stream) {
  const char* fn = "dl3p_grad_clip_sumsq";
  int rc = clip_check_buffers(fn, g, w, l2_elem, lr_scale_elem, grad_scale, clip_value, vars, blockmap);
  if (rc) return rc;
  DL3P_CHECK_ARG(partials && (reinterpret_cast<uintptr_t>(partials) & 7u) == 0, "%s: null or misaligned partials", fn);
  rc = clip_check_tables(fn, n, vars_host, nvars, blockmap_host, nblocks);
  if (rc) return rc;
  ClipArgs p = {};
  p.g = const_cast<float*>(g); p.w = w; p.l2e = l2_elem; p.lre = lr_scale_elem; p.gscale = grad_scale; p.cval = clip_value;
  p.vars = vars; p.map = reinterpret_cast<const int2*>(blockmap); p.partials = partials;
  dl3p_launch(grad_clip_kernel<0>, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_grad_clip_finalize(const double* partials, const int64_t* vars, const int64_t* vars_host, int nvars, int nblocks,
                                       int mode, double threshold, float* scale, double* norm, void* stream) {
  const char* fn = "dl3p_grad_clip_finalize";
  DL3P_CHECK_ARG(partials && vars && vars_host && scale && norm, "%s: null pointer", fn);
  DL3P_CHECK_ARG(((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(vars) | reinterpret_cast<uintptr_t>(norm)) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(scale) & 3u) == 0, "%s: misaligned pointer", fn);
  DL3P_CHECK_ARG(mode == 1 || mode == 2, "%s: mode %d is neither 1 (per variable) nor 2 (global)", fn, mode);
  DL3P_CHECK_ARG(threshold > 0.0 && threshold - threshold == 0.0, "%s: threshold must be positive and finite", fn);
  DL3P_CHECK_ARG(nvars > 0 && nvars <= CLIP_MAX_VARS, "%s: nvars %d outside 1..%d", fn, nvars, CLIP_MAX_VARS);
  int64_t next = 0;
  for (int v = 0; v < nvars; ++v) {
    DL3P_CHECK_ARG(vars_host[3 * v + 1] > 0 && vars_host[3 * v + 2] == next, "%s: variable %d starts at block %lld, expected %lld", fn,
                   v, (long long)vars_host[3 * v + 2], (long long)next);
    next += clip_blocks_of(vars_host[3 * v + 1]);
  }
  DL3P_CHECK_ARG(next == nblocks, "%s: the variables have %lld blocks, the partials %d", fn, (long long)next, nblocks);
  dl3p_launch(grad_clip_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials, vars, nvars, mode, threshold, scale,
              norm);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_grad_clip_apply(float* g, const float* w, const float* l2_elem, const float* lr_scale_elem, size_t n,
                                    float grad_scale, float clip_value, const float* scale, const int64_t* vars,
                                    const int64_t* vars_host, int nvars, const int* blockmap, const int* blockmap_host, int nblocks,
                                    double* partials, void* stream) {
  const char* fn = "dl3p_grad_clip_apply";
  int rc = clip_check_buffers(fn, g, w, l2_elem, lr_scale_elem, grad_scale, clip_value, vars, blockmap);
  if (rc) return rc;
  DL3P_CHECK_ARG((reinterpret_cast<uintptr_t>(scale) & 3u) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7u) == 0,
                 "%s: misaligned scale or partials", fn);
  DL3P_CHECK_ARG(scale || clip_value > 0.f, "%s: neither a scale table nor a clip_value: nothing to apply", fn);
  rc = clip_check_tables(fn, n, vars_host, nvars, blockmap_host, nblocks);
  if (rc) return rc;
  ClipArgs p = {};
  p.g = g; p.w = w; p.l2e = l2_elem; p.lre = lr_scale_elem; p.gscale = grad_scale; p.cval = clip_value;
  p.vars = vars; p.map = reinterpret_cast<const int2*>(blockmap); p.scale = scale; p.partials = partials;
  dl3p_launch(grad_clip_kernel<1>, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
