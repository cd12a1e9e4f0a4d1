// The OpenCV steps of SegmentationGenerator.__getitem__ on the device (reference deeplabv3p/data.py:78-79, 105-111,
// common/data_utils.py:127-149, 241-273): random_zoom_rotate (cv2.warpAffine, INTER_NEAREST), random_histeq (BGR2YUV, CLAHE on Y,
// YUV2BGR) and the generator's final cv2.resize (INTER_LINEAR image, INTER_NEAREST label).
// UNPINNED restatements of OpenCV's published 8-bit arithmetic, like random_grayscale / random_blur in augment.hip: cv2 is not in this
// image, so the kernels are held bit for bit to tests/cv_rules.py, a NumPy statement of the same rules (DESIGN.md section 7 writes them
// out), not to OpenCV itself.  Everything float64 in those rules (the inverted rotation matrix, the resize scales) is evaluated on the
// host into small integer tables (augment.warp_tables / augment.resize_tables); the kernels are integer arithmetic plus, in CLAHE,
// float32 operations that are each rounded once (__fmul_rn / __fadd_rn / __fsub_rn: no fused multiply-add whatever the compiler flags).
#include "common.h"

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------- warpAffine, INTER_NEAREST, BORDER_CONSTANT 0
// tables of image n: adelta[W], bdelta[W], X0[H], Y0[H] (22.10 fixed point, the rounding half 512 already inside X0 / Y0).
// X = sat16((X0[y] + adelta[x]) >> 10): the sum wraps like OpenCV's int addition, the shift is arithmetic.
__global__ __launch_bounds__(256) void aug_warp_nn_kernel(const unsigned char* img, unsigned char* out, const unsigned char* label,
                                                          unsigned char* label_out, const int* flags, const int* tables, int H, int W) {
  const int n = blockIdx.y;
  const bool warp = flags[n] != 0;
  const int* adelta = tables + (size_t)n * (2 * W + 2 * H);
  const int* bdelta = adelta + W;
  const int* X0 = bdelta + W;
  const int* Y0 = X0 + H;
  const long long P = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    long long s = i;
    bool inside = true;
    if (warp) {
      const int X = clampi((int)((unsigned)X0[y] + (unsigned)adelta[x]) >> 10, -32768, 32767);
      const int Y = clampi((int)((unsigned)Y0[y] + (unsigned)bdelta[x]) >> 10, -32768, 32767);
      inside = X >= 0 && X < W && Y >= 0 && Y < H;
      s = (long long)Y * W + X;
    }
    const long long d = (long long)n * P + i;
    s += (long long)n * P;
    if (img) {
      out[3 * d] = inside ? img[3 * s] : 0; out[3 * d + 1] = inside ? img[3 * s + 1] : 0; out[3 * d + 2] = inside ? img[3 * s + 2] : 0;
    }
    if (label) label_out[d] = inside ? label[s] : 0;
  }
}

extern "C" int dl3p_aug_warp_nn_u8(const unsigned char* img, unsigned char* out, const unsigned char* label, unsigned char* label_out,
                                   const int* flags, const int* tables, int N, int H, int W, void* stream) {
  DL3P_CHECK_ARG((img || label) && flags && tables && N > 0 && H > 0 && W > 0, "dl3p_aug_warp_nn_u8: bad arguments");
  DL3P_CHECK_ARG((!img || (out && out != img)) && (!label || (label_out && label_out != label)), "dl3p_aug_warp_nn_u8: needs distinct outputs");
  const long long P = (long long)H * W;
  long long gx = ceil_div_ll(P, 256 * 8);
  if (gx > 1024) gx = 1024;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(aug_warp_nn_kernel, dim3((unsigned)gx, N), dim3(256), 0, (hipStream_t)stream, img, out, label, label_out, flags,
                     tables, H, W);
  DL3P_CHECK_LAUNCH("dl3p_aug_warp_nn_u8");
  return DL3P_OK;
}

// ---------------------------------------------------------------------------------- BGR2YUV, CLAHE(2.0, (8, 8)) on Y, YUV2BGR
// cvtColor on uint8 (yuv_shift = 14; c0 is the array's first channel: the reference hands an RGB array to a BGR conversion):
//   Y = DESCALE(c0 1868 + c1 9617 + c2 4899), U = DESCALE((c0 - Y) 8061 + (128 << 14)), V = DESCALE((c2 - Y) 14369 + (128 << 14))
//   c0 = Y + DESCALE((U - 128) 33292), c1 = Y + DESCALE((U - 128)(-6472) + (V - 128)(-9519)), c2 = Y + DESCALE((V - 128) 18678)
// DESCALE(v) = (v + 8192) >> 14 (arithmetic), every result clamped to 0..255.
__device__ __forceinline__ int cv_descale(int v) { return (v + 8192) >> 14; }
__device__ __forceinline__ int cv_luma(int c0, int c1, int c2) { return clampi(cv_descale(c0 * 1868 + c1 * 9617 + c2 * 4899), 0, 255); }
__device__ __forceinline__ int sat_u8_rint(float v) { return clampi((int)rintf(v), 0, 255); }

// pass 1, one workgroup per tile: histogram of Y over the tile of the (reflect-101 extended) plane in LDS, clip at `clip`, spread the
// excess (clipped / 256 to every bin, the residual to every step-th bin from bin 0), prefix sum, lut = sat_u8(rint(sum * lut_scale))
__global__ __launch_bounds__(256) void aug_clahe_lut_kernel(const unsigned char* img, const int* flags, unsigned char* luts, int H, int W,
                                                            int th, int tw, int clip, float lut_scale) {
  const int n = blockIdx.y;
  if (!flags[n]) return;                       // uniform over the workgroup: before any barrier
  __shared__ int hist[256];
  __shared__ int scan[2][256];
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  const int tile = blockIdx.x, ty = tile >> 3, tx = tile & 7;
  const unsigned char* src = img + (size_t)n * H * W * 3;
  hist[t] = 0;
  __syncthreads();
  const int area = th * tw;
  for (int i = t; i < area; i += 256) {
    const int r = i / tw, c = i - r * tw;
    int y = ty * th + r, x = tx * tw + c;
    if (y >= H) y = 2 * (H - 1) - y;           // BORDER_REFLECT_101 below / right of the image; H, W >= 8 keeps it >= 0
    if (x >= W) x = 2 * (W - 1) - x;
    const unsigned char* q = src + ((size_t)y * W + x) * 3;
    atomicAdd(&hist[cv_luma(q[0], q[1], q[2])], 1);
  }
  __syncthreads();
  int h = hist[t];
  int excess = h > clip ? h - clip : 0;
  for (int o = 32; o > 0; o >>= 1) excess += __shfl_xor(excess, o);
  if ((t & 63) == 0) wsum[t >> 6] = excess;
  __syncthreads();
  const int clipped = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  const int batch = clipped >> 8, residual = clipped - (batch << 8);
  h = (h > clip ? clip : h) + batch;
  if (residual) {                              // for (i = 0; i < 256 && residual > 0; i += step, --residual) ++h[i]
    const int step = 256 / residual > 1 ? 256 / residual : 1;
    if (t % step == 0 && t / step < residual) ++h;
  }
  int cur = 0;
  scan[0][t] = h;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {          // inclusive prefix sum, integers: any order gives the same value
    scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  luts[((size_t)n * 64 + tile) * 256 + t] = (unsigned char)sat_u8_rint(__fmul_rn((float)scan[cur][t], lut_scale));
}

// pass 2, per pixel of the ORIGINAL H x W: Y, U, V again from the untouched input pixel, Y through the four neighbouring LUTs, back
__global__ __launch_bounds__(256) void aug_clahe_apply_kernel(const unsigned char* img, unsigned char* out, const int* flags,
                                                              const unsigned char* luts, int H, int W, float inv_th, float inv_tw) {
  const int n = blockIdx.y;
  const bool on = flags[n] != 0;
  const long long P = (long long)H * W;
  const unsigned char* src = img + (size_t)n * P * 3;
  unsigned char* dst = out + (size_t)n * P * 3;
  const unsigned char* L = luts + (size_t)n * 64 * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    int c0 = src[3 * i], c1 = src[3 * i + 1], c2 = src[3 * i + 2];
    if (on) {
      const int y = (int)(i / W), x = (int)(i - (long long)y * W);
      const int Y = cv_luma(c0, c1, c2);
      const int U = clampi(cv_descale((c0 - Y) * 8061 + (128 << 14)), 0, 255);
      const int V = clampi(cv_descale((c2 - Y) * 14369 + (128 << 14)), 0, 255);
      const float txf = __fsub_rn(__fmul_rn((float)x, inv_tw), 0.5f), tyf = __fsub_rn(__fmul_rn((float)y, inv_th), 0.5f);
      const float fx = floorf(txf), fy = floorf(tyf);
      const float xa = __fsub_rn(txf, fx), ya = __fsub_rn(tyf, fy);
      const float xa1 = __fsub_rn(1.0f, xa), ya1 = __fsub_rn(1.0f, ya);
      const int tx1u = (int)fx, ty1u = (int)fy;      // clamped only after the weights are formed
      const int tx1 = tx1u > 0 ? tx1u : 0, tx2 = tx1u + 1 < 7 ? tx1u + 1 : 7;
      const int ty1 = ty1u > 0 ? ty1u : 0, ty2 = ty1u + 1 < 7 ? ty1u + 1 : 7;
      const float l11 = (float)L[(ty1 * 8 + tx1) * 256 + Y], l12 = (float)L[(ty1 * 8 + tx2) * 256 + Y];
      const float l21 = (float)L[(ty2 * 8 + tx1) * 256 + Y], l22 = (float)L[(ty2 * 8 + tx2) * 256 + Y];
      const float top = __fadd_rn(__fmul_rn(l11, xa1), __fmul_rn(l12, xa));
      const float bot = __fadd_rn(__fmul_rn(l21, xa1), __fmul_rn(l22, xa));
      const int Yq = sat_u8_rint(__fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya)));
      c0 = clampi(Yq + cv_descale((U - 128) * 33292), 0, 255);
      c1 = clampi(Yq + cv_descale((U - 128) * -6472 + (V - 128) * -9519), 0, 255);
      c2 = clampi(Yq + cv_descale((V - 128) * 18678), 0, 255);
    }
    dst[3 * i] = (unsigned char)c0; dst[3 * i + 1] = (unsigned char)c1; dst[3 * i + 2] = (unsigned char)c2;
  }
}

extern "C" int dl3p_aug_clahe_u8(const unsigned char* img, unsigned char* out, const int* flags, unsigned char* luts, size_t luts_bytes,
                                 int N, int H, int W, void* stream) {
  DL3P_CHECK_ARG(img && out && flags && luts && N > 0, "dl3p_aug_clahe_u8: bad arguments");
  DL3P_CHECK_ARG(H >= 8 && W >= 8, "dl3p_aug_clahe_u8: an 8 x 8 tile grid needs H, W >= 8 (got %d x %d)", H, W);
  DL3P_CHECK_ARG(luts_bytes >= (size_t)N * 64 * 256, "dl3p_aug_clahe_u8: the LUT workspace holds N x 64 x 256 bytes");
  const int th = (H + 7) / 8, tw = (W + 7) / 8;     // tile of the plane extended to a multiple of 8
  DL3P_CHECK_ARG((long long)th * tw < (1 << 24), "dl3p_aug_clahe_u8: tile area beyond exact float32 counts");
  const int area = th * tw;
  int clip = (int)(2.0 * area / 256);
  if (clip < 1) clip = 1;
  // host float32 divisions (IEEE, rounded once): lutScale = 255.0f / area, and the reciprocal tile sizes of the interpolation
  const float lut_scale = 255.0f / (float)area, inv_th = 1.0f / (float)th, inv_tw = 1.0f / (float)tw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(aug_clahe_lut_kernel, dim3(64, N), dim3(256), 0, st, img, flags, luts, H, W, th, tw, clip, lut_scale);
  DL3P_CHECK_LAUNCH("dl3p_aug_clahe_u8 (tables)");
  const long long P = (long long)H * W;
  long long gx = ceil_div_ll(P, 256 * 4);
  if (gx > 2048) gx = 2048;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(aug_clahe_apply_kernel, dim3((unsigned)gx, N), dim3(256), 0, st, img, out, flags, luts, H, W, inv_th, inv_tw);
  DL3P_CHECK_LAUNCH("dl3p_aug_clahe_u8");
  return DL3P_OK;
}

// ---------------------------------------------------------------------------------- cv2.resize: INTER_LINEAR image, INTER_NEAREST label
// tables: sx[W], x1[W], a0[W], a1[W], nx[W], sy0[H], sy1[H], b0[H], b1[H], ny[H].  Linear, in OpenCV's 11-bit fixed point:
//   T[row][dx] = S[row][sx] a0 + S[row][x1] a1;  out = (((b0 (T[sy0] >> 4)) >> 16) + ((b1 (T[sy1] >> 4)) >> 16) + 2) >> 2
// mode 0: equal size, a copy; mode 1: exactly half size, INTER_LINEAR turns into the 2 x 2 area mean (s00 + s01 + s10 + s11 + 2) >> 2.
// Source indices from the tables are clamped to the image again here: a bad table cannot make the kernel read outside it.
__global__ __launch_bounds__(256) void aug_resize_kernel(const unsigned char* img, int img_pitch, unsigned char* out,
                                                         const unsigned char* label, int label_pitch, unsigned char* label_out,
                                                         const int* tables, int mode, int h, int w, int H, int W) {
  const int n = blockIdx.y;
  const int *sx = tables, *x1 = sx + W, *a0 = x1 + W, *a1 = a0 + W, *nx = a1 + W;
  const int *sy0 = nx + W, *sy1 = sy0 + H, *b0 = sy1 + H, *b1 = b0 + H, *ny = b1 + H;
  const long long P = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const long long d = (long long)n * P + i;
    if (img) {
      const unsigned char* src = img + (size_t)n * h * img_pitch;
      if (mode == 0) {
        const unsigned char* q = src + (size_t)y * img_pitch + 3 * x;
        out[3 * d] = q[0]; out[3 * d + 1] = q[1]; out[3 * d + 2] = q[2];
      } else if (mode == 1) {
        const unsigned char* q = src + (size_t)(2 * y) * img_pitch + 6 * x;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * d + c] = (unsigned char)((q[c] + q[3 + c] + q[img_pitch + c] + q[img_pitch + 3 + c] + 2) >> 2);
      } else {
        const int xs = clampi(sx[x], 0, w - 1), xe = clampi(x1[x], 0, w - 1), wa0 = a0[x], wa1 = a1[x];
        const unsigned char* r0 = src + (size_t)clampi(sy0[y], 0, h - 1) * img_pitch;
        const unsigned char* r1 = src + (size_t)clampi(sy1[y], 0, h - 1) * img_pitch;
        const int wb0 = b0[y], wb1 = b1[y];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int t0 = r0[3 * xs + c] * wa0 + r0[3 * xe + c] * wa1, t1 = r1[3 * xs + c] * wa0 + r1[3 * xe + c] * wa1;
          out[3 * d + c] = (unsigned char)((((wb0 * (t0 >> 4)) >> 16) + ((wb1 * (t1 >> 4)) >> 16) + 2) >> 2);
        }
      }
    }
    if (label)
      label_out[d] = label[(size_t)n * h * label_pitch + (size_t)clampi(ny[y], 0, h - 1) * label_pitch + clampi(nx[x], 0, w - 1)];
  }
}

extern "C" int dl3p_aug_resize_u8(const unsigned char* img, int img_pitch, unsigned char* out, const unsigned char* label, int label_pitch,
                                  unsigned char* label_out, const int* tables, int N, int h, int w, int H, int W, void* stream) {
  DL3P_CHECK_ARG((img || label) && tables && N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "dl3p_aug_resize_u8: bad arguments");
  DL3P_CHECK_ARG((!img || (out && out != img && img_pitch >= 3 * w)) && (!label || (label_out && label_out != label && label_pitch >= w)),
                 "dl3p_aug_resize_u8: needs distinct outputs and row pitches of at least one row");
  const int mode = (h == H && w == W) ? 0 : ((h == 2 * H && w == 2 * W) ? 1 : 2);
  const long long P = (long long)H * W;
  long long gx = ceil_div_ll(P, 256 * 4);
  if (gx > 2048) gx = 2048;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(aug_resize_kernel, dim3((unsigned)gx, N), dim3(256), 0, (hipStream_t)stream, img, img_pitch, out, label, label_pitch,
                     label_out, tables, mode, h, w, H, W);
  DL3P_CHECK_LAUNCH("dl3p_aug_resize_u8");
  return DL3P_OK;
}
