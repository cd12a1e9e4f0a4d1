// The byte-level ends of the reference's deeplab.py on the device (common/data_utils.py:436-477, common/utils.py:221-263, 305-315):
// preprocess_image's Image.resize(size, BICUBIC) in front of the network, and behind it mask_resize (cv2.INTER_NEAREST back to the
// frame's size), the PASCAL colour map and the alpha composite of visualize_segmentation, at the frame's own resolution.
// dl3p_pil_resize_u8 is PINNED: Pillow's 8-bit resampler (ImagingResample: 22-bit fixed-point coefficients, a horizontal pass rounded
// to bytes, then a vertical pass) restated in integers and held bit for bit to tests/pil_rules.py, which is held to Pillow itself
// (live and tests/golden/pil_bicubic.npz).  dl3p_mask_overlay_u8 follows this repository's stated rules: the INTER_NEAREST index rule
// of tests/cv_rules.py and the project's own integer blend.  Everything float64 (the filter weights, the nearest
// scales) is evaluated on the host into integer tables (augment.pil_resize_tables, inference.overlay_tables); the kernels read only those.
#include "common.h"

#define PIL_MAX_K 65        // coefficients per output sample: a shrink by up to 16 (support 2 * 16, 2 * 32 + 1 taps)
#define PIL_BITS 22         // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int io_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int io_mini(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int pil_clip8(int acc) { return io_clampi(acc >> PIL_BITS, 0, 255); }

// ---------------------------------------------------------------------------------- Image.resize(size, BICUBIC), horizontal pass
// tab: xmin[W], xcnt[W], k[W][kx].  rows = N h source rows, src_pitch / dst_pitch bytes apart.  A workgroup owns 64 output columns
// (one per lane) and walks rows, one per wave at a time: the 64 coefficient rows are staged once in LDS, tap-major with a row of 65
// words, so the staging writes (consecutive taps of one column) and the reads (one tap of consecutive columns) both fall on
// different banks.  The taps of one output are 3 cnt contiguous bytes of one source row.
// xmin / xcnt are clamped to the row again here: a bad table cannot make the kernel read outside it.
__global__ __launch_bounds__(256) void pil_resize_h_kernel(const unsigned char* __restrict__ src, int src_pitch,
                                                           unsigned char* __restrict__ dst, int dst_pitch, const int* __restrict__ tab,
                                                           int kx, long long rows, int w, int W) {
  __shared__ int coef[PIL_MAX_K * 65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * 64;
  const int ncol = io_mini(64, W - x0);
  const int* k = tab + 2 * (size_t)W + (size_t)x0 * kx;
  for (int i = threadIdx.x; i < ncol * kx; i += 256) {
    const int c = i / kx, t = i - c * kx;
    coef[t * 65 + c] = k[i];
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= W) return;                                  // (no barrier below)
  const int xmin = io_clampi(tab[x], 0, w - 1);
  const int cnt = io_clampi(tab[W + x], 0, io_mini(kx, w - xmin));
  for (long long r = (long long)blockIdx.y * 4 + wave; r < rows; r += (long long)gridDim.y * 4) {
    const unsigned char* p = src + (size_t)r * src_pitch + 3 * (size_t)xmin;
    int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < cnt; ++t) {
      const int c = coef[t * 65 + lane];
      a0 += p[3 * t] * c; a1 += p[3 * t + 1] * c; a2 += p[3 * t + 2] * c;
    }
    unsigned char* q = dst + (size_t)r * dst_pitch + 3 * (size_t)x;
    q[0] = (unsigned char)pil_clip8(a0); q[1] = (unsigned char)pil_clip8(a1); q[2] = (unsigned char)pil_clip8(a2);
  }
}

// ---------------------------------------------------------------------------------- vertical pass
// tab: ymin[H], ycnt[H], k[H][ky].  A workgroup belongs to one output row of one image, so the row's first tap, tap count and
// coefficients are the same in every lane (scalar loads); the taps are whole source rows of RB = 3 W bytes, read V bytes per lane.
// V = 4: one 32-bit load per tap and one 32-bit store (the host picks it when both pointers, the source pitch and RB allow it).
template <int V>
__global__ __launch_bounds__(256) void pil_resize_v_kernel(const unsigned char* __restrict__ src, int src_pitch,
                                                           unsigned char* __restrict__ dst, const int* __restrict__ tab, int ky, int h,
                                                           int H, int RB) {
  const int Y = blockIdx.y, n = blockIdx.z;
  const int ymin = io_clampi(tab[Y], 0, h - 1);
  const int cnt = io_clampi(tab[H + Y], 0, io_mini(ky, h - ymin));
  const int* k = tab + 2 * (size_t)H + (size_t)Y * ky;
  const unsigned char* s = src + ((size_t)n * h + ymin) * src_pitch;
  unsigned char* d = dst + ((size_t)n * H + Y) * RB;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < RB; i += gridDim.x * 256 * V) {
    int acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 1 << (PIL_BITS - 1);
    for (int t = 0; t < cnt; ++t) {
      const int c = k[t];
      const unsigned char* p = s + (size_t)t * src_pitch + i;
      if (V == 4) {
        const unsigned v = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * c;
      } else {
        acc[0] += p[0] * c;
      }
    }
    if (V == 4) {
      unsigned v = 0;
#pragma unroll
      for (int j = 0; j < V; ++j) v |= (unsigned)pil_clip8(acc[j]) << (8 * j);
      *reinterpret_cast<unsigned*>(d + i) = v;
    } else {
      d[i] = (unsigned char)pil_clip8(acc[0]);
    }
  }
}

static inline size_t pil_tmp_pitch(int W) { return ((size_t)3 * W + 3) & ~(size_t)3; }

extern "C" size_t dl3p_pil_resize_workspace(int N, int h, int w, int H, int W) {
  if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1 || w == W || h == H) return 0;      // at most one pass: no intermediate
  return (size_t)N * h * pil_tmp_pitch(W);
}

static void pil_launch_v(const unsigned char* src, int src_pitch, unsigned char* dst, const int* tab, int ky, int N, int h, int H, int W,
                         hipStream_t st) {
  const int RB = 3 * W;
  const bool vec = RB % 4 == 0 && src_pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst) & 3u) == 0;
  const int per_block = 256 * (vec ? 4 : 1);
  int gx = ceil_div(RB, per_block);
  if (gx > 64) gx = 64;
  if (vec)
    hipLaunchKernelGGL(pil_resize_v_kernel<4>, dim3(gx, H, N), dim3(256), 0, st, src, src_pitch, dst, tab, ky, h, H, RB);
  else
    hipLaunchKernelGGL(pil_resize_v_kernel<1>, dim3(gx, H, N), dim3(256), 0, st, src, src_pitch, dst, tab, ky, h, H, RB);
}

extern "C" int dl3p_pil_resize_u8(const unsigned char* img, int img_pitch, unsigned char* out, unsigned char* workspace,
                                  size_t workspace_bytes, const int* tables, int kx, int ky, int N, int h, int w, int H, int W,
                                  void* stream) {
  DL3P_CHECK_ARG(img && out && out != img && N > 0 && h > 0 && w > 0, "dl3p_pil_resize_u8: bad arguments");
  DL3P_CHECK_ARG(H >= 1 && W >= 1, "dl3p_pil_resize_u8: the output size must be at least 1 x 1 (got %d x %d)", H, W);
  DL3P_CHECK_ARG(N <= 65535 && H <= 65535 && w <= (1 << 24) && W <= (1 << 24) && (long long)img_pitch >= 3ll * w,
                 "dl3p_pil_resize_u8: N, H up to 65535, rows up to 2^24 pixels, a row pitch of at least one row");
  DL3P_CHECK_ARG(kx >= 0 && ky >= 0 && kx <= PIL_MAX_K && ky <= PIL_MAX_K,
                 "dl3p_pil_resize_u8: at most %d coefficients per sample (a shrink by up to 16), got ksize %d x %d", PIL_MAX_K, kx, ky);
  DL3P_CHECK_ARG((kx == 0) == (w == W) && (ky == 0) == (h == H),
                 "dl3p_pil_resize_u8: a pass is skipped (ksize 0) exactly when its axis keeps its length");
  DL3P_CHECK_ARG(tables || (!kx && !ky), "dl3p_pil_resize_u8: the coefficient tables are missing");
  const size_t need = dl3p_pil_resize_workspace(N, h, w, H, W);
  DL3P_CHECK_ARG(need == 0 || (workspace && workspace != img && workspace != out && workspace_bytes >= need &&
                               (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0),
                 "dl3p_pil_resize_u8: short workspace: two passes need %zu bytes (dl3p_pil_resize_workspace), 4-byte aligned, got %zu",
                 need, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (!kx && !ky) {                                     // equal size: Pillow returns a copy
    hipError_t e = hipMemcpy2DAsync(out, (size_t)3 * W, img, (size_t)img_pitch, (size_t)3 * W, (size_t)N * h, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      dl3p_set_error("dl3p_pil_resize_u8: copy failed: %s", hipGetErrorString(e));
      return DL3P_ELAUNCH;
    }
    return DL3P_OK;
  }
  const int* ytab = tables + (kx ? (size_t)W * (2 + kx) : 0);
  const unsigned char* vsrc = img;
  int vpitch = img_pitch;
  if (kx) {
    unsigned char* hdst = ky ? workspace : out;
    const int hpitch = ky ? (int)pil_tmp_pitch(W) : 3 * W;
    const long long rows = (long long)N * h;
    const int gx = ceil_div(W, 64);
    long long gy = ceil_div_ll(rows, 16);                // four rows per wave before another workgroup stages the same coefficients
    const long long cap = 2048 / gx > 1 ? 2048 / gx : 1;
    if (gy > cap) gy = cap;
    hipLaunchKernelGGL(pil_resize_h_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, st, img, img_pitch, hdst, hpitch, tables, kx, rows, w,
                       W);
    DL3P_CHECK_LAUNCH("dl3p_pil_resize_u8 (horizontal)");
    vsrc = hdst;
    vpitch = hpitch;
  }
  if (ky) {
    pil_launch_v(vsrc, vpitch, out, ytab, ky, N, h, H, W, st);
    DL3P_CHECK_LAUNCH("dl3p_pil_resize_u8 (vertical)");
  }
  return DL3P_OK;
}

// ---------------------------------------------------------------------------------- mask_resize + colour map + alpha composite
// tab: nx[w0], ny[h0], the INTER_NEAREST source index of every output column / row (clamped to the mask again here).
//   m = pred[n][ny[y]][nx[x]];  mask_out = (uint8) m;  d = (n_valid > 0 && m > n_valid - 1) ? n_valid : m;  col = colormap[d]
//   overlay_out = (img (256 - A) + col A + 128) >> 8 per channel
// V pixels per lane: 4 when w0 is a multiple of 4 and every pointer is 4-byte aligned (3 + 3 + 1 32-bit accesses), else 1.
template <int V>
__global__ __launch_bounds__(256) void mask_overlay_kernel(const int* __restrict__ pred, const unsigned char* __restrict__ img,
                                                           unsigned char* __restrict__ mask_out, unsigned char* __restrict__ overlay_out,
                                                           const int* __restrict__ tab, const unsigned char* __restrict__ colormap,
                                                           int n_valid, int A, int H, int W, int h0, int w0) {
  const int n = blockIdx.y;
  const int* nx = tab;
  const int* ny = tab + w0;
  const long long P = (long long)h0 * w0;
  const int* pm = pred + (size_t)n * H * W;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V; i < P; i += (long long)gridDim.x * 256 * V) {
    const int y = (int)(i / w0), x = (int)(i - (long long)y * w0);      // (V == 4: w0 % 4 == 0, the V pixels share the row)
    const int* row = pm + (size_t)io_clampi(ny[y], 0, H - 1) * W;
    const size_t o = (size_t)n * P + i;
    unsigned char px[3 * V], mk[V];
    if (overlay_out) {
      if (V == 4) {
        const unsigned* q = reinterpret_cast<const unsigned*>(img + 3 * o);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const unsigned v = q[j];
          px[4 * j] = v & 255u; px[4 * j + 1] = (v >> 8) & 255u; px[4 * j + 2] = (v >> 16) & 255u; px[4 * j + 3] = v >> 24;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = img[3 * o + c];
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int m = row[io_clampi(nx[x + j], 0, W - 1)];
      mk[j] = (unsigned char)m;
      if (overlay_out) {
        const int d = io_clampi((n_valid > 0 && m > n_valid - 1) ? n_valid : m, 0, 255);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[3 * j + c] = (unsigned char)((px[3 * j + c] * (256 - A) + colormap[3 * d + c] * A + 128) >> 8);
      }
    }
    if (V == 4) {
      if (mask_out) *reinterpret_cast<unsigned*>(mask_out + o) = mk[0] | (mk[1] << 8) | (mk[2] << 16) | ((unsigned)mk[3] << 24);
      if (overlay_out) {
        unsigned* q = reinterpret_cast<unsigned*>(overlay_out + 3 * o);
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] = px[4 * j] | (px[4 * j + 1] << 8) | (px[4 * j + 2] << 16) | ((unsigned)px[4 * j + 3] << 24);
      }
    } else {
      if (mask_out) mask_out[o] = mk[0];
      if (overlay_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) overlay_out[3 * o + c] = px[c];
      }
    }
  }
}

extern "C" int dl3p_mask_overlay_u8(const int* pred, const unsigned char* img, unsigned char* mask_out, unsigned char* overlay_out,
                                    const int* tables, const unsigned char* colormap, int n_valid, int alpha, int N, int H, int W, int h0,
                                    int w0, void* stream) {
  DL3P_CHECK_ARG(pred && tables && (mask_out || overlay_out) && N > 0 && N <= 65535 && H > 0 && W > 0 && h0 > 0 && w0 > 0,
                 "dl3p_mask_overlay_u8: bad arguments");
  DL3P_CHECK_ARG(!overlay_out || (img && colormap && overlay_out != img), "dl3p_mask_overlay_u8: the overlay needs the frame, the colour map and an output of its own");
  DL3P_CHECK_ARG(alpha >= 0 && alpha <= 256 && n_valid >= 0 && n_valid <= 255,
                 "dl3p_mask_overlay_u8: alpha is 0..256 (overlay * 256), n_valid 0..255 (got %d, %d)", alpha, n_valid);
  const long long P = (long long)h0 * w0;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(mask_out) | reinterpret_cast<uintptr_t>(overlay_out);
  const bool vec = w0 % 4 == 0 && (bits & 3u) == 0;
  long long gx = ceil_div_ll(P, 256 * (vec ? 4 : 1));
  if (gx > 2048) gx = 2048;
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(mask_overlay_kernel<4>, dim3((unsigned)gx, N), dim3(256), 0, st, pred, img, mask_out, overlay_out, tables, colormap,
                       n_valid, alpha, H, W, h0, w0);
  else
    hipLaunchKernelGGL(mask_overlay_kernel<1>, dim3((unsigned)gx, N), dim3(256), 0, st, pred, img, mask_out, overlay_out, tables, colormap,
                       n_valid, alpha, H, W, h0, w0);
  DL3P_CHECK_LAUNCH("dl3p_mask_overlay_u8");
  return DL3P_OK;
}
