// Narrow-output dense k x k convolutions (k = 3, stride 1, 'same'): PeleeNet's dense-layer branch1b / branch2b / branch2c
// convs (deeplabv3p_peleenet.py:73-83, Cout = 16, Cin = 16 / 32 / 64).  At these channel counts the implicit GEMM of
// dl3p_conv2d_gemm_* spends most of every MFMA tile on padding; these kernels are direct, packed-FMA convolutions.  Measured
// slower than the implicit GEMM at every PeleeNet shape: the executor takes them with DL3P_NARROW_CONV=1 only.
//
// One workgroup (256 threads) works on tiles of TH x TW output pixels of one image.  The input tile with its 1-pixel halo is
// staged in LDS once per tile -- act(x * scale + shift) formed on the way in, zeros outside the image ('same' padding pads the
// activated input) -- so each input pixel is read from HBM once per tile, (TH+2)(TW+2)/(TH TW) = 1.4 times per launch.  The
// kernel (9 Cin Cout floats, at most 72 KB) is read through the vector cache: a wavefront's lanes ask for at most Cout / 4
// distinct float4 per step.
//   fwd:        y [N][H][W][Cout] (ldy) = conv(act(x)); with stat_partials, one row [2][Cout] (sum, sum of squares) per workgroup,
//               summed over its tiles in a fixed order (deterministic), for dl3p_bn_finalize.
//   bwd_data:   gx (+)= d/d(act(x)) (the producer's BatchNorm backward applies act'), dy tile with halo in LDS.
//   bwd_weight: one slab of 9 Cin Cout partial sums per workgroup, pixels in a fixed order; dl3p_reduce_rows(_batched) sums the
//               slabs in row order -- no float atomics.
#include "common.h"

namespace {

constexpr int TH = 8, TW = 16, TP = TH * TW;          // output pixels per tile
constexpr int HH = TH + 2, HW = TW + 2;               // with the halo
constexpr int NT = 256;
constexpr int MAX_CIN = 64, MAX_COUT = 32;
constexpr int MAX_WTASK = 9 * MAX_CIN * MAX_COUT / 4 / NT;   // float4 weight-gradient accumulators per thread (18)

struct NarrowParams {
  const float* x; int ldx;
  const float* scale; const float* shift; int act;
  const float* w;                 // [3][3][Cin][Cout]
  const float* dy; int lddy;
  float* y; int ldy;              // fwd output / bwd_data gx
  float* part;                    // fwd: stat partial rows; bwd_weight: slabs
  int accumulate;
  int N, H, W, Cin, Cout;
  int tiles_y, tiles_x, ntiles;
};

__device__ __forceinline__ void tile_coords(const NarrowParams& p, int t, int& n, int& y0, int& x0) {
  const int tx = t % p.tiles_x;
  int r = t / p.tiles_x;
  const int ty = r % p.tiles_y;
  n = r / p.tiles_y;
  y0 = ty * TH;
  x0 = tx * TW;
}

// act(x) of the tile rows y0-1 .. y0+TH, columns x0-1 .. x0+TW into xs [HH*HW][Cin]
__device__ __forceinline__ void stage_input(const NarrowParams& p, float* xs, int n, int y0, int x0) {
  const int c4n = p.Cin / 4;
  const float* img = p.x + (size_t)n * p.H * p.W * p.ldx;
  for (int i = threadIdx.x; i < HH * HW * c4n; i += NT) {
    const int c = (i % c4n) * 4;
    const int pix = i / c4n;
    const int iy = y0 - 1 + pix / HW, ix = x0 - 1 + pix % HW;
    float4 v = zero4();
    if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
      v = ld4(img + ((size_t)iy * p.W + ix) * p.ldx + c);
      if (p.scale) v = fma4(v, ld4(p.scale + c), ld4(p.shift + c));
      v = act_apply4(v, p.act);
    }
    *reinterpret_cast<float4*>(xs + pix * p.Cin + c) = v;
  }
}

__global__ __launch_bounds__(NT) void narrow_fwd_kernel(NarrowParams p) {
  extern __shared__ float4 smem4[];
  float* xs = reinterpret_cast<float*>(smem4);
  const int c4n = p.Cout / 4;                 // 1, 2, 4 or 8: divides NT, so a thread keeps one output channel group
  const int co = (threadIdx.x % c4n) * 4;
  float4 s = zero4(), q = zero4();
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    int n, y0, x0;
    tile_coords(p, t, n, y0, x0);
    __syncthreads();
    stage_input(p, xs, n, y0, x0);
    __syncthreads();
    for (int task = threadIdx.x; task < TP * c4n; task += NT) {
      const int pix = task / c4n;
      const int py = pix / TW, px = pix % TW;
      float4 acc = zero4();
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          const float* xr = xs + ((py + ky) * HW + px + kx) * p.Cin;
          const float* wr = p.w + (size_t)(ky * 3 + kx) * p.Cin * p.Cout + co;
          for (int ci = 0; ci < p.Cin; ci += 4) {
            const float4 xv = *reinterpret_cast<const float4*>(xr + ci);
            acc = fma4(make_float4(xv.x, xv.x, xv.x, xv.x), ld4(wr + (size_t)(ci + 0) * p.Cout), acc);
            acc = fma4(make_float4(xv.y, xv.y, xv.y, xv.y), ld4(wr + (size_t)(ci + 1) * p.Cout), acc);
            acc = fma4(make_float4(xv.z, xv.z, xv.z, xv.z), ld4(wr + (size_t)(ci + 2) * p.Cout), acc);
            acc = fma4(make_float4(xv.w, xv.w, xv.w, xv.w), ld4(wr + (size_t)(ci + 3) * p.Cout), acc);
          }
        }
      const int oy = y0 + py, ox = x0 + px;
      if (oy < p.H && ox < p.W) {
        st4(p.y + (((size_t)n * p.H + oy) * p.W + ox) * p.ldy + co, acc);
        s = add4(s, acc);
        q = add4(q, mul4(acc, acc));
      }
    }
  }
  if (!p.part) return;
  // per-channel sums of this workgroup: threads with the same channel group, in thread order
  __syncthreads();
  float4* red = smem4;                        // [2][NT]
  red[threadIdx.x] = s;
  red[NT + threadIdx.x] = q;
  __syncthreads();
  if (threadIdx.x < 2 * c4n) {
    const int which = threadIdx.x / c4n, g = threadIdx.x % c4n;
    float4 a = zero4();
    for (int i = g; i < NT; i += c4n) a = add4(a, red[which * NT + i]);
    st4(p.part + (size_t)blockIdx.x * 2 * p.Cout + which * p.Cout + g * 4, a);
  }
}

__global__ __launch_bounds__(NT) void narrow_bwd_data_kernel(NarrowParams p) {
  extern __shared__ float4 smem4[];
  float* ds = reinterpret_cast<float*>(smem4);     // dy rows y0-1 .. y0+TH [HH*HW][Cout]
  const int ci4n = p.Cin / 4, co4n = p.Cout / 4;
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    int n, y0, x0;
    tile_coords(p, t, n, y0, x0);
    __syncthreads();
    for (int i = threadIdx.x; i < HH * HW * co4n; i += NT) {
      const int c = (i % co4n) * 4;
      const int pix = i / co4n;
      const int oy = y0 - 1 + pix / HW, ox = x0 - 1 + pix % HW;
      float4 v = zero4();
      if (oy >= 0 && oy < p.H && ox >= 0 && ox < p.W) v = ld4(p.dy + (((size_t)n * p.H + oy) * p.W + ox) * p.lddy + c);
      *reinterpret_cast<float4*>(ds + pix * p.Cout + c) = v;
    }
    __syncthreads();
    for (int task = threadIdx.x; task < TP * ci4n; task += NT) {
      const int ci = (task % ci4n) * 4;
      const int pix = task / ci4n;
      const int py = pix / TW, px = pix % TW;
      const int iy = y0 + py, ix = x0 + px;
      if (iy >= p.H || ix >= p.W) continue;
      float4 g = zero4();
      // gx[i] = sum over taps of dy[i - (ky - 1, kx - 1)] . w[ky][kx][ci][:]
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          const float* dr = ds + ((py + 2 - ky) * HW + px + 2 - kx) * p.Cout;
          const float* wr = p.w + ((size_t)(ky * 3 + kx) * p.Cin + ci) * p.Cout;
          for (int co = 0; co < p.Cout; co += 4) {
            const float4 d = *reinterpret_cast<const float4*>(dr + co);
            const float4 w0 = ld4(wr + co), w1 = ld4(wr + p.Cout + co), w2 = ld4(wr + 2 * p.Cout + co),
                         w3 = ld4(wr + 3 * p.Cout + co);
            g.x += d.x * w0.x + d.y * w0.y + d.z * w0.z + d.w * w0.w;
            g.y += d.x * w1.x + d.y * w1.y + d.z * w1.z + d.w * w1.w;
            g.z += d.x * w2.x + d.y * w2.y + d.z * w2.z + d.w * w2.w;
            g.w += d.x * w3.x + d.y * w3.y + d.z * w3.z + d.w * w3.w;
          }
        }
      float* o = p.y + (((size_t)n * p.H + iy) * p.W + ix) * p.ldy + ci;
      if (p.accumulate) g = add4(g, ld4(o));
      st4(o, g);
    }
  }
}

__global__ __launch_bounds__(NT) void narrow_bwd_weight_kernel(NarrowParams p) {
  extern __shared__ float4 smem4[];
  float* xs = reinterpret_cast<float*>(smem4);                  // [HH*HW][Cin]
  float* ds = xs + HH * HW * p.Cin;                             // [TP][Cout]
  const int co4n = p.Cout / 4;
  const int ntask = 9 * p.Cin * co4n;                           // (tap, ci, co4), co4 fastest
  float4 acc[MAX_WTASK];
#pragma unroll
  for (int j = 0; j < MAX_WTASK; ++j) acc[j] = zero4();
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    int n, y0, x0;
    tile_coords(p, t, n, y0, x0);
    __syncthreads();
    stage_input(p, xs, n, y0, x0);
    for (int i = threadIdx.x; i < TP * co4n; i += NT) {
      const int c = (i % co4n) * 4;
      const int pix = i / co4n;
      const int oy = y0 + pix / TW, ox = x0 + pix % TW;
      float4 v = zero4();                                       // (pixels outside the image contribute nothing)
      if (oy < p.H && ox < p.W) v = ld4(p.dy + (((size_t)n * p.H + oy) * p.W + ox) * p.lddy + c);
      *reinterpret_cast<float4*>(ds + pix * p.Cout + c) = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MAX_WTASK; ++j) {
      const int task = threadIdx.x + j * NT;
      if (task < ntask) {
      const int co = (task % co4n) * 4;
      const int r = task / co4n;
      const int ci = r % p.Cin, tap = r / p.Cin;
      const int ky = tap / 3, kx = tap % 3;
      float4 a = acc[j];
#pragma unroll 1
      for (int py = 0; py < TH; ++py) {
        const float* xr = xs + ((py + ky) * HW + kx) * p.Cin + ci;
        const float* dr = ds + py * TW * p.Cout + co;
#pragma unroll 4
        for (int px = 0; px < TW; ++px) {
          const float xv = xr[px * p.Cin];
          a = fma4(make_float4(xv, xv, xv, xv), *reinterpret_cast<const float4*>(dr + px * p.Cout), a);
        }
      }
      acc[j] = a;
      }
    }
  }
  const size_t n_el = (size_t)9 * p.Cin * p.Cout;
#pragma unroll
  for (int j = 0; j < MAX_WTASK; ++j) {
    const int task = threadIdx.x + j * NT;
    if (task < ntask) {
      const int co = (task % co4n) * 4;
      const int r = task / co4n;                                // tap * Cin + ci
      st4(p.part + (size_t)blockIdx.x * n_el + (size_t)r * p.Cout + co, acc[j]);
    }
  }
}

bool narrow_ok(int Cin, int Cout) {
  return Cin > 0 && Cin % 4 == 0 && Cin <= MAX_CIN && (Cout == 4 || Cout == 8 || Cout == 16 || Cout == 32);
}

NarrowParams make_params(int N, int H, int W, int Cin, int Cout) {
  NarrowParams p = {};
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.tiles_y = (H + TH - 1) / TH;
  p.tiles_x = (W + TW - 1) / TW;
  p.ntiles = N * p.tiles_y * p.tiles_x;
  return p;
}

constexpr int MAX_STAT_ROWS = 1024;   // forward statistics rows (the executor's partial buffer holds 2048)
constexpr int MAX_SLABS = 512;        // weight-gradient slabs

int grid_fwd(const NarrowParams& p) { return p.ntiles < MAX_STAT_ROWS ? p.ntiles : MAX_STAT_ROWS; }
int grid_wgrad(const NarrowParams& p) { return p.ntiles < MAX_SLABS ? p.ntiles : MAX_SLABS; }

#define NARROW_CHECK(fn, N, H, W, Cin, Cout)                                                                        \
  DL3P_CHECK_ARG(N > 0 && H > 0 && W > 0 && narrow_ok(Cin, Cout) &&                                                   \
                     (long long)N * H * W * (Cin > Cout ? Cin : Cout) < (1LL << 31),                                   \
                 "%s: unsupported shape (N=%d H=%d W=%d Cin=%d Cout=%d)", fn, N, H, W, Cin, Cout)

}  // namespace

extern "C" int dl3p_conv_narrow_supported(int Cin, int Cout, int k, int stride, int rate) {
  return (k == 3 && stride == 1 && rate == 1 && narrow_ok(Cin, Cout)) ? 1 : 0;
}

extern "C" int dl3p_conv_narrow_fwd(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                    const float* w, float* y, int ldy, float* stat_partials, int* rows_out, int N, int H,
                                    int W, int Cin, int Cout, void* stream) {
  NARROW_CHECK("dl3p_conv_narrow_fwd", N, H, W, Cin, Cout);
  DL3P_CHECK_ARG(x && w && y && aligned16(x) && aligned16(w) && aligned16(y) && ldx % 4 == 0 && ldx >= Cin &&
                     ldy % 4 == 0 && ldy >= Cout && !in_scale == !in_shift &&
                     (!in_scale || (aligned16(in_scale) && aligned16(in_shift))) && (!stat_partials || aligned16(stat_partials)),
                 "dl3p_conv_narrow_fwd: bad layout");
  NarrowParams p = make_params(N, H, W, Cin, Cout);
  p.x = x; p.ldx = ldx; p.scale = in_scale; p.shift = in_shift; p.act = in_act; p.w = w; p.y = y; p.ldy = ldy;
  p.part = stat_partials;
  const int grid = grid_fwd(p);
  if (rows_out) *rows_out = stat_partials ? grid : 0;
  size_t lds = (size_t)HH * HW * Cin * 4;
  if (lds < 2 * NT * 16) lds = 2 * NT * 16;
  hipLaunchKernelGGL(narrow_fwd_kernel, dim3(grid), dim3(NT), lds, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH("dl3p_conv_narrow_fwd");
  return DL3P_OK;
}

extern "C" int dl3p_conv_narrow_bwd_data(const float* dy, int lddy, const float* w, float* gx, int ldgx, int accumulate,
                                         int N, int H, int W, int Cin, int Cout, void* stream) {
  NARROW_CHECK("dl3p_conv_narrow_bwd_data", N, H, W, Cin, Cout);
  DL3P_CHECK_ARG(dy && w && gx && aligned16(dy) && aligned16(w) && aligned16(gx) && lddy % 4 == 0 && lddy >= Cout &&
                     ldgx % 4 == 0 && ldgx >= Cin,
                 "dl3p_conv_narrow_bwd_data: bad layout");
  NarrowParams p = make_params(N, H, W, Cin, Cout);
  p.dy = dy; p.lddy = lddy; p.w = w; p.y = gx; p.ldy = ldgx; p.accumulate = accumulate;
  long long grid = p.ntiles < 4096 ? p.ntiles : 4096;
  hipLaunchKernelGGL(narrow_bwd_data_kernel, dim3((unsigned)grid), dim3(NT), (size_t)HH * HW * Cout * 4, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH("dl3p_conv_narrow_bwd_data");
  return DL3P_OK;
}

extern "C" size_t dl3p_conv_narrow_bwd_weight_workspace(int N, int H, int W, int Cin, int Cout) {
  if (!narrow_ok(Cin, Cout) || N <= 0 || H <= 0 || W <= 0) return 0;
  NarrowParams p = make_params(N, H, W, Cin, Cout);
  return (size_t)grid_wgrad(p) * 9 * Cin * Cout * 4;
}

extern "C" int dl3p_conv_narrow_bwd_weight_slabs(const float* x, int ldx, const float* in_scale, const float* in_shift,
                                                 int in_act, const float* dy, int lddy, float* workspace,
                                                 size_t workspace_bytes, int* rows_out, int N, int H, int W, int Cin,
                                                 int Cout, void* stream) {
  NARROW_CHECK("dl3p_conv_narrow_bwd_weight_slabs", N, H, W, Cin, Cout);
  DL3P_CHECK_ARG(x && dy && workspace && aligned16(x) && aligned16(dy) && aligned16(workspace) && ldx % 4 == 0 &&
                     ldx >= Cin && lddy % 4 == 0 && lddy >= Cout && !in_scale == !in_shift &&
                     (!in_scale || (aligned16(in_scale) && aligned16(in_shift))),
                 "dl3p_conv_narrow_bwd_weight_slabs: bad layout");
  DL3P_CHECK_ARG(workspace_bytes >= dl3p_conv_narrow_bwd_weight_workspace(N, H, W, Cin, Cout),
                 "dl3p_conv_narrow_bwd_weight_slabs: workspace too small (%zu bytes)", workspace_bytes);
  NarrowParams p = make_params(N, H, W, Cin, Cout);
  p.x = x; p.ldx = ldx; p.scale = in_scale; p.shift = in_shift; p.act = in_act; p.dy = dy; p.lddy = lddy; p.part = workspace;
  const int grid = grid_wgrad(p);
  if (rows_out) *rows_out = grid;
  const size_t lds = ((size_t)HH * HW * Cin + (size_t)TP * Cout) * 4;
  hipLaunchKernelGGL(narrow_bwd_weight_kernel, dim3(grid), dim3(NT), lds, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH("dl3p_conv_narrow_bwd_weight_slabs");
  return DL3P_OK;
}

extern "C" int dl3p_conv_narrow_bwd_weight(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                           const float* dy, int lddy, float* gw, float* workspace, size_t workspace_bytes,
                                           int N, int H, int W, int Cin, int Cout, void* stream) {
  DL3P_CHECK_ARG(gw, "dl3p_conv_narrow_bwd_weight: gw is NULL");
  int rows = 0;
  int rc = dl3p_conv_narrow_bwd_weight_slabs(x, ldx, in_scale, in_shift, in_act, dy, lddy, workspace, workspace_bytes, &rows,
                                             N, H, W, Cin, Cout, stream);
  if (rc) return rc;
  return dl3p_reduce_rows(workspace, rows, (size_t)9 * Cin * Cout, gw, 0, stream);
}
