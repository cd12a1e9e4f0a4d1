// Nearest upsampling met at the full resolution only (Fast-SCNN, fast_scnn/models/fast_scnn.py:116-128): the fused
// Add([a, UpSampling2D(r)(b)]) with the statistics of the BatchNorm behind it, its transpose (the r x r block sum of a gradient), and
// the non-overlapping window average pooling of the pyramid pooling block (:67-83).  Memory-bound streaming kernels: 16-byte accesses,
// channel lanes fastest, 64-bit offsets, fixed summation orders (no floating-point atomics).
#include "common.h"

namespace {

int check_view(const char* fn, const char* what, const void* a, int ld, int C) {
  DL3P_CHECK_ARG(a != nullptr, "%s: %s is null", fn, what);
  DL3P_CHECK_ARG(aligned16(a), "%s: %s must be 16-byte aligned", fn, what);
  DL3P_CHECK_ARG(ld % 4 == 0 && ld >= C, "%s: bad leading dimension of %s (ld=%d, C=%d)", fn, what, ld, C);
  return DL3P_OK;
}

int check_coeffs(const char* fn, const float* scale, const float* shift) {
  DL3P_CHECK_ARG(!scale == !shift && (!scale || (aligned16(scale) && aligned16(shift))),
                 "%s: scale and shift come together, 16-byte aligned", fn);
  return DL3P_OK;
}

int check_up(const char* fn, int N, int h, int w, int C, int H, int W, int r) {
  DL3P_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C=%d must be a positive multiple of 4", fn, C);
  DL3P_CHECK_ARG(r >= 1 && r <= 8, "%s: r=%d outside 1..8", fn, r);
  DL3P_CHECK_ARG(N > 0 && h > 0 && w > 0 && (long long)H == (long long)r * h && (long long)W == (long long)r * w,
                 "%s: (H, W) = (%d, %d) is not r = %d times (h, w) = (%d, %d)", fn, H, W, r, h, w);
  return DL3P_OK;
}

unsigned grid_for(long long total) {
  long long b = (total + 255) / 256;
  const long long cap = (long long)DL3P_NUM_CUS * 16;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ------------------------------------------------------------------------------ out = pre_a(a) + pre_b(up_r(b)), with statistics
struct UpAddParams {
  const float* a; int lda; const float* asc; const float* ash; int aact;
  const float* b; int ldb; const float* bsc; const float* bsh; int bact;
  float* out; int ldo; float* partials;
  int h, w, H, W, C, r;
  long long M;                       // N * H * W
  int c4s, px, nslab, nbx;
};

// 256 threads = px pixel lanes x c4s channel lanes (pick_lanes); workgroup bx of a channel slab walks the full-resolution pixels
// bx * px + pl, + nbx * px, ... and leaves ONE partial row (sum, sum of squares of what it wrote)
__global__ __launch_bounds__(256) void upsample_add_kernel(UpAddParams p) {
  const int b = blockIdx.x;
  const int slab = b / p.nbx, bx = b - slab * p.nbx;
  const int pl = threadIdx.x / p.c4s, cl = threadIdx.x - pl * p.c4s;
  const bool active = pl < p.px;
  const int cbase4 = slab * p.c4s;
  const int c = (cbase4 + cl) * 4;
  float4 acc[2] = {zero4(), zero4()};
  if (active) {
    float4 sa = zero4(), ha = zero4(), sb = zero4(), hb = zero4();
    if (p.asc) { sa = ld4(p.asc + c); ha = ld4(p.ash + c); }
    if (p.bsc) { sb = ld4(p.bsc + c); hb = ld4(p.bsh + c); }
    for (long long m = (long long)bx * p.px + pl; m < p.M; m += (long long)p.nbx * p.px) {
      const int x = (int)(m % p.W);
      const long long t = m / p.W;
      const int y = (int)(t % p.H);
      const long long n = t / p.H;
      const size_t ml = ((size_t)n * p.h + y / p.r) * p.w + x / p.r;
      float4 va = ld4(p.a + (size_t)m * p.lda + c);
      if (p.asc) va = fma4(va, sa, ha);
      va = act_apply4(va, p.aact);
      float4 vb = ld4(p.b + ml * p.ldb + c);
      if (p.bsc) vb = fma4(vb, sb, hb);
      vb = act_apply4(vb, p.bact);
      const float4 o = add4(va, vb);
      st4(p.out + (size_t)m * p.ldo + c, o);
      acc[0] = add4(acc[0], o);
      acc[1] = fma4(o, o, acc[1]);
    }
  }
  if (p.partials) block_reduce_store<2>(acc, active, pl, cl, p.c4s, p.px, cbase4, p.C, p.partials + (size_t)bx * 2 * p.C);
}

// ------------------------------------------------------------------------------ g_low = r x r block sum of g
struct BlockSumParams {
  const float* g; int ldg; float* gl; int ldgl; int accumulate;
  int h, w, H, W, C, r;
  long long total;                   // N * h * w * (C / 4)
};

// one thread per (low-resolution pixel, 4 channels): r rows of r * ldg contiguous floats each, summed in (i, j) order
__global__ __launch_bounds__(256) void block_sum_kernel(BlockSumParams p) {
  const int c4s = p.C / 4;
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    const int c = (int)(s % c4s) * 4;
    const long long m = s / c4s;
    const int x = (int)(m % p.w);
    const long long t = m / p.w;
    const int y = (int)(t % p.h);
    const long long n = t / p.h;
    const float* src = p.g + (((size_t)n * p.H + (size_t)y * p.r) * p.W + (size_t)x * p.r) * p.ldg + c;
    float4 acc = zero4();
    for (int i = 0; i < p.r; ++i)
      for (int j = 0; j < p.r; ++j) acc = add4(acc, ld4(src + ((size_t)i * p.W + j) * p.ldg));
    float* o = p.gl + (size_t)m * p.ldgl + c;
    if (p.accumulate) acc = add4(acc, ld4(o));
    st4(o, acc);
  }
}

// ------------------------------------------------------------------------------ window average pooling
struct WinPoolParams {
  const float* x; int ldx; const float* scale; const float* shift; int act;
  float* y; int ldy;                 // forward output / backward: gradient w.r.t. the activated input
  const float* dy; int lddy; int accumulate;
  int H, W, C, kh, kw, Ho, Wo;
  long long total;
  int c4s, px, nslab;
};

__device__ __forceinline__ float4 win_in(const WinPoolParams& p, const float* px, float4 sc, float4 sh) {
  float4 v = ld4(px);
  if (p.scale) v = fma4(v, sc, sh);
  return act_apply4(v, p.act);
}

__device__ __forceinline__ float4 div4(float4 v, float d) { return make_float4(v.x / d, v.y / d, v.z / d, v.w / d); }

// windows of a few taps: one thread per (output pixel, 4 channels), taps in (ky, kx) order
__global__ __launch_bounds__(256) void winpool_fwd_small_kernel(WinPoolParams p) {
  const int c4s = p.C / 4;
  const float area = (float)(p.kh * p.kw);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    const int c = (int)(s % c4s) * 4;
    const long long m = s / c4s;
    const int ox = (int)(m % p.Wo);
    const long long t = m / p.Wo;
    const int oy = (int)(t % p.Ho);
    const long long n = t / p.Ho;
    float4 sc = zero4(), sh = zero4();
    if (p.scale) { sc = ld4(p.scale + c); sh = ld4(p.shift + c); }
    const float* src = p.x + (((size_t)n * p.H + (size_t)oy * p.kh) * p.W + (size_t)ox * p.kw) * p.ldx + c;
    float4 acc = zero4();
    for (int ky = 0; ky < p.kh; ++ky)
      for (int kx = 0; kx < p.kw; ++kx) acc = add4(acc, win_in(p, src + ((size_t)ky * p.W + kx) * p.ldx, sc, sh));
    st4(p.y + (size_t)m * p.ldy + c, div4(acc, area));
  }
}

// large windows: one workgroup per (output pixel, channel slab); pixel lane pl sums the taps pl, pl + px, ... and the lanes are
// combined in lane order
__global__ __launch_bounds__(256) void winpool_fwd_block_kernel(WinPoolParams p) {
  __shared__ float4 sm[256];
  const int pl = threadIdx.x / p.c4s, cl = threadIdx.x - pl * p.c4s;
  const bool active = pl < p.px;
  const int taps = p.kh * p.kw;
  const float area = (float)taps;
  for (long long s = blockIdx.x; s < p.total; s += gridDim.x) {      // workgroup-uniform trip count
    const int slab = (int)(s % p.nslab);
    const long long m = s / p.nslab;
    const int ox = (int)(m % p.Wo);
    const long long t = m / p.Wo;
    const int oy = (int)(t % p.Ho);
    const long long n = t / p.Ho;
    const int c = (slab * p.c4s + cl) * 4;
    float4 acc = zero4();
    if (active) {
      float4 sc = zero4(), sh = zero4();
      if (p.scale) { sc = ld4(p.scale + c); sh = ld4(p.shift + c); }
      const float* src = p.x + (((size_t)n * p.H + (size_t)oy * p.kh) * p.W + (size_t)ox * p.kw) * p.ldx + c;
      for (int tap = pl; tap < taps; tap += p.px) {
        const int ky = tap / p.kw, kx = tap - ky * p.kw;
        acc = add4(acc, win_in(p, src + ((size_t)ky * p.W + kx) * p.ldx, sc, sh));
      }
    }
    __syncthreads();
    if (active) sm[pl * p.c4s + cl] = acc;
    __syncthreads();
    if ((int)threadIdx.x < p.c4s) {
      float4 a = sm[threadIdx.x];
      for (int q = 1; q < p.px; ++q) a = add4(a, sm[q * p.c4s + threadIdx.x]);
      st4(p.y + (size_t)m * p.ldy + (size_t)(slab * p.c4s + threadIdx.x) * 4, div4(a, area));
    }
  }
}

// one thread per (input pixel, 4 channels): the one window that holds the pixel, or nothing
__global__ __launch_bounds__(256) void winpool_bwd_kernel(WinPoolParams p) {
  const int c4s = p.C / 4;
  const float area = (float)(p.kh * p.kw);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < p.total; s += (long long)gridDim.x * 256) {
    const int c = (int)(s % c4s) * 4;
    const long long m = s / c4s;
    const int ix = (int)(m % p.W);
    const long long t = m / p.W;
    const int iy = (int)(t % p.H);
    const long long n = t / p.H;
    const int oy = iy / p.kh, ox = ix / p.kw;
    const bool covered = oy < p.Ho && ox < p.Wo;
    float* o = p.y + (size_t)m * p.ldy + c;
    if (!covered) {
      if (!p.accumulate) st4(o, zero4());
      continue;
    }
    float4 g = div4(ld4(p.dy + (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.lddy + c), area);
    if (p.accumulate) g = add4(g, ld4(o));
    st4(o, g);
  }
}

int check_win(const char* fn, int N, int H, int W, int C, int kh, int kw, int Ho, int Wo) {
  DL3P_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C=%d must be a positive multiple of 4", fn, C);
  DL3P_CHECK_ARG(N > 0 && kh >= 1 && kh <= 128 && kw >= 1 && kw <= 128 && H >= kh && W >= kw && Ho == H / kh && Wo == W / kw,
                 "%s: bad dims (H=%d W=%d window %dx%d Ho=%d Wo=%d)", fn, H, W, kh, kw, Ho, Wo);
  return DL3P_OK;
}

}  // namespace

extern "C" int dl3p_upsample_add_fwd(const float* a, int lda, const float* a_scale, const float* a_shift, int a_act,
                                     const float* b, int ldb, const float* b_scale, const float* b_shift, int b_act, float* out,
                                     int ldo, float* stat_partials, int* rows_out, int N, int h, int w, int C, int H, int W,
                                     int r, void* stream) {
  const char* fn = "dl3p_upsample_add_fwd";
  int rc = check_up(fn, N, h, w, C, H, W, r);
  if (rc) return rc;
  if ((rc = check_view(fn, "a", a, lda, C)) || (rc = check_view(fn, "b", b, ldb, C)) || (rc = check_view(fn, "out", out, ldo, C)))
    return rc;
  if ((rc = check_coeffs(fn, a_scale, a_shift)) || (rc = check_coeffs(fn, b_scale, b_shift))) return rc;
  DL3P_CHECK_ARG(!stat_partials || aligned16(stat_partials), "%s: stat_partials must be 16-byte aligned", fn);
  UpAddParams p = {};
  p.a = a; p.lda = lda; p.asc = a_scale; p.ash = a_shift; p.aact = a_act;
  p.b = b; p.ldb = ldb; p.bsc = b_scale; p.bsh = b_shift; p.bact = b_act;
  p.out = out; p.ldo = ldo; p.partials = stat_partials;
  p.h = h; p.w = w; p.H = H; p.W = W; p.C = C; p.r = r;
  p.M = (long long)N * H * W;
  pick_lanes(C, &p.c4s, &p.px, &p.nslab);
  long long nbx = ceil_div_ll(p.M, p.px);
  long long target = DL3P_NUM_CUS * 4 / p.nslab;
  if (target < 1) target = 1;
  if (nbx > target) nbx = target;
  if (nbx > DL3P_MAX_STAT_ROWS) nbx = DL3P_MAX_STAT_ROWS;
  p.nbx = (int)nbx;
  if (rows_out) *rows_out = p.nbx;
  hipLaunchKernelGGL(upsample_add_kernel, dim3((unsigned)(p.nbx * p.nslab)), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_block_sum_bwd(const float* g, int ldg, float* g_low, int ldgl, int accumulate, int N, int h, int w, int C,
                                  int H, int W, int r, void* stream) {
  const char* fn = "dl3p_block_sum_bwd";
  int rc = check_up(fn, N, h, w, C, H, W, r);
  if (rc) return rc;
  if ((rc = check_view(fn, "g", g, ldg, C)) || (rc = check_view(fn, "g_low", g_low, ldgl, C))) return rc;
  BlockSumParams p = {};
  p.g = g; p.ldg = ldg; p.gl = g_low; p.ldgl = ldgl; p.accumulate = accumulate;
  p.h = h; p.w = w; p.H = H; p.W = W; p.C = C; p.r = r;
  p.total = (long long)N * h * w * (C / 4);
  hipLaunchKernelGGL(block_sum_kernel, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_winpool2d_fwd(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act, float* y,
                                  int ldy, int N, int H, int W, int C, int kh, int kw, int Ho, int Wo, void* stream) {
  const char* fn = "dl3p_winpool2d_fwd";
  int rc = check_win(fn, N, H, W, C, kh, kw, Ho, Wo);
  if (rc) return rc;
  if ((rc = check_view(fn, "x", x, ldx, C)) || (rc = check_view(fn, "y", y, ldy, C)) || (rc = check_coeffs(fn, in_scale, in_shift)))
    return rc;
  WinPoolParams p = {};
  p.x = x; p.ldx = ldx; p.scale = in_scale; p.shift = in_shift; p.act = in_act; p.y = y; p.ldy = ldy;
  p.H = H; p.W = W; p.C = C; p.kh = kh; p.kw = kw; p.Ho = Ho; p.Wo = Wo;
  if (kh * kw <= 16) {
    p.total = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(winpool_fwd_small_kernel, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  } else {
    pick_lanes(C, &p.c4s, &p.px, &p.nslab);
    p.total = (long long)N * Ho * Wo * p.nslab;
    const long long cap = (long long)DL3P_NUM_CUS * 16;
    hipLaunchKernelGGL(winpool_fwd_block_kernel, dim3((unsigned)(p.total < cap ? p.total : cap)), dim3(256), 0,
                       (hipStream_t)stream, p);
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_winpool2d_bwd(const float* dy, int lddy, float* gx, int ldgx, int accumulate, int N, int H, int W, int C,
                                  int kh, int kw, int Ho, int Wo, void* stream) {
  const char* fn = "dl3p_winpool2d_bwd";
  int rc = check_win(fn, N, H, W, C, kh, kw, Ho, Wo);
  if (rc) return rc;
  if ((rc = check_view(fn, "dy", dy, lddy, C)) || (rc = check_view(fn, "gx", gx, ldgx, C))) return rc;
  WinPoolParams p = {};
  p.y = gx; p.ldy = ldgx; p.dy = dy; p.lddy = lddy; p.accumulate = accumulate;
  p.H = H; p.W = W; p.C = C; p.kh = kh; p.kw = kw; p.Ho = Ho; p.Wo = Wo;
  p.total = (long long)N * H * W * (C / 4);
  hipLaunchKernelGGL(winpool_bwd_kernel, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}
