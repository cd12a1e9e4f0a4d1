// Pointwise (1x1) convolution = row-major GEMM on the MFMA f32 path (v_mfma_f32_16x16x4_f32) for gfx950.
//
// Replaces Conv2D(filters,(1,1)) at /root/reference deeplabv3p/models/layers.py:105,134,141,157,209,
// deeplabv3p_mobilenetv2.py:47,63, deeplabv3p_xception.py:81, deeplabv3p/model.py:75 (93-98 % of the
// model's MACs).
//
//   fwd    Y[M,N]  = act(X[M,K]*scale+shift) @ W[K,N] (+bias)      + per-channel (sum, sum^2) partials
//   dgrad  GX[M,K] (+)= DY[M,N] @ W[K,N]^T
//   wgrad  GW[K,N] = act(X*scale+shift)^T @ DY                      (split over M, slab reduce)
//
// fp32 in / fp32 accumulate is exact f32 (bitwise an fmaf chain), which the 1e-3 parity budget needs;
// it runs at 64 FLOP/clk/SIMD so the kernels are MFMA-issue bound and LDS traffic is negligible
// (one 16-B fragment read feeds four MFMAs).  Tiling is for 64-wide waves: a workgroup = 4 waves, each
// wave owns 32 rows x (16*NT) columns as 2 x NT accumulators of 16x16.  The k index inside a
// 16-deep group is permuted (lane quarter q supplies k = 4q+j at step j) so that every A fragment is ONE
// ds_read_b128; both operands use the same permutation so the sum is unchanged.
// Operands are swapped in the MFMA (D = W^T-frag x X-frag) so a lane ends up with 4 CONSECUTIVE output
// channels of one pixel: the epilogue is a single 16-B store per accumulator and the BN statistics are
// a 16-lane shuffle reduction.  Workgroups are persistent over M tiles: statistics stay in registers
// and leave as one partial row per workgroup (deterministic, no atomics); the global->LDS staging of
// the next tile is issued before the current tile's MFMAs (register double buffering) and applies the
// producer's BN+activation on the way in, so normalised activations are never materialised in HBM.
//
// This file, in order: plans (which kernel, tile and grid a launch takes), launch switches (plan -> template instantiation),
// entry points, the plan query.  The kernel templates are in pw_gemm_kernels.h / pw_wgrad_kernels.h and are instantiated here only.
#include "common.h"
#include "options.h"
#include "pw_gemm_kernels.h"
#include "pw_wgrad_kernels.h"
#include <algorithm>

// ====================================================================================== plans
// The kernel form of a launch.  The split-bf16 family's forms keep the values dl3p_gemm_plan_query reports in out6[3].
enum GemmForm {
  FORM_PIPE = 0,              // split: producer / consumer (pw_split.hip, opt-in)
  FORM_TILED = 1,             // split: two-workgroups-per-CU tiles; fp32: pw_gemm_kernel
  FORM_WIDE = 2,              // split: one 512-thread workgroup per CU
  FORM_ROW_STATIONARY = 3,    // split: pw_split_rs.hip
  FORM_PINNED = 4,            // split: pw_split3.hip
  FORM_STREAMING,             // fp32: pw_small_kernel (the whole kernel matrix in LDS)
  FORM_TINY                   // fp32: pw_tiny.hip (M <= 64 rows)
};
struct SmallShape { int kt, ntn; };
struct GemmPlan {
  GemmForm form;
  int nt, mi, wm;             // tile: 16 nt columns x 64 mi wm rows
  int gx, gy, m_tiles;
  SmallShape small;           // FORM_STREAMING: the instantiation
  bool from_table;            // a measured row of gemm_tuned.h / sb_tuned.h knows this launch
};
// What a planner has to know about the launch beyond (role, M, K, N).  The defaults are the permissive ones: every form the shape
// allows serves the launch (what dl3p_gemm_plan_query assumes).
struct GemmTraits {
  int act = DL3P_ACT_NONE;                                        // input activation
  bool has_scale = true, has_bias = false, accumulate = false;
  int pitch = 0;                                                  // row length of the pre-split kernel planes (0: K rounded up to 32)
  int ld_max = 0;                                                 // widest leading dimension of the operands
  bool b_kn = false;                                              // fp32: the kernel as stored, [K][N] (no tiny kernel, no measured tiles)
  bool tiny_ok = true, streaming_ok = true;                       // fp32: those kernels serve the launch's epilogue
};

// (reduction tiles, output tiles) instantiated for the forward / data-gradient small kernel
static bool pw_small_pick(int K, int N, SmallShape* out) {
  // measured against the tiled kernel (scripts/gemm_sweep.py): these shapes win 5-25 % at M >= 2^17 rows;
  // 2x2 (32x32), 2x16 / 16x2 and the 67600-row layers lose and stay on the tiled kernel
  static const SmallShape list[] = {{1, 2}, {2, 1}, {6, 1}, {1, 6}, {2, 3}, {3, 2}, {6, 2}, {2, 6}, {2, 9}, {9, 2}};
  static const int off = env_int("DL3P_PW_SMALL", 1) == 0;
  if (off) return false;
  const int kt = ceil_div(K, 16), ntn = ceil_div(N, 16);
  int best = -1, best_tiles = 1 << 30;
  for (int i = 0; i < (int)(sizeof(list) / sizeof(list[0])); ++i)
    if (list[i].kt >= kt && list[i].ntn >= ntn && list[i].kt * list[i].ntn < best_tiles) { best = i; best_tiles = list[i].kt * list[i].ntn; }
  if (best < 0 || best_tiles > 2 * kt * ntn) return false;
  *out = list[best];
  return true;
}

static int pw_small_grid(int M) {
  static const int per_cu = env_int("DL3P_PW_SMALL_PER_CU", 2);
  int g = ceil_div(M, 16) / (4 * 2);          // >= 2 row tiles per wave
  if (g > DL3P_NUM_CUS * per_cu) g = DL3P_NUM_CUS * per_cu;   // two resident workgroups per CU
  if (g > DL3P_MAX_STAT_ROWS) g = DL3P_MAX_STAT_ROWS;
  if (g < 1) g = 1;
  return g;
}

// Measured tile choices for the GEMM shapes of the BASELINE graphs (scripts/tune_gemm.py writes gemm_tuned.h from timings
// on an MI355X; the heuristics below serve every other shape).  role: 0 forward, 1 forward + BatchNorm statistics,
// 2 data gradient, 3 data gradient + fused BatchNorm-backward sums; M rows, K reduction length, N output columns of the
// GEMM as launched.  dl3p_set_option("gemm_nt" / "gemm_mi", v) pins a choice (v = 0: automatic) -- that is how the
// tuner tries the candidates; ("gemm_tuned", 0) ignores the table.
struct GemmTuned { int role, M, K, N, nt, mi, pc; };   // pc: persistent workgroups per CU (0 = by tile width)
struct SbPays { int role, M, K, N, pays; };
#include "gemm_tuned.h"
#include "sb_tuned.h"
static bool tuned_tables_on() { return opt(OPT_GEMM_TUNED) != 0; }
static const GemmTuned* gemm_tuned_lookup(int role, int M, int K, int N) {
  if (!tuned_tables_on()) return nullptr;
  if (role >= 5) {      // the split-bf16 kernel's rows (scripts/tune_split.py): role + 5
    for (size_t i = 0; i < sizeof(g_sb_tuned) / sizeof(g_sb_tuned[0]); ++i) {
      const GemmTuned& e = g_sb_tuned[i];
      if (e.role == role && e.M == M && e.K == K && e.N == N) return &e;
    }
    return nullptr;
  }
  for (size_t i = 0; i < sizeof(g_gemm_tuned) / sizeof(g_gemm_tuned[0]); ++i) {
    const GemmTuned& e = g_gemm_tuned[i];
    if (e.role == role && e.M == M && e.K == K && e.N == N) return &e;
  }
  return nullptr;
}
// a split-kernel row (roles 5..8 of sb_tuned.h) packs the kernel family into pc: up to 100 it is the tiled form's workgroups per CU;
// above, the wide family with wm = pc - 100, and 103 marks the row-stationary form.  Decoded here only.
struct SbTuned { bool wide, row_stationary; int nt, mi, wm, pc; };
static SbTuned sb_tuned_decode(const GemmTuned& e) {
  const bool wide = e.pc > 100;
  return {wide, e.pc == 103, e.nt, e.mi, wide ? e.pc - 100 : 1, wide ? 0 : e.pc};
}

// choose the columns-per-workgroup (NT tiles of 16) that wastes the fewest MFMA columns
static int pick_nt(int N, int M) {
  const int ntiles = ceil_div(N, 16);
  static const int cand[] = {8, 7, 6, 5, 4, 3, 2, 1};
  int best = 1;
  float best_cost = 1e30f;
  static const int nt_max = env_int("DL3P_GEMM_NT_MAX", 8);
  static const int quant = env_int("DL3P_GEMM_QUANT", 1);
  // Small grids (Xception at batch 4: M = 4356, N = 728 -> 414 workgroups of 64x128 on 256 CUs): what counts is how
  // many workgroups the busiest CU has to run, times the cost of one (fixed part ~2 column blocks + nt).  112-column
  // tiles (nt = 7) exist for this regime only: 483 workgroups of 7/8 the work instead of 414.
  const long long mt64 = ceil_div(M, 64);
  const bool small = quant && mt64 * ceil_div(ntiles, 8) <= 6LL * DL3P_NUM_CUS;
  for (int c : cand) {
    if (c > nt_max || (c == 7 && !small)) continue;
    float cost;
    if (small) {
      cost = (float)ceil_div_ll(mt64 * ceil_div(ntiles, c), DL3P_NUM_CUS) * (2.f + (float)c);
    } else {
      // MFMA columns actually computed, plus the A-tile re-reads/staging that every column block repeats
      cost = (float)(ceil_div(ntiles, c) * c) * (1.f + 1.5f / (float)c);
    }
    if (cost < best_cost) { best = c; best_cost = cost; }
  }
  return best;
}

// grid: persistent workgroups over M tiles.  Small maps (M = N*33*33) give only ~137 tiles of 128 rows,
// which quantises badly over 256 CUs; 64-row tiles (MI = 1) are used whenever 128-row tiles would leave
// the chip under two rounds of work.
static void gemm_grid(GemmPlan* pl, int M, int N, bool bn_sums = false, int force_mi = 0, int force_pc = 0) {
  const int nt = pl->nt;
  const int nb = ceil_div(N, 16 * nt);
  int mi = 2;
  if ((long long)ceil_div(M, 128) * nb < 4LL * DL3P_NUM_CUS) mi = 1;
  // Long GEMMs with wide column blocks (the decoder layers: 266256 rows, 256 / 304 columns): 64-row tiles leave room for
  // THREE resident workgroups per CU (137 VGPRs, 44 KB of LDS each) instead of two of 128 rows.  The SQ counters show
  // the two-workgroup version's waves parked on their barriers / load waits 21 % of the time and, sharing one matrix
  // pipe, in step with each other (profiles/r02_gemm_wave_state_counters.txt); a third workgroup fills those gaps:
  // 266256x304->256 forward 492 -> 455 us, data gradient 462 -> 428; 256->256 400 -> 376 / 348 -> 319 (same box).
  static const int long_rows = env_int("DL3P_GEMM_LONG_ROWS", 60000);
  static const int long_nt = env_int("DL3P_GEMM_LONG_NT", 2);
  // (not for the data gradient with the fused BatchNorm sums: its z-prefetch registers cap it at two workgroups per CU
  // either way -- forced under 168 VGPRs it spills 7-26 registers and is no faster -- and at 64 rows with two it is 6-15 %
  // slower: 537 -> 615 us in the step)
  if (M >= long_rows && nt >= long_nt && !bn_sums) mi = 1;
  int per_cu = nt <= 1 ? 6 : (nt == 2 ? 5 : (nt <= 4 ? 3 : 2));
  if (mi == 1 && per_cu < 3) per_cu = 3;
  if (force_mi) { mi = force_mi; if (mi == 1 && per_cu < 3) per_cu = 3; }
  if (force_pc) per_cu = force_pc;
  if (opt_env(OPT_GEMM_MI)) mi = opt_env(OPT_GEMM_MI);            // (the environment last: it beats the option and the table)
  if (opt_env(OPT_GEMM_PER_CU)) per_cu = opt_env(OPT_GEMM_PER_CU);
  const int bm = 64 * mi;
  const int mt = ceil_div(M, bm);
  int gx_max = (DL3P_NUM_CUS * per_cu) / nb;
  if (gx_max < 8) gx_max = 8;
  if (gx_max > DL3P_MAX_STAT_ROWS) gx_max = DL3P_MAX_STAT_ROWS;
  int g = mt;
  if (mt > gx_max) {
    const int per = ceil_div(mt, gx_max);
    g = ceil_div(mt, per);
  }
  pl->gx = g; pl->gy = nb; pl->m_tiles = mt; pl->mi = mi; pl->wm = 1;
}
// one workgroup per CU over mt row tiles (the wide and the producer / consumer forms)
static void one_per_cu_grid(GemmPlan* pl, int M, int N, int bm) {
  const int nb = ceil_div(N, 16 * pl->nt), mt = ceil_div(M, bm);
  int gxm = DL3P_NUM_CUS / nb;
  if (gxm < 1) gxm = 1;
  if (gxm > DL3P_MAX_STAT_ROWS) gxm = DL3P_MAX_STAT_ROWS;
  int g = mt;
  if (mt > gxm) g = ceil_div(mt, ceil_div(mt, gxm));
  pl->gx = g; pl->gy = nb; pl->m_tiles = mt;
}

// ---- the fp32 family: tiny / streaming / tiled.  role: 0 forward, 1 forward + BatchNorm statistics, 2 data gradient, 3 data
// gradient + fused BatchNorm-backward sums; (M, K, N) as launched.  Tile choice of the tiled kernel: the tuned table, a pinned
// option, or the heuristics
static GemmForm gemm_route(int M, int K, int N, const GemmTraits& t, SmallShape* small) {
  if (!t.b_kn && t.tiny_ok && dl3p_pw_tiny_applies(M)) return FORM_TINY;
  if (t.streaming_ok && M >= opt(OPT_PW_SMALL_MIN_ROWS) && pw_small_pick(K, N, small)) return FORM_STREAMING;
  return FORM_TILED;
}
static GemmPlan plan_gemm(int role, int M, int K, int N, const GemmTraits& t = GemmTraits()) {
  GemmPlan pl = {};
  pl.form = gemm_route(M, K, N, t, &pl.small);
  if (pl.form == FORM_TINY) { pl.gx = 1; return pl; }
  if (pl.form == FORM_STREAMING) { pl.gx = pw_small_grid(M); return pl; }
  pl.nt = pick_nt(N, M);
  if (t.b_kn) { gemm_grid(&pl, M, N); return pl; }
  int force_mi = 0, force_pc = 0;
  if (role == 3 && N <= 768 && K <= 320) {
    // the data gradient with the fused BatchNorm sums: up to 64-column blocks of 64-row tiles are the widest that fit
    // three resident workgroups per CU (147 VGPRs; wider ones need 180-256) -- what the tuner picks for 9 shapes in 10
    // of this role with a short reduction (the project convs of the inverted residuals: K = 24..256), 20-34 % faster
    // than the widest-block choice on the 17424-row layers.  Long reductions (Xception: K = 728..2048 on 4356 rows) pay
    // more for re-staging A per column block than the third workgroup returns: they keep the wide blocks.
    int best = 4, waste = 1 << 30;
    for (int c = 4; c >= 2; --c) {
      const int w = ceil_div(N, 16 * c) * 16 * c - N;
      if (w < waste) { waste = w; best = c; }
    }
    if (ceil_div(N, 16) < best) best = ceil_div(N, 16);
    pl.nt = best;
    force_mi = 1;
  }
  if (const GemmTuned* e = gemm_tuned_lookup(role, M, K, N)) { pl.nt = e->nt; force_mi = e->mi; force_pc = e->pc; pl.from_table = true; }
  if (opt_set(OPT_GEMM_NT)) pl.nt = opt_set(OPT_GEMM_NT);
  if (opt_set(OPT_GEMM_MI)) force_mi = opt_set(OPT_GEMM_MI);
  if (opt_set(OPT_GEMM_PER_CU)) force_pc = opt_set(OPT_GEMM_PER_CU);
  gemm_grid(&pl, M, N, role == 3, force_mi, force_pc);
  return pl;
}

// ---- the split-bf16 family (pw_split*.hip): pinned / row-stationary / producer-consumer / wide / tiled
extern "C" int dl3p_pwconv_sb_pays(int role, int M, int K, int N) {
  // measured verdict for this exact launch (csrc/sb_tuned.h): 1 the split kernel is faster than the fp32-input MFMA kernel,
  // 0 it is not, -1 never measured (or the tables are switched off) -- the caller's threshold rule decides
  if (!tuned_tables_on()) return -1;
  for (size_t i = 0; i < sizeof(g_sb_pays) / sizeof(g_sb_pays[0]); ++i) {
    const SbPays& e = g_sb_pays[i];
    if (e.role == role && e.M == M && e.K == K && e.N == N) return e.pays;
  }
  return -1;
}

// another form of the split kernel is pinned by an option
static bool sb_form_pinned() { return opt_set(OPT_SB_WM) != 0 || opt(OPT_SB_PIPE) > 0 || opt_set(OPT_GEMM_NT) || opt_set(OPT_GEMM_MI); }

// the row-stationary form (pw_split_rs.hip): pinned by dl3p_set_option("sb_rs", 1), otherwise by the measured table or the rule below
static bool sb_rs_route(int role, int M, int K, int N) {
  if (!dl3p_sb_rs_supported(role, M, K, N) || sb_form_pinned()) return false;
  if (opt_set(OPT_SB_RS) >= 0) return opt_set(OPT_SB_RS) == 1;
  if (opt_env(OPT_SB_RS) >= 0) return opt_env(OPT_SB_RS) != 0;
    // the measured table (csrc/sb_tuned.h, {2, 1, 103} rows) decides where it knows the launch; elsewhere the rule measured on the
    // decoder shapes (scripts/micro/sb_rs.py, profiles/r04_split_gemm_row_stationary.txt): long data gradients with a reduction of
    // 225-320 -- with the fused BatchNorm-backward sums 362 against 494-512 us on 266256 x 256 -> 304, 288 against 340 onto 256
    // columns, 175 against 216 at 131072 rows; plain 258 against 345, 213 against 234, 120 against 146.  Forwards tie (247 against
    // 255 at K = 256) or lose (K = 304: 372 against 349), as does everything under ~10^5 rows (one workgroup per CU and 64-row half
    // tiles: tile quantisation)
  static const int fwd = env_int("DL3P_SB_RS_FWD", 0);      // (A/B switch: forwards too)
  if (fwd && role <= 1 && M >= 131072 && K > 224) return true;
  if (const GemmTuned* e = gemm_tuned_lookup(role + 5, M, K, N)) return sb_tuned_decode(*e).row_stationary;
  return role >= 2 && M >= 131072 && K > 224;
}

static bool sb3_debug() {
  static const bool on = getenv("DL3P_SB3_DEBUG") != nullptr;
  return on;
}
// the pinned-schedule form (pw_split3.hip): forwards onto 256 columns from 65536 rows up whose reduction is 8, 10, 12 ... K-steps
// long.  dl3p_set_option("sb3", 1) takes it wherever it is supported, 0 never, -1 (default) by the rule -- unless the measured
// table knows the launch.  A launch whose activation / bias / pitch / leading dimension the form does not serve is refused here:
// the tiled kernels take it.
static bool sb3_route(int role, int M, int K, int N, const GemmTraits& t) {
  const int sb3 = opt(OPT_SB3), pitch = (K + 31) / 32 * 32;
  if (sb3 == 0 || !dl3p_sb3_supported(role, M, K, N, pitch, DL3P_ACT_NONE, true, false, false, 0)) return false;
  if (sb3 != 1) {
    if (sb_form_pinned() || opt_set(OPT_SB_RS) == 1) return false;       // another form is pinned
    if (gemm_tuned_lookup(role + 5, M, K, N) || M < 65536) return false;
  }
  if (dl3p_sb3_supported(role, M, K, N, t.pitch ? t.pitch : pitch, t.act, t.has_scale, t.accumulate, t.has_bias, t.ld_max)) return true;
  if (sb3_debug())
    fprintf(stderr, "dl3p_pwconv_fwd_sb: pinned form vetoed (M=%d K=%d N=%d pitch=%d act=%d scale=%d bias=%d stats=%d)\n", M, K, N,
            t.pitch ? t.pitch : pitch, t.act, t.has_scale, t.has_bias, role == 1);
  return false;
}

// Wide tiles (one workgroup per CU: 128 or 256 rows x up to 256 columns, the A tile split once for all of N) where there are
// enough row tiles to go round; otherwise the 2-workgroups-per-CU tiles of the fp32 kernel.
static GemmPlan plan_gemm_sb(int role, int M, int K, int N, const GemmTraits& t = GemmTraits()) {
  GemmPlan pl = {};
  const GemmTuned* e = gemm_tuned_lookup(role + 5, M, K, N);      // roles 5..8 (csrc/sb_tuned.h)
  pl.from_table = e != nullptr;
  pl.wm = 1;
  if (sb3_route(role, M, K, N, t)) {
    pl.form = FORM_PINNED; pl.nt = 16; pl.mi = 2; pl.gx = dl3p_sb3_grid(M); pl.gy = 1; pl.m_tiles = ceil_div(M, 128);
    return pl;
  }
  if (sb_rs_route(role, M, K, N)) {
    pl.form = FORM_ROW_STATIONARY; pl.nt = 2; pl.mi = 1; pl.gx = dl3p_sb_rs_grid(M); pl.gy = 1; pl.m_tiles = ceil_div(M, 64);
    return pl;
  }
  const int pin_nt = opt_set(OPT_GEMM_NT), pin_mi = opt_set(OPT_GEMM_MI), pin_wide = opt_set(OPT_SB_WM);
  pl.nt = pick_nt(N, M);
  if (opt(OPT_SB_PIPE) && pin_wide <= 0) {      // measured slower than the symmetric form: opt-in
    // producer / consumer form: one 512-thread workgroup per CU, 128 (or 64) rows x up to 128 columns
    pl.form = FORM_PIPE;
    if (pl.nt > 8) pl.nt = 8;
    if (pin_nt) pl.nt = pin_nt > 8 ? 8 : pin_nt;
    pl.mi = pin_mi ? pin_mi : (M >= 4096 ? 2 : 1);
    one_per_cu_grid(&pl, M, N, 64 * pl.mi);
    return pl;
  }
  // measured (scripts/micro/sb_gemm.py, profiles/r03_split_gemm.txt): 128-row tiles with the widest column block win on every
  // shape with a few thousand rows or more (the fp32 kernel's 64-row / three-workgroup choice for long GEMMs loses here: two A
  // register sets); with the fused BatchNorm sums 128 x 64, the widest that does not spill.  The one-workgroup-per-CU wide tiles
  // (sb_wm) pay on long forwards onto 256-column layers only (below); elsewhere they tie or lose and stay opt-in.
  int force_mi = 0, force_pc = 0;
  if (M >= 4096) force_mi = 2;
  if (role == 3 && N > 64) { pl.nt = 4; force_mi = 2; }
  int wide_nt = 0, wide_mi = 2, wide_wm = 1;
  bool wide_bnb = false;
  if (e) {
    const SbTuned d = sb_tuned_decode(*e);
    if (d.wide) { wide_nt = d.nt; wide_mi = d.mi; wide_wm = d.wm; wide_bnb = true; }
    else { pl.nt = d.nt; force_mi = d.mi; force_pc = d.pc; }
  }
  // long forwards onto 256-column layers: 128 rows x 256 columns, 512 threads, one workgroup per CU (the A tile is split once for
  // all of N): 306 against 335 us on 266256 x 304 -> 256, 255 against 278 on K = 256, 98 against 107 on 74498 rows -- since the
  // operand requests stopped being drained at every stage (pw_split.hip, the note in step()); before that the wide tiles tied
  if (!e && role <= 1 && N % 256 == 0 && M >= 65536) { wide_nt = 16; wide_mi = 1; wide_wm = 2; }
  // the long decoder data gradients with the fused BatchNorm sums: 256 rows x 128 columns, 512 threads (334 against 368 us on
  // 266256 x 256 -> 256, 469 against 495 onto 304 columns; the 256-column tiles lose here -- the z tile of the sums comes on top)
  if (!e && role == 3 && N >= 256 && M >= 131072) { wide_nt = 8; wide_mi = 2; wide_wm = 2; wide_bnb = true; }
  if (pin_wide > 0) { wide_nt = opt_set(OPT_SB_NT) ? opt_set(OPT_SB_NT) : 16; wide_wm = pin_wide; wide_mi = pin_mi ? pin_mi : 2; }
  if (pin_wide < 0) wide_nt = 0;
  if (wide_nt && dl3p_sb_wide_config(wide_nt, wide_mi, wide_wm) && (role != 3 || wide_bnb || pin_wide > 0)) {     // (role 3 takes the wide family only where measured -- above -- or pinned)
    pl.form = static_cast<GemmForm>(wide_wm);      // (FORM_TILED | FORM_WIDE are wm 1 | 2 by value: the wide family's wm = 1 tiles report as tiled, as they always have)
    pl.nt = wide_nt; pl.mi = wide_mi; pl.wm = wide_wm;
    one_per_cu_grid(&pl, M, N, 64 * wide_mi * wide_wm);
    return pl;
  }
  pl.form = FORM_TILED;
  if (pin_nt) pl.nt = pin_nt;
  if (pin_mi) force_mi = pin_mi;
  if (opt_set(OPT_GEMM_PER_CU)) force_pc = opt_set(OPT_GEMM_PER_CU);
  if (pl.nt > 8) pl.nt = 8;
  gemm_grid(&pl, M, N, role == 3, force_mi, force_pc);
  // 128-row tiles with the fused BatchNorm sums spill from 80 columns up (two A register sets + the z prefetch)
  if (role == 3 && pl.mi == 2 && pl.nt > 4) gemm_grid(&pl, M, N, true, 1, force_pc);
  return pl;
}

// the gathered-conv variant (dense convs as implicit GEMMs on the split kernel): tiled only
static GemmPlan plan_gemm_sb_ga(int M, int N) {
  GemmPlan pl = {};
  pl.form = FORM_TILED;
  pl.nt = pick_nt(N, M);
  if (pl.nt > 8) pl.nt = 8;
  if (opt_set(OPT_GEMM_NT)) pl.nt = opt_set(OPT_GEMM_NT) > 8 ? 8 : opt_set(OPT_GEMM_NT);
  // (128-row tiles with the gather's index registers spill from 96 columns up: 64-row tiles there)
  gemm_grid(&pl, M, N, false, opt_set(OPT_GEMM_MI) ? opt_set(OPT_GEMM_MI) : ((M >= 4096 && pl.nt < 6) ? 2 : 1), opt_set(OPT_GEMM_PER_CU));
  return pl;
}

// the pinned-schedule data gradient with the folded BatchNorm-backward apply
static bool sb3d_takes(int M, int K, int N, int pitch, int bn_act, int front_act, bool bnb, bool accumulate, int ld_max) {
  // OPT-IN by rule (DL3P_SB3_DGRAD=1; dl3p_set_option("sb3", 1) takes it wherever it is supported): measured on MI355X the pinned form
  // is 7-12 % faster than the row-stationary kernel without the fused sums (263-300 against 281-340 us on 262144-266256 rows) and
  // level with it with them (346-396 against 343-426), and the headline step does not move (11.87 ms either way): this launch moves
  // 1.09-1.36 GB (g, z, dz, gx and the front layer's z) -- 240-300 us at the 4.5-5 TB/s such kernels reach -- so it is bound by HBM,
  // not by the matrix pipe (scripts/micro/sb3d_bench.py)
  static const int sb3d = env_int("DL3P_SB3_DGRAD", 0);
  const int sb3 = opt(OPT_SB3);
  if (sb3 == 0 || !dl3p_sb3d_supported(M, K, N, pitch, bn_act, front_act, bnb, accumulate, ld_max)) return false;
  return sb3 == 1 || (sb3d && M >= 65536);
}

// ---- split-K forward
// Few rows and a long reduction (Xception's / ResNet50's ASPP at a 33 x 33 map: 4356 x 2048 -> 256) give the tiled kernel 34 row
// tiles for 256 CUs: with 32-column blocks (its best, 552 workgroups) every workgroup re-reads its 64 x 2048 slice of A for a
// quarter of the output width and the launch runs at a third of the fp32 matrix rate.  Here the REDUCTION is cut into slices of
// >= 256: 64 x 128 tiles x ~5 slices fill the chip with workgroups that each stream a 64 x 416 panel of A once; the slices leave
// slabs [S][M][N] in a workspace and splitk_finish_kernel adds them in slice order (+ bias) and takes the BatchNorm statistic rows
// from the finished output.  Deterministic; the sum is associated differently from the one-launch kernel (equal to rounding).
// (The same slices on the split-bf16 kernel were measured at 52.8-55.3 us against 59.0 here for 4356 x 2048 -> 256, 39.4-39.9 against
// 41.2 at K = 1280 -- both forms are bound by the latency of their 13 K-steps per tile, not by the matrix pipe -- and are not built in.)
// -> slices (0: the one-launch kernel)
extern "C" int dl3p_pwconv_fwd_splitk_plan(int M, int K, int N) {
  const int force = opt_set(OPT_SPLITK);      // (DL3P_SPLITK=0: never -- an A/B switch that counts while the option is negative)
  if (force == 0 || (force < 0 && opt_env(OPT_SPLITK) == 0)) return 0;
  if (!(N == 128 || N == 256 || N == 512) || K % 4 || K < 512 || M < 1024) return 0;
  if ((unsigned long long)M * (unsigned long long)K * 4ull >= (1ull << 32)) return 0;
  // measured (scripts/micro/splitk_bench.py, 64 x 128 tiles): 4356 x 2048 -> 256: one launch 93.8 us, 5 slices 59.8 (8: 64.6, 10: 62.4,
  // 4: 69.5); 4356 x 1280: 55.2 -> 41.1 (4: 46.7, 8: 46.2); 8712 x 2048: 131.5 -> 102.5;
  // 17424 x 2048 (546 tiles): 226.9 -> 182.7 (4: 183.8, 2: 196.9, 8: 197.5), x 1280: 143.9 -> 124.3-127.9.  Five slices are the best
  // or within 3 % of it at every size measured; rule: five (slices of at least 256) for up to 640 tiles of 64 x 128.
  const int tiles = ceil_div(M, 64) * ceil_div(N, 128);
  if (force < 0 && (tiles > 640 || K < 1024)) return 0;
  int S = force > 0 ? force : 5;
  S = std::min(S, std::min(16, K / 256));
  while (S > 1 && ceil_div(ceil_div(K, S), 32) * 32 * (S - 1) >= K) --S;   // every slice owns at least one column
  return S > 1 ? S : 0;
}
extern "C" size_t dl3p_pwconv_fwd_splitk_workspace(int M, int K, int N) {
  const int S = dl3p_pwconv_fwd_splitk_plan(M, K, N);
  return S ? sizeof(float) * (size_t)S * M * N : 0;
}

// ---- weight gradient: tiny / streaming / split-bf16 / tiled
enum WgradForm { WGRAD_TILED = 0, WGRAD_STREAMING = 1, WGRAD_TINY = 2, WGRAD_SPLIT = 4 };      // (as dl3p_gemm_plan_query reports them in out6[0])
struct WgradPlan {
  WgradForm form;
  int slabs;                                          // of the form taken (tiny: none)
  bool has_small; SmallShape small; int small_grid;   // the streaming kernel's instantiation for (K, N), if there is one
  int kw, nw, ktiles, ntiles, mchunk, tiled_slabs;    // the tiled kernel's plan (always filled in): tile (64 kw) x (16 nw)
  int pin_per_cu; bool from_table;                    //   workgroups per CU pinned by the option or the table (0: the default)
  int sb_slabs, kf, sb_nw, sb_ktiles, sb_ntiles, mrows;      // the split kernel's plan (sb_slabs = 0: it does not take the launch)
};
struct WgradTraits {
  size_t max_slabs = DL3P_MAX_STAT_ROWS;              // what the caller's workspace holds
  bool tiny_ok = true, streaming_ok = true, split_ok = true;
  bool gathered = false;                              // dense conv: X gathered while it is staged (split or tiled only)
};

// workgroups for the small-K.N kernel (all resident at once)
static int wgrad_small_grid(int M, int KT, int NTN) {
  const int tiles = ceil_div(M, 16);
  // measured (kernel + slab reduce): two workgroups per CU stream as fast as four and halve the slabs;
  // below two row tiles per wave the per-wave prologue / reduction dominates
  static const int occ_env = env_int("DL3P_WGRAD_SMALL_PER_CU", 2);
  const int occ = occ_env, tpw = 2;
  (void)KT; (void)NTN;
  int g = tiles / (4 * tpw);
  if (g > DL3P_NUM_CUS * occ) g = DL3P_NUM_CUS * occ;
  if (g > DL3P_MAX_STAT_ROWS) g = DL3P_MAX_STAT_ROWS;
  if (g < 1) g = 1;
  return g;
}

// the (KT, NTN) instantiations: kernels of the 513x513 MobileNetV2 / V3 / Xception graphs at OS 2-8
static bool wgrad_small_pick(int K, int N, SmallShape* out) {
  static const SmallShape list[] = {{1, 2}, {2, 1}, {2, 2}, {1, 6}, {2, 3}, {2, 4}, {4, 2}, {6, 2}, {2, 6}, {2, 9}, {9, 2},
                                    {2, 12}, {12, 2}, {4, 4}};
  static const int off = env_int("DL3P_WGRAD_SMALL", 1) == 0;
  if (off) return false;
  const int kt = ceil_div(K, 16), ntn = ceil_div(N, 16);
  int best = -1, best_tiles = 1 << 30;
  for (int i = 0; i < (int)(sizeof(list) / sizeof(list[0])); ++i)
    if (list[i].kt >= kt && list[i].ntn >= ntn && list[i].kt * list[i].ntn < best_tiles) { best = i; best_tiles = list[i].kt * list[i].ntn; }
  if (best < 0 || best_tiles > 2 * kt * ntn) return false;   // too much padding: use the tiled kernel
  *out = list[best];
  return true;
}

// tile shape (KW, NW) -> (64 KW) x (16 NW): fewest padded MFMA columns, weighted by the operand re-reads; then the slices of M
static void wgrad_tiled_plan(WgradPlan* pl, int M, int K, int N) {
  static const int cand[4][2] = {{1, 4}, {2, 4}, {1, 8}, {2, 8}};
  // role 4 of the measured table: nt = tile index (0: 64x64, 1: 128x64, 2: 64x128, 3: 128x128), mi = workgroups per CU
  const GemmTuned* e = gemm_tuned_lookup(4, M, K, N);
  pl->from_table = e != nullptr;
  int force = opt_env(OPT_WGRAD_TILE);
  if (e) force = e->nt;
  if (opt_set(OPT_WGRAD_TILE) >= 0) force = opt_set(OPT_WGRAD_TILE);
  // measured: larger tiles pay only when M is large (decoder layers: 64 x 128 is 8-10 % faster than 64 x 64);
  // on the 17424-row layers they cut the number of workgroups too far
  pl->kw = 1; pl->nw = 4;
  if (force >= 0 || M >= 65536) {
    float best = 1e30f;
    for (int i = 0; i < 4; ++i) {
      if (force >= 0 && i != force) continue;
      const int tk = 64 * cand[i][0], tn = 16 * cand[i][1];
      const float area = (float)(ceil_div(K, tk) * tk) * (float)(ceil_div(N, tn) * tn);
      const float cost = area * (1.f + 0.5f * (64.f / tk + 64.f / tn));
      if (cost < best) { best = cost; pl->kw = cand[i][0]; pl->nw = cand[i][1]; }
    }
  }
  pl->ktiles = ceil_div(K, 64 * pl->kw);
  pl->ntiles = ceil_div(N, 16 * pl->nw);
  const int tiles = pl->ktiles * pl->ntiles;
  int per_cu = opt_env(OPT_WGRAD_PER_CU);
  if (e) per_cu = e->mi;
  if (opt_set(OPT_WGRAD_PER_CU)) per_cu = opt_set(OPT_WGRAD_PER_CU);
  pl->pin_per_cu = opt_set(OPT_WGRAD_PER_CU) ? opt_set(OPT_WGRAD_PER_CU) : (e ? e->mi : 0);
  int s = (DL3P_NUM_CUS * per_cu) / tiles;
  if (s < 1) s = 1;
  int max_s = ceil_div(M, 256);          // at least 256 rows per slice
  if (s > max_s) s = max_s;
  if (s > DL3P_MAX_STAT_ROWS) s = DL3P_MAX_STAT_ROWS;
  int chunk = ceil_div(ceil_div(M, s), 32) * 32;
  pl->tiled_slabs = ceil_div(M, chunk);
  pl->mchunk = chunk;
}

extern "C" int dl3p_conv2d_gemm_sb_pays(int role, int M, int K, int N);
// does this weight gradient run on the split-bf16 kernel?  -> sb_slabs (0: no) + its plan.  The measured verdict / tile of this exact
// launch where there is one (csrc/sb_tuned.h: g_sb_pays role 4, g_sb_tuned role 9 {tile, workgroups per CU}), else the rule
static void wgrad_sb_route(WgradPlan* pl, int M, int K, int N, const WgradTraits& t) {
  int tile = opt_set(OPT_SPLIT_WGRAD_TILE), per_cu = opt_set(OPT_SPLIT_WGRAD_PER_CU);
  if (t.gathered) {
    if (!dl3p_conv2d_gemm_sb_pays(4, M, K, N)) return;
    if (tile == 4) tile = 0;      // (the gathered-operand instantiations stop at 128 x 128: a pinned 128 x 256 tile means 128 x 128 here)
  } else {
    if (opt(OPT_SPLIT_WGRAD) <= 0) return;      // follows the switch of the split forward / data-gradient GEMMs unless set itself
    if (tile < 0 && per_cu <= 0) {
      const int pays = dl3p_pwconv_sb_pays(4, M, K, N);
      if (pays == 0 || (pays < 0 && (K < 128 || N < 128 || M < 16384))) return;
      if (const GemmTuned* e = gemm_tuned_lookup(9, M, K, N)) { tile = e->nt; per_cu = e->mi; }
    }
  }
  const int max_slabs = (int)std::min(t.max_slabs, (size_t)DL3P_MAX_STAT_ROWS);
  pl->sb_slabs = dl3p_wgrad_sb_plan(M, K, N, max_slabs, tile, per_cu, &pl->kf, &pl->sb_nw, &pl->sb_ktiles, &pl->sb_ntiles, &pl->mrows);
}

static WgradPlan plan_wgrad(int M, int K, int N, const WgradTraits& t = WgradTraits()) {
  WgradPlan pl = {};
  wgrad_tiled_plan(&pl, M, K, N);
  pl.has_small = !t.gathered && wgrad_small_pick(K, N, &pl.small);
  if (pl.has_small) pl.small_grid = wgrad_small_grid(M, pl.small.kt, pl.small.ntn);
  if (!t.gathered && t.tiny_ok && dl3p_pw_tiny_applies(M)) { pl.form = WGRAD_TINY; return pl; }
  if (M >= 16 && pl.has_small && t.streaming_ok) { pl.form = WGRAD_STREAMING; pl.slabs = pl.small_grid; return pl; }
  if (t.split_ok) wgrad_sb_route(&pl, M, K, N, t);
  pl.form = pl.sb_slabs > 0 ? WGRAD_SPLIT : WGRAD_TILED;
  pl.slabs = pl.sb_slabs > 0 ? pl.sb_slabs : pl.tiled_slabs;
  return pl;
}
// slabs the workspace must hold: whatever a launch of this shape may take (the streaming kernel wherever it has an instantiation)
static size_t wgrad_workspace_slabs(int M, int K, int N, bool gathered) {
  WgradTraits t;
  t.tiny_ok = false; t.gathered = gathered;
  const WgradPlan pl = plan_wgrad(M, K, N, t);
  return pl.has_small ? (size_t)pl.small_grid : (size_t)std::max(pl.tiled_slabs, pl.sb_slabs);
}

// ====================================================================================== launch switches
template <int KT, int NTN, bool STATS, bool BNB = false>
static void launch_pw_small(const GemmParams& p, int grid, hipStream_t st) {
  constexpr size_t lds = pw_small_lds<KT, NTN, BNB>();
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)pw_small_kernel<KT, NTN, STATS, BNB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  dl3p_launch(pw_small_kernel<KT, NTN, STATS, BNB>, dim3(grid), dim3(256), lds, st, p);
}

template <bool STATS, bool BNB = false>
static void launch_pw_small_any(const GemmParams& p, SmallShape sh, int grid, hipStream_t st) {
#define DL3P_PS(a, b) if (sh.kt == a && sh.ntn == b) { launch_pw_small<a, b, STATS, BNB>(p, grid, st); return; }
  DL3P_PS(1, 2) DL3P_PS(2, 1) DL3P_PS(6, 1) DL3P_PS(1, 6) DL3P_PS(2, 3) DL3P_PS(3, 2) DL3P_PS(6, 2) DL3P_PS(2, 6)
  DL3P_PS(2, 9) DL3P_PS(9, 2)
#undef DL3P_PS
}

template <int NT, bool B_KN, bool STATS, int MI, int BKT, bool BNB = false, bool GA = false>
static void launch_gemm_one(const GemmParams& p, dim3 grid, hipStream_t st) {
  constexpr int BM = 64 * MI, BN = 16 * NT, AP = BKT + 4;
  constexpr int BS = B_KN ? BKT * (BN + 4) : BN * AP;
  constexpr int TPP = NT < 4 ? NT : 4;
  constexpr int ES = 4 * 16 * MI * (16 * TPP + 4);
  constexpr int OPER = BM * AP + BS;
  constexpr int RED = STATS ? 2 * 4 * BN : 0;
  constexpr size_t lds = sizeof(float) * (size_t)((BKT > 32 ? (OPER > ES ? OPER : ES) : OPER + ES) + RED);
  static bool attr_set = false;
  if (!attr_set) {
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)pw_gemm_kernel<NT, B_KN, STATS, MI, BKT, BNB, GA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  dl3p_launch(pw_gemm_kernel<NT, B_KN, STATS, MI, BKT, BNB, GA>, grid, dim3(256), lds, st, p);
}

template <bool B_KN, bool STATS, int MI, int BKT, bool BNB = false, bool GA = false>
static void launch_gemm_mi(const GemmParams& p, int nt, dim3 grid, hipStream_t st) {
  switch (nt) {
    case 1: launch_gemm_one<1, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    case 2: launch_gemm_one<2, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    case 3: launch_gemm_one<3, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    case 4: launch_gemm_one<4, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    case 5: launch_gemm_one<5, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    case 6: launch_gemm_one<6, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    case 7: launch_gemm_one<7, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
    default: launch_gemm_one<8, B_KN, STATS, MI, BKT, BNB, GA>(p, grid, st); break;
  }
}

template <bool B_KN, bool STATS, bool BNB = false, bool GA = false>
static void launch_gemm(const GemmParams& p_in, int nt, int mi, dim3 grid, hipStream_t st) {
  GemmParams p = p_in;
  // (BKT = 64 -- half the barriers and staging passes per MFMA -- was measured neutral on the decoder layers and is
  // not instantiated: the loop is bound by matrix-pipe sharing between the two resident workgroups)
  if (mi == 1) launch_gemm_mi<B_KN, STATS, 1, 32, BNB, GA>(p, nt, grid, st);
  else launch_gemm_mi<B_KN, STATS, 2, 32, BNB, GA>(p, nt, grid, st);
}

template <int KT, int NTN, bool BNA = false>
static void launch_wgrad_small(const WgradParams& p, int grid, hipStream_t st) {
  constexpr size_t lds = wgrad_small_lds<KT, NTN, BNA>();
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)pw_wgrad_small_kernel<KT, NTN, BNA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  dl3p_launch(pw_wgrad_small_kernel<KT, NTN, BNA>, dim3(grid), dim3(256), lds, st, p);
}

template <bool BNA = false>
static void launch_wgrad_small_any(const WgradParams& p, SmallShape sh, int grid, hipStream_t st) {
#define DL3P_WS(a, b) if (sh.kt == a && sh.ntn == b) { launch_wgrad_small<a, b, BNA>(p, grid, st); return; }
  DL3P_WS(1, 2) DL3P_WS(2, 1) DL3P_WS(2, 2) DL3P_WS(1, 6) DL3P_WS(2, 3) DL3P_WS(2, 4) DL3P_WS(4, 2) DL3P_WS(6, 2)
  DL3P_WS(2, 6) DL3P_WS(2, 9) DL3P_WS(9, 2) DL3P_WS(2, 12) DL3P_WS(12, 2) DL3P_WS(4, 4)
#undef DL3P_WS
}

template <bool GX = false, bool BNA = false>
static void launch_wgrad_tiled(const WgradParams& p, const WgradPlan& pl, hipStream_t st) {
  const int kw = pl.kw, nw = pl.nw;
  const dim3 grid(p.ktiles * p.ntiles, pl.tiled_slabs), block(256);
  if (kw == 1 && nw == 4) dl3p_launch(pw_wgrad_kernel<1, 4, GX, BNA>, grid, block, 0, st, p);
  else if (kw == 2 && nw == 4) dl3p_launch(pw_wgrad_kernel<2, 4, GX, BNA>, grid, block, 0, st, p);
  else if (kw == 1 && nw == 8) dl3p_launch(pw_wgrad_kernel<1, 8, GX, BNA>, grid, block, 0, st, p);
  else dl3p_launch(pw_wgrad_kernel<2, 8, GX, BNA>, grid, block, 0, st, p);
}

// a planned split-bf16 launch
static int launch_plan_sb(const char* fn, const GemmParams& p, const GemmPlan& pl, bool stats, bool bnb, hipStream_t st) {
  switch (pl.form) {
    case FORM_PINNED:
      DL3P_CHECK_ARG(dl3p_launch_gemm_sb3(p, stats, pl.gx, st), "%s: no pinned-schedule instantiation for activation %d", fn, p.act);
      break;
    case FORM_ROW_STATIONARY:
      DL3P_CHECK_ARG(dl3p_launch_gemm_sbr(p, bnb ? 2 : (stats ? 1 : 0), pl.gx, st), "%s: no row-stationary instantiation for K=%d", fn, p.K);
      break;
    case FORM_PIPE: dl3p_launch_gemm_sbp(p, stats, bnb, pl.nt, pl.mi, dim3(pl.gx, pl.gy), st); break;
    default: dl3p_launch_gemm_sb(p, stats, bnb, false, pl.nt, pl.mi, pl.wm, dim3(pl.gx, pl.gy), st); break;
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// ---- small helper kernels
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float* __restrict__ slabs, int S, const float* __restrict__ bias,
                                                            float* __restrict__ y, int ldy, float* __restrict__ partials, int M,
                                                            int N, int rows_per_wg) {
  __shared__ float red[2][256 * 4];
  const int c4n = N / 4;                       // float4 columns per row; 256 % c4n == 0 (host)
  const int rpp = 256 / c4n;                   // rows per pass of the workgroup
  const int c4 = threadIdx.x % c4n, rg = threadIdx.x / c4n;
  const int r0 = blockIdx.x * rows_per_wg;
  float4 s = zero4(), ss = zero4();
  float4 b4 = zero4();
  if (bias) b4 = ld4(bias + c4 * 4);
  for (int r = r0 + rg; r < min(r0 + rows_per_wg, M); r += rpp) {
    float4 acc = ld4(slabs + ((size_t)r * N + c4 * 4));
    for (int z = 1; z < S; ++z) acc = add4(acc, ld4(slabs + (((size_t)z * M + r) * N + c4 * 4)));
    acc = add4(acc, b4);
    st4(y + (size_t)r * ldy + c4 * 4, acc);
    s = add4(s, acc);
    ss.x = fmaf(acc.x, acc.x, ss.x); ss.y = fmaf(acc.y, acc.y, ss.y); ss.z = fmaf(acc.z, acc.z, ss.z); ss.w = fmaf(acc.w, acc.w, ss.w);
  }
  if (!partials) return;
  *reinterpret_cast<float4*>(&red[0][threadIdx.x * 4]) = s;
  *reinterpret_cast<float4*>(&red[1][threadIdx.x * 4]) = ss;
  __syncthreads();
  if (rg == 0) {
    float4 a = zero4(), b = zero4();
    for (int g = 0; g < rpp; ++g) {
      a = add4(a, *reinterpret_cast<const float4*>(&red[0][(g * c4n + c4) * 4]));
      b = add4(b, *reinterpret_cast<const float4*>(&red[1][(g * c4n + c4) * 4]));
    }
    st4(partials + ((size_t)blockIdx.x * 2) * N + c4 * 4, a);
    st4(partials + ((size_t)blockIdx.x * 2 + 1) * N + c4 * 4, b);
  }
}

// dst[off + n*K + k] = src[off + k*N + n] for every (off, K, N) row of `table` (device, int[n][4]): the transposed
// copies of all pointwise kernels in the flat parameter buffer, refreshed once per optimiser step
// 64 x 64 tiles (round 5; 32 x 32 before: 128-byte row segments each way, 2.3 TB/s on Xception's 164 MB of kernels): a wave reads and
// writes 256 contiguous bytes per instruction, all sixteen loads of a thread before the first LDS store; clamped addresses, no load in a
// branch
__global__ __launch_bounds__(256) void transpose_batch_kernel(const float* src, float* dst, const int* table) {
  __shared__ float tile[64][65];
  const int off = table[blockIdx.x * 4], K = table[blockIdx.x * 4 + 1], N = table[blockIdx.x * 4 + 2];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int tk = (K + 63) / 64, tn = (N + 63) / 64;
  for (int tl = blockIdx.y; tl < tk * tn; tl += gridDim.y) {
    const int k0 = (tl / tn) * 64, n0 = (tl % tn) * 64;
    float v[16];
    const int n = n0 + tx, nc = n < N ? n : N - 1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = k0 + ty + 4 * i;
      v[i] = src[off + (size_t)(k < K ? k : K - 1) * N + nc];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[ty + 4 * i][tx] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int nn = n0 + ty + 4 * i, k = k0 + tx;
      if (k < K && nn < N) dst[off + (size_t)nn * K + k] = tile[tx][ty + 4 * i];
    }
  }
}

// column sums of dy (bias gradient): one partial row per workgroup
__global__ __launch_bounds__(256) void colsum_kernel(const float* dy, int lddy, long long M, int C, int c4s, int px,
                                                     int nbx, float* partials) {
  const int b = blockIdx.x;
  const int slab = b / nbx;
  const int bx = b - slab * nbx;
  const int pl = threadIdx.x / c4s;
  const int cl = threadIdx.x - pl * c4s;
  const bool active = pl < px;
  const int cbase4 = slab * c4s;
  const int c = (cbase4 + cl) * 4;
  float4 acc[1] = {zero4()};
  if (active)
    for (long long m = (long long)bx * px + pl; m < M; m += (long long)nbx * px) acc[0] = add4(acc[0], ld4(dy + (size_t)m * lddy + c));
  block_reduce_store<1>(acc, active, pl, cl, c4s, px, cbase4, C, partials + (size_t)bx * C);
}

// the kernel of a dense conv as the operand of its data-gradient GEMM (dl3p_conv2d_gemm_dgrad_weights)
__global__ void conv_dgrad_weights_kernel(const float* w, float* wd, int taps, int Cin, int Cout) {
  const int total = taps * Cin * Cout;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int co = i % Cout, r = i / Cout;
    const int ci = r % Cin, tap = r / Cin;
    wd[((size_t)ci * taps + tap) * Cout + co] = w[i];
  }
}

// ====================================================================================== entry points
struct MatArg { const void* ptr; int ld, cols; };
static int check_mats(const char* fn, std::initializer_list<MatArg> mats) {
  for (const MatArg& m : mats) {
    DL3P_CHECK_ARG(m.ptr != nullptr, "%s: null pointer", fn);
    DL3P_CHECK_ARG(m.cols > 0 && m.cols % 4 == 0, "%s: channel count %d must be a positive multiple of 4", fn, m.cols);
    DL3P_CHECK_ARG(m.ld % 4 == 0 && m.ld >= m.cols && aligned16(m.ptr), "%s: bad layout (ld=%d)", fn, m.ld);
  }
  return DL3P_OK;
}
#define DL3P_CHECK_MATS(fn, ...)                                   \
  do {                                                             \
    const int rc_ = check_mats(fn, {__VA_ARGS__});                 \
    if (rc_) return rc_;                                           \
  } while (0)
static int check_sb(const char* fn, const void* wsp, int pitch, int K) {
  DL3P_CHECK_ARG(wsp && aligned16(wsp) && pitch % 32 == 0 && pitch >= K, "%s: the split kernel must be [3][rows][pitch], pitch a multiple of 32 >= %d (got %d)", fn, K, pitch);
  return DL3P_OK;
}
// the kernels address their operands with 32-bit byte offsets: rows x the widest leading dimension must stay under 4 GiB
static bool fits_4g(unsigned long long rows, std::initializer_list<int> lds) {
  return rows * (unsigned long long)std::max(lds) * 4ull < (1ull << 32);
}

static void fill_fwd(GemmParams* p, const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act, const float* bias,
                     float* y, int ldy, float* stat_partials, int M, int K, int N) {
  p->A = x; p->lda = ldx; p->scale = in_scale; p->shift = in_shift; p->act = in_act;
  p->bias = bias; p->Y = y; p->ldy = ldy; p->partials = stat_partials;
  p->M = M; p->K = K; p->N = N;
}
// data gradient gx[M][K] (+)= dy[M][N] . W[K][N]^T: reduce over N, produce K columns
static void fill_dgrad(GemmParams* p, const float* dy, int lddy, float* gx, int ldgx, int accumulate, int M, int K, int N) {
  p->A = dy; p->lda = lddy; p->act = DL3P_ACT_NONE;
  p->Y = gx; p->ldy = ldgx; p->accumulate = accumulate;
  p->M = M; p->K = N; p->N = K;
}
// the fused BatchNorm-backward sums of the data gradient
static void fill_bb(GemmParams* p, float* partials, const float* z, int ldz, const float* scale, const float* shift, int act,
                    const float* save_mean, const float* save_invstd) {
  p->partials = partials;
  p->bb_z = z; p->bb_ldz = ldz; p->bb_scale = scale; p->bb_shift = shift; p->bb_mean = save_mean; p->bb_invstd = save_invstd;
  p->bb_act = act;
}
// the pre-split kernel planes [3][rows][pitch]
static void fill_bsp(GemmParams* p, const void* wsp, int pitch, int rows) {
  p->Bsp = (const unsigned short*)wsp; p->bsp_pitch = pitch; p->bsp_plane = (long long)rows * pitch;
}
static void fill_wgrad(WgradParams* p, const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act, const float* dy,
                       int lddy, float* slabs, int M, int K, int N, const WgradPlan& pl) {
  p->X = x; p->ldx = ldx; p->scale = in_scale; p->shift = in_shift; p->act = in_act;
  p->DY = dy; p->lddy = lddy; p->slabs = slabs; p->M = M; p->K = K; p->N = N;
  p->ktiles = pl.ktiles; p->ntiles = pl.ntiles; p->mchunk = pl.mchunk;
}

static int pwconv_fwd_impl(const char* fn, const float* x, int ldx, const float* in_scale, const float* in_shift,
                           int in_act, const float* w, bool w_kn, const float* bias, float* y, int ldy,
                           float* stat_partials, int* rows_out, int M, int K, int N, void* stream) {
  DL3P_CHECK_MATS(fn, {x, ldx, K}, {y, ldy, N});
  DL3P_CHECK_ARG(w && aligned16(w) && M > 0, "%s: bad arguments", fn);
  DL3P_CHECK_ARG(fits_4g(M, {ldx, ldy}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  GemmParams p = {};
  fill_fwd(&p, x, ldx, in_scale, in_shift, in_act, bias, y, ldy, stat_partials, M, K, N);
  p.B = w; p.ldb = w_kn ? N : K;
  hipStream_t st = (hipStream_t)stream;
  GemmTraits t;
  t.b_kn = w_kn;
  const GemmPlan pl = plan_gemm(stat_partials ? 1 : 0, M, K, N, t);
  if (rows_out) *rows_out = pl.gx;
  if (pl.form == FORM_TINY) {
    dl3p_pw_tiny_nt(x, ldx, in_scale, in_shift, in_act, w, K, bias, y, ldy, 0, stat_partials, M, K, N, st);
  } else if (pl.form == FORM_STREAMING) {
    p.b_kn = w_kn ? 1 : 0;
    if (stat_partials) launch_pw_small_any<true>(p, pl.small, pl.gx, st);
    else launch_pw_small_any<false>(p, pl.small, pl.gx, st);
  } else {
    p.num_m_tiles = pl.m_tiles;
    const dim3 grid(pl.gx, pl.gy);
    if (w_kn) {
      if (stat_partials) launch_gemm<true, true>(p, pl.nt, pl.mi, grid, st);
      else launch_gemm<true, false>(p, pl.nt, pl.mi, grid, st);
    } else {
      if (stat_partials) launch_gemm<false, true>(p, pl.nt, pl.mi, grid, st);
      else launch_gemm<false, false>(p, pl.nt, pl.mi, grid, st);
    }
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_pwconv_fwd(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                               const float* w, const float* bias, float* y, int ldy, float* stat_partials,
                               int* rows_out, int M, int K, int N, void* stream) {
  return pwconv_fwd_impl("dl3p_pwconv_fwd", x, ldx, in_scale, in_shift, in_act, w, true, bias, y, ldy, stat_partials,
                         rows_out, M, K, N, stream);
}

// the same product with the kernel handed over transposed, wt[N][K]: the B tile then sits in LDS as [n][k] and its
// MFMA fragments are one ds_read_b128 instead of four ds_read_b32 (the layout the data-gradient GEMM gets for free)
extern "C" int dl3p_pwconv_fwd_wt(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                  const float* wt, const float* bias, float* y, int ldy, float* stat_partials,
                                  int* rows_out, int M, int K, int N, void* stream) {
  return pwconv_fwd_impl("dl3p_pwconv_fwd_wt", x, ldx, in_scale, in_shift, in_act, wt, false, bias, y, ldy,
                         stat_partials, rows_out, M, K, N, stream);
}

extern "C" int dl3p_pwconv_fwd_wt_splitk(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                         const float* wt, const float* bias, float* y, int ldy, float* stat_partials,
                                         int* rows_out, void* workspace, size_t workspace_bytes, int M, int K, int N,
                                         void* stream) {
  const char* fn = "dl3p_pwconv_fwd_wt_splitk";
  DL3P_CHECK_MATS(fn, {x, ldx, K}, {y, ldy, N});
  DL3P_CHECK_ARG(wt && aligned16(wt) && M > 0 && workspace && aligned16(workspace), "%s: bad arguments", fn);
  const int S = dl3p_pwconv_fwd_splitk_plan(M, K, N);
  DL3P_CHECK_ARG(S > 1, "%s: M=%d K=%d N=%d is not served (dl3p_pwconv_fwd_splitk_plan; use dl3p_pwconv_fwd_wt)", fn, M, K, N);
  DL3P_CHECK_ARG(workspace_bytes >= sizeof(float) * (size_t)S * M * N, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes,
                 sizeof(float) * (size_t)S * M * N);
  DL3P_CHECK_ARG(fits_4g(M, {ldx, ldy}) && (unsigned long long)S * M * N * 4ull < (1ull << 32), "%s: operands of 4 GiB or more are not supported", fn);
  GemmParams p = {};
  fill_fwd(&p, x, ldx, in_scale, in_shift, in_act, nullptr, (float*)workspace, N, nullptr, M, K, N);
  p.B = wt; p.ldb = K;
  p.ksplit = S; p.kchunk = ceil_div(ceil_div(K, S), 32) * 32;
  static const int nt_env = env_int("DL3P_SPLITK_NT", 8);
  static const int mi_env = env_int("DL3P_SPLITK_MI", 1);
  const int nt = std::min(nt_env, ceil_div(N, 16)), mi = mi_env;
  p.num_m_tiles = ceil_div(M, 64 * mi);
  const int nb = ceil_div(N, 16 * nt);
  hipStream_t st = (hipStream_t)stream;
  launch_gemm<false, false>(p, nt, mi, dim3(p.num_m_tiles, nb * S), st);
  DL3P_CHECK_LAUNCH(fn);
  const int rpp = 256 / (N / 4);
  int rows_per_wg = rpp * 4;
  while (ceil_div(M, rows_per_wg) > DL3P_MAX_STAT_ROWS) rows_per_wg += rpp;
  const int wgs = ceil_div(M, rows_per_wg);
  if (rows_out) *rows_out = wgs;
  hipLaunchKernelGGL(splitk_finish_kernel, dim3(wgs), dim3(256), 0, st, (const float*)workspace, S, bias, y, ldy, stat_partials, M, N,
                     rows_per_wg);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_transpose_batch(const float* src, float* dst, const int* table, int n_matrices, void* stream) {
  DL3P_CHECK_ARG(src && dst && table && n_matrices > 0, "dl3p_transpose_batch: bad arguments");
  hipLaunchKernelGGL(transpose_batch_kernel, dim3(n_matrices, 96), dim3(256), 0, (hipStream_t)stream, src, dst, table);
  DL3P_CHECK_LAUNCH("dl3p_transpose_batch");
  return DL3P_OK;
}

extern "C" int dl3p_pwconv_bwd_data(const float* dy, int lddy, const float* w, float* gx, int ldgx, int accumulate,
                                    int M, int K, int N, void* stream) {
  const char* fn = "dl3p_pwconv_bwd_data";
  DL3P_CHECK_MATS(fn, {dy, lddy, N}, {gx, ldgx, K});
  DL3P_CHECK_ARG(w && aligned16(w) && M > 0, "%s: bad arguments", fn);
  DL3P_CHECK_ARG(fits_4g(M, {lddy, ldgx}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  GemmParams p = {};
  fill_dgrad(&p, dy, lddy, gx, ldgx, accumulate, M, K, N);
  p.B = w; p.ldb = N;           // W[K][N]: output column k, reduction n contiguous
  hipStream_t st = (hipStream_t)stream;
  const GemmPlan pl = plan_gemm(2, M, N, K);
  if (pl.form == FORM_TINY) {
    dl3p_pw_tiny_nt(dy, lddy, nullptr, nullptr, DL3P_ACT_NONE, w, N, nullptr, gx, ldgx, accumulate, nullptr, M, N, K, st);
  } else if (pl.form == FORM_STREAMING) {
    p.b_kn = 0;
    launch_pw_small_any<false>(p, pl.small, pl.gx, st);
  } else {
    p.num_m_tiles = pl.m_tiles;
    launch_gemm<false, false>(p, pl.nt, pl.mi, dim3(pl.gx, pl.gy), st);
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// data gradient of a layer whose input is act(BN(z)): writes gx and, from the finished gradient in the epilogue, the
// BatchNorm-backward partial sums of that BN (the separate dl3p_bn_bwd_reduce pass over gx and z disappears)
extern "C" int dl3p_pwconv_bwd_data_bn(const float* dy, int lddy, const float* w, float* gx, int ldgx, int accumulate,
                                       int M, int K, int N, const float* z, int ldz, const float* scale,
                                       const float* shift, int act, const float* save_mean, const float* save_invstd,
                                       float* partials, int* rows_out, void* stream) {
  const char* fn = "dl3p_pwconv_bwd_data_bn";
  DL3P_CHECK_MATS(fn, {dy, lddy, N}, {gx, ldgx, K}, {z, ldz, K});
  DL3P_CHECK_ARG(w && aligned16(w) && M > 0 && scale && shift && save_mean && save_invstd && partials && rows_out,
                 "%s: bad arguments", fn);
  DL3P_CHECK_ARG(fits_4g(M, {lddy, ldgx, ldz}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  GemmParams p = {};
  fill_dgrad(&p, dy, lddy, gx, ldgx, accumulate, M, K, N);
  p.B = w; p.ldb = N;
  fill_bb(&p, partials, z, ldz, scale, shift, act, save_mean, save_invstd);
  static const int small_bnb = env_int("DL3P_PW_SMALL_BNB", 1);
  GemmTraits t;
  t.tiny_ok = false;                  // (the tiny kernel has no fused sums)
  t.streaming_ok = small_bnb != 0;
  const GemmPlan pl = plan_gemm(3, M, N, K, t);
  *rows_out = pl.gx;
  if (pl.form == FORM_STREAMING) {
    // few channels, many rows: the streaming kernel (the whole kernel matrix in LDS, no workgroup barrier in the row loop)
    p.b_kn = 0;
    launch_pw_small_any<true, true>(p, pl.small, pl.gx, (hipStream_t)stream);
  } else {
    p.num_m_tiles = pl.m_tiles;
    launch_gemm<false, true, true>(p, pl.nt, pl.mi, dim3(pl.gx, pl.gy), (hipStream_t)stream);
  }
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// ------------------------------------------------------------------------------ split-bf16 twins (pw_split.hip)
// The same three products on the bf16 matrix pipe with fp32-accurate results: the conv kernel arrives pre-split into three bf16
// planes [3][rows][pitch] (dl3p_split_bf16x3_batch; rows = the GEMM's OUTPUT columns, reduction index contiguous, pitch a
// multiple of 32 with zero padding), the activations are split while their tile is staged.  Shapes the tiled kernel does not serve
// (few rows, or few-channel layers on the streaming kernels) must go through the fp32 entry points: *_sb_supported says which.
extern "C" int dl3p_pwconv_sb_supported(int role, int M, int K, int N) {
  // role 0 / 1 forward, 2 / 3 data gradient: (M, K, N) as launched (K = reduction length)
  if (M <= 0 || K < 4 || N < 4 || K % 4 || N % 4) return 0;
  SmallShape sh;
  (void)role;
  return gemm_route(M, K, N, GemmTraits(), &sh) == FORM_TILED;
}

extern "C" int dl3p_pwconv_fwd_sb(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                  const void* wsp, int pitch, const float* bias, float* y, int ldy, float* stat_partials,
                                  int* rows_out, int M, int K, int N, void* stream) {
  const char* fn = "dl3p_pwconv_fwd_sb";
  DL3P_CHECK_MATS(fn, {x, ldx, K}, {y, ldy, N});
  int rc = check_sb(fn, wsp, pitch, K);
  if (rc) return rc;
  const int role = stat_partials ? 1 : 0;
  DL3P_CHECK_ARG(M > 0 && dl3p_pwconv_sb_supported(role, M, K, N), "%s: shape M=%d K=%d N=%d is not served by the tiled kernel", fn, M, K, N);
  DL3P_CHECK_ARG(fits_4g(M, {ldx, ldy}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  GemmParams p = {};
  fill_fwd(&p, x, ldx, in_scale, in_shift, in_act, bias, y, ldy, stat_partials, M, K, N);
  fill_bsp(&p, wsp, pitch, N);
  GemmTraits t;
  t.act = in_act; t.has_scale = in_scale != nullptr; t.has_bias = bias != nullptr; t.pitch = pitch; t.ld_max = std::max(ldx, ldy);
  const GemmPlan pl = plan_gemm_sb(role, M, K, N, t);
  p.num_m_tiles = pl.m_tiles;
#ifdef DL3P_SB_ABLATE
  { p.stagger = env_int("DL3P_SB_ABLATE", 0); if (p.stagger == 100 && stat_partials) p.B = stat_partials + (size_t)DL3P_MAX_STAT_ROWS * 2 * N; }      // (ablation build: stamps behind the partial rows)
#endif
  if (rows_out) *rows_out = pl.gx;
  if (pl.form == FORM_PINNED && sb3_debug()) fprintf(stderr, "dl3p_pwconv_fwd_sb: pinned form M=%d K=%d N=%d grid %d\n", M, K, N, pl.gx);
  return launch_plan_sb(fn, p, pl, stat_partials != nullptr, false, (hipStream_t)stream);
}

// gx[M][K] (+)= dy[M][N] . W[K][N]^T with W pre-split as [3][K][pitch >= N]; z != NULL: also the BatchNorm-backward partial sums
// of dl3p_pwconv_bwd_data_bn
extern "C" int dl3p_pwconv_bwd_data_sb(const float* dy, int lddy, const void* wsp, int pitch, float* gx, int ldgx, int accumulate,
                                       int M, int K, int N, const float* z, int ldz, const float* scale, const float* shift,
                                       int act, const float* save_mean, const float* save_invstd, float* partials,
                                       int* rows_out, void* stream) {
  const char* fn = "dl3p_pwconv_bwd_data_sb";
  DL3P_CHECK_MATS(fn, {dy, lddy, N}, {gx, ldgx, K});
  int rc = check_sb(fn, wsp, pitch, N);
  if (rc) return rc;
  const bool bnb = z != nullptr;
  if (bnb) {
    DL3P_CHECK_MATS(fn, {z, ldz, K});
    DL3P_CHECK_ARG(scale && shift && save_mean && save_invstd && partials && rows_out, "%s: bad BatchNorm arguments", fn);
  }
  DL3P_CHECK_ARG(M > 0 && dl3p_pwconv_sb_supported(bnb ? 3 : 2, M, N, K), "%s: shape M=%d K=%d N=%d is not served by the tiled kernel", fn, M, K, N);
  DL3P_CHECK_ARG(fits_4g(M, {lddy, ldgx, ldz}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  GemmParams p = {};
  fill_dgrad(&p, dy, lddy, gx, ldgx, accumulate, M, K, N);
  fill_bsp(&p, wsp, pitch, K);
  if (bnb) fill_bb(&p, partials, z, ldz, scale, shift, act, save_mean, save_invstd);
  const GemmPlan pl = plan_gemm_sb(bnb ? 3 : 2, M, N, K);
  p.num_m_tiles = pl.m_tiles;
  if (rows_out) *rows_out = pl.gx;
  return launch_plan_sb(fn, p, pl, bnb, bnb, (hipStream_t)stream);
}

extern "C" int dl3p_pwconv_bwd_data_sb_apply_supported(int M, int K, int N, int bn_act, int with_sums) {
  // (M, K, N) as dl3p_pwconv_bwd_data_sb: K output columns, N the reduction = channels of the folded BatchNorm.  Two kernels serve
  // it: the pinned-schedule form (256 x 256, no accumulation: the call falls back where the caller accumulates) and the
  // row-stationary one
  if (sb3d_takes(M, K, N, (N + 31) / 32 * 32, bn_act, DL3P_ACT_RELU, with_sums != 0, false, 0) && M >= 131072) return 1;
  if (M < 131072 || !dl3p_sb_rs_fold_supported(M, N, K, bn_act)) return 0;
  return 1;
}

extern "C" int dl3p_pwconv_bwd_data_sb_apply(const float* g, int ldg, const float* z_out, int ldz_out, const float* bn_scale,
                                             const float* bn_shift, int bn_act, const float* bn_mean, const float* bn_invstd,
                                             const float* bn_coef, float* dz, int lddz, const void* wsp, int pitch, float* gx,
                                             int ldgx, int accumulate, int M, int K, int N, const float* z, int ldz,
                                             const float* scale, const float* shift, int act, const float* save_mean,
                                             const float* save_invstd, float* partials, int* rows_out, void* stream) {
  const char* fn = "dl3p_pwconv_bwd_data_sb_apply";
  DL3P_CHECK_MATS(fn, {g, ldg, N}, {z_out, ldz_out, N}, {dz, lddz, N}, {gx, ldgx, K});
  int rc = check_sb(fn, wsp, pitch, N);
  if (rc) return rc;
  DL3P_CHECK_ARG(bn_scale && bn_shift && bn_mean && bn_invstd && bn_coef, "%s: bad BatchNorm-apply arguments", fn);
  const bool bnb = z != nullptr;
  if (bnb) {
    DL3P_CHECK_MATS(fn, {z, ldz, K});
    DL3P_CHECK_ARG(scale && shift && save_mean && save_invstd && partials && rows_out, "%s: bad BatchNorm arguments", fn);
  }
  const int ldm = std::max({ldg, ldgx, ldz, ldz_out, lddz});
  // (the pinned form refuses leading dimensions whose padding rows would wrap; the row-stationary kernel then takes the launch)
  const bool take3 = sb3d_takes(M, K, N, pitch, bn_act, act, bnb, accumulate != 0, ldm);
  DL3P_CHECK_ARG(take3 || (M >= 131072 && dl3p_sb_rs_fold_supported(M, N, K, bn_act)), "%s: shape M=%d K=%d N=%d act %d is not served", fn, M, K, N, bn_act);
  DL3P_CHECK_ARG(fits_4g(M, {ldm}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  GemmParams p = {};
  fill_dgrad(&p, g, ldg, gx, ldgx, accumulate, M, K, N);
  p.f_z = z_out; p.f_ldz = ldz_out; p.f_scale = bn_scale; p.f_shift = bn_shift; p.f_mean = bn_mean; p.f_invstd = bn_invstd;
  p.f_coef = bn_coef; p.f_act = bn_act; p.f_dz = dz; p.f_lddz = lddz;
  fill_bsp(&p, wsp, pitch, K);
  if (bnb) fill_bb(&p, partials, z, ldz, scale, shift, act, save_mean, save_invstd);
  // the pinned-schedule form (pw_split3.hip) where it serves the launch: 256 output columns over a reduction of 256,
  // no accumulation; dl3p_set_option("sb3", 0) / DL3P_SB3_DGRAD=0 keep the row-stationary kernel
  if (take3) {
    const int g3 = dl3p_sb3_grid(M);
    if (rows_out) *rows_out = g3;
    DL3P_CHECK_ARG(dl3p_launch_gemm_sb3d(p, bnb, g3, (hipStream_t)stream), "%s: no pinned-schedule instantiation for activation %d", fn, bn_act);
    DL3P_CHECK_LAUNCH(fn);
    return DL3P_OK;
  }
  p.num_m_tiles = ceil_div(M, 64);
  const int gxn = dl3p_sb_rs_grid(M);
  if (rows_out) *rows_out = gxn;
  DL3P_CHECK_ARG(dl3p_launch_gemm_sbr(p, bnb ? 2 : 0, gxn, (hipStream_t)stream), "dl3p_pwconv_bwd_data_sb_apply: no row-stationary instantiation for K=%d", N);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// ------------------------------------------------------------------------------ weight gradient
extern "C" size_t dl3p_pwconv_bwd_weight_workspace(int M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return 0;
  const size_t a = wgrad_workspace_slabs(M, K, N, false) * K * N;
  const size_t b = (size_t)512 * N;  // bias column-sum partial rows
  return (a > b ? a : b) * sizeof(float);
}

// bias gradient: column sums of dy through the workspace
static int launch_colsum(const char* fn, const float* dy, int lddy, int M, int N, float* gb, float* workspace, hipStream_t st) {
  int c4s, px, nslab;
  pick_lanes(N, &c4s, &px, &nslab);
  const long long need_b = ceil_div_ll(M, px);
  const int nbx = (int)(need_b < 512 ? need_b : 512);
  hipLaunchKernelGGL(colsum_kernel, dim3(nbx * nslab), dim3(256), 0, st, dy, lddy, (long long)M, N, c4s, px, nbx, workspace);
  DL3P_CHECK_LAUNCH(fn);
  return dl3p_reduce_rows_impl(workspace, nbx, (size_t)N, gb, 0, st);
}

// rows_out != NULL: leave the slabs in the workspace for dl3p_reduce_rows_batched (gw / gb unused) and report how many
static int pwconv_bwd_weight_impl(const float* x, int ldx, const float* in_scale, const float* in_shift,
                                  int in_act, const float* dy, int lddy, float* gw, float* gb, float* workspace,
                                  size_t workspace_bytes, int M, int K, int N, int* rows_out, void* stream) {
  const char* fn = "dl3p_pwconv_bwd_weight";
  DL3P_CHECK_MATS(fn, {x, ldx, K}, {dy, lddy, N});
  DL3P_CHECK_ARG((gw || rows_out) && workspace && aligned16(workspace) && M > 0, "dl3p_pwconv_bwd_weight: bad arguments");
  DL3P_CHECK_ARG(!rows_out || (!gb && !dl3p_pw_tiny_applies(M)),
                 "dl3p_pwconv_bwd_weight_slabs: no bias gradient and more than %d rows (use dl3p_pwconv_bwd_weight)", 64);
  const size_t need = dl3p_pwconv_bwd_weight_workspace(M, K, N);
  if (workspace_bytes < need) {
    dl3p_set_error("dl3p_pwconv_bwd_weight: workspace %zu < %zu bytes", workspace_bytes, need);
    return DL3P_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  WgradTraits t;
  t.max_slabs = workspace_bytes / ((size_t)K * N * 4);
  t.streaming_ok = fits_4g(M, {ldx, lddy});
  const WgradPlan pl = plan_wgrad(M, K, N, t);
  if (pl.form == WGRAD_TINY) {
    DL3P_CHECK_ARG(aligned16(gw) && (!gb || aligned16(gb)), "dl3p_pwconv_bwd_weight: gw/gb must be 16-byte aligned");
    dl3p_pw_tiny_wgrad(x, ldx, in_scale, in_shift, in_act, dy, lddy, gw, gb, M, K, N, st);
    DL3P_CHECK_LAUNCH(fn);
    return DL3P_OK;
  }
  WgradParams p = {};
  fill_wgrad(&p, x, ldx, in_scale, in_shift, in_act, dy, lddy, workspace, M, K, N, pl);
  if (pl.form == WGRAD_STREAMING) launch_wgrad_small_any(p, pl.small, pl.slabs, st);
  // fp32-accurate on the bf16 matrix pipe (pw_split.hip, pw_wgrad_sb_kernel): both operands split while they are staged
  else if (pl.form == WGRAD_SPLIT)
    dl3p_launch_wgrad_sb(x, ldx, in_scale, in_shift, in_act, dy, lddy, workspace, M, K, N, pl.kf, pl.sb_nw, pl.sb_ktiles, pl.sb_ntiles, pl.mrows, pl.slabs, st);
  else launch_wgrad_tiled<false>(p, pl, st);
  DL3P_CHECK_LAUNCH(fn);
  if (rows_out) { *rows_out = pl.slabs; return DL3P_OK; }
  int rc = dl3p_reduce_rows_impl(workspace, pl.slabs, (size_t)K * N, gw, 0, st);
  if (rc || !gb) return rc;
  return launch_colsum("dl3p_pwconv_bwd_weight(colsum)", dy, lddy, M, N, gb, workspace, st);
}

extern "C" int dl3p_pwconv_bwd_weight(const float* x, int ldx, const float* in_scale, const float* in_shift,
                                      int in_act, const float* dy, int lddy, float* gw, float* gb, float* workspace,
                                      size_t workspace_bytes, int M, int K, int N, void* stream) {
  return pwconv_bwd_weight_impl(x, ldx, in_scale, in_shift, in_act, dy, lddy, gw, gb, workspace, workspace_bytes, M, K, N,
                                nullptr, stream);
}

extern "C" int dl3p_pwconv_bwd_weight_slabs(const float* x, int ldx, const float* in_scale, const float* in_shift,
                                            int in_act, const float* dy, int lddy, float* workspace, size_t workspace_bytes,
                                            int* rows_out, int M, int K, int N, void* stream) {
  DL3P_CHECK_ARG(rows_out != nullptr, "dl3p_pwconv_bwd_weight_slabs: rows_out is required");
  return pwconv_bwd_weight_impl(x, ldx, in_scale, in_shift, in_act, dy, lddy, nullptr, nullptr, workspace, workspace_bytes, M, K,
                                N, rows_out, stream);
}


// Weight gradient of a conv whose output z goes through BatchNorm (+ activation), with that BatchNorm's backward apply
// folded in: `g` is the gradient of act(BN(z)), `coef` what dl3p_bn_bwd_finalize left.  The kernel forms dz while it stages
// its tiles, multiplies with it, and (dz != nullptr) writes it for the data gradient that follows -- dz must not alias g.
// Served where the kernel reads the gradient operand ONCE: the streaming kernels of the few-channel layers (every wave
// owns the whole K x N gradient) and tiled launches with a single k tile.  With several k tiles every one of them would
// re-form dz from two operands instead of reading one: measured 46 % slower per launch on the 17424 x 64..960 layers
// and a net loss per step (14.64 against 14.32 ms), so those shapes keep dl3p_bn_bwd_apply.
static int wgrad_bn_route(const WgradPlan& pl, int M, int K, int N) {      // 0: not served, 1: streaming kernel, 2: tiled kernel, one k tile
  if (M <= 64 || pl.form == WGRAD_TINY || N % 4 || K % 4) return 0;
  if (pl.form == WGRAD_STREAMING) return (pl.small.kt == 2 && pl.small.ntn == 12) ? 0 : 1;   // (2, 12) + the fold spills
  return (K <= 64 * pl.kw && !(pl.kw == 2 && pl.nw == 8)) ? 2 : 0;      // (the 128 x 128 tile has no registers left for the fold)
}
static WgradPlan plan_wgrad_bn(int M, int K, int N) {      // (the split kernel has no fold)
  WgradTraits t;
  t.split_ok = false;
  return plan_wgrad(M, K, N, t);
}

extern "C" int dl3p_pwconv_bwd_weight_bn_supported(int M, int K, int N) {
  return M > 0 && K > 0 && N > 0 && wgrad_bn_route(plan_wgrad_bn(M, K, N), M, K, N) != 0;
}

extern "C" int dl3p_pwconv_bwd_weight_slabs_bn(const float* x, int ldx, const float* in_scale, const float* in_shift,
                                               int in_act, const float* g, int ldg, const float* z, int ldz,
                                               const float* bn_scale, const float* bn_shift, int bn_act,
                                               const float* save_mean, const float* save_invstd, const float* coef,
                                               float* dz, int lddz, float* workspace, size_t workspace_bytes,
                                               int* rows_out, int M, int K, int N, void* stream) {
  const char* fn = "dl3p_pwconv_bwd_weight_slabs_bn";
  DL3P_CHECK_MATS(fn, {x, ldx, K}, {g, ldg, N}, {z, ldz, N});
  if (dz) DL3P_CHECK_MATS(fn, {dz, lddz, N});
  DL3P_CHECK_ARG(rows_out && workspace && aligned16(workspace) && save_mean && save_invstd && coef && dz != g,
                 "%s: bad arguments", fn);
  const WgradPlan pl = plan_wgrad_bn(M, K, N);
  const int route = wgrad_bn_route(pl, M, K, N);
  DL3P_CHECK_ARG(route != 0, "%s: shape M=%d K=%d N=%d is not served by the tiled kernel", fn, M, K, N);
  DL3P_CHECK_ARG(fits_4g(M, {ldx, ldg, ldz, lddz}), "%s: operands of 4 GiB or more are not supported (M=%d)", fn, M);
  const size_t need = dl3p_pwconv_bwd_weight_workspace(M, K, N);
  if (workspace_bytes < need) {
    dl3p_set_error("%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    return DL3P_EWORKSPACE;
  }
  WgradParams p = {};
  fill_wgrad(&p, x, ldx, in_scale, in_shift, in_act, g, ldg, workspace, M, K, N, pl);
  p.Z = z; p.ldz = ldz; p.b_scale = bn_scale; p.b_shift = bn_shift; p.b_mean = save_mean; p.b_invstd = save_invstd;
  p.b_coef = coef; p.b_act = bn_act; p.DZ = dz; p.lddz = lddz;
  if (route == 1) launch_wgrad_small_any<true>(p, pl.small, pl.small_grid, (hipStream_t)stream);
  else launch_wgrad_tiled<false, true>(p, pl, (hipStream_t)stream);
  DL3P_CHECK_LAUNCH(fn);
  *rows_out = route == 1 ? pl.small_grid : pl.tiled_slabs;
  return DL3P_OK;
}


// ------------------------------------------------------------------------------ dense convolutions as implicit GEMMs
// k x k convolutions with Cin % 4 == 0 (Xception entry_flow_conv1_2 3x3 32->64 and its strided 1x1 shortcuts,
// deeplabv3p_xception.py:119-127,175-183; ResNet50's 3x3 / strided convs) on the tiled GEMM kernels above with the patch
// operand GATHERED while the A tile is staged into LDS (north_star "LDS-staged im2col tiles"): no [M][k*k*Cin] matrix in
// HBM, no im2col / col2im pass.  Four consecutive k are four channels of one tap (Cin % 4 == 0), so the gather keeps the
// 16-byte loads of the pointwise path; taps in the padding are selected to zero after the prologue.
static int conv_gemm_check(const char* fn, int N, int H, int W, int Cin, int Cout, int k, int stride, int rate, int pad_t,
                           int pad_l, int Ho, int Wo) {
  DL3P_CHECK_ARG(dl3p_conv2d_gemm_supported(Cin, Cout, k, stride), "%s: unsupported conv (Cin=%d Cout=%d k=%d stride=%d)", fn,
                 Cin, Cout, k, stride);
  DL3P_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && rate > 0 && pad_t >= 0 && pad_l >= 0, "%s: bad geometry", fn);
  DL3P_CHECK_ARG((long long)N * H * W < (1ll << 24) && (long long)N * Ho * Wo < (1ll << 24) && H < 16384 && W < 16384,
                 "%s: tensor too large", fn);
  DL3P_CHECK_ARG((Ho - 1) * stride - pad_t < H && (Wo - 1) * stride - pad_l < W, "%s: output larger than the strided input", fn);
  return DL3P_OK;
}

extern "C" int dl3p_conv2d_gemm_supported(int Cin, int Cout, int k, int stride) {
  static const int enabled = env_int("DL3P_CONV_GEMM", 1);
  return enabled && Cin > 0 && Cout > 0 && Cin % 4 == 0 && Cout % 4 == 0 && k >= 1 && k <= 7 && (stride == 1 || stride == 2) &&
         (long long)k * k * Cin < 65536;
}

static void conv_gather_fwd(GemmParams* p, int H, int W, int Cin, int k, int stride, int rate, int pad_t, int pad_l, int Ho,
                            int Wo) {
  p->g_RH = Ho; p->g_RW = Wo; p->g_SH = H; p->g_SW = W; p->g_C = Cin; p->g_kw = k;
  p->g_mul = stride; p->g_ay = -pad_t; p->g_ax = -pad_l; p->g_d = rate; p->g_shift = 0;
  p->g_cmagic = (uint32_t)((1ull << 32) / (unsigned)Cin) + 1u;
  p->g_kwmagic = 65536 / k + 1;
}
// data gradient: rows = input pixels; the tap (ky, kx) of input pixel (iy, ix) is output pixel ((iy + pad_t - ky*rate) / stride, ...)
static void conv_gather_dgrad(GemmParams* p, int H, int W, int Cout, int k, int stride, int rate, int pad_t, int pad_l, int Ho,
                              int Wo) {
  p->g_RH = H; p->g_RW = W; p->g_SH = Ho; p->g_SW = Wo; p->g_C = Cout; p->g_kw = k;
  p->g_mul = 1; p->g_ay = pad_t; p->g_ax = pad_l; p->g_d = -rate; p->g_shift = stride == 2 ? 1 : 0;
  p->g_cmagic = (uint32_t)((1ull << 32) / (unsigned)Cout) + 1u;
  p->g_kwmagic = 65536 / k + 1;
}
// the plan of the fp32 implicit GEMMs (forward: N = Cout over output pixels; data gradient: N = Cin over input pixels): the
// heuristics only -- the measured table and the pinned tiles belong to the pointwise launches.  What the launches below and
// dl3p_conv2d_gemm_plan_query both take.
static GemmPlan plan_conv_gemm(int M, int N) {
  GemmPlan pl = {};
  pl.form = FORM_TILED;
  pl.nt = pick_nt(N, M);
  gemm_grid(&pl, M, N);
  return pl;
}
// the gathered operand [N][H][W][ld] and the GEMM-side operand [M][ldm] both stay under 4 GiB
static bool conv_fits_4g(int N, int H, int W, int ld, int M, int ldm) {
  return fits_4g((unsigned long long)N * H * W, {ld}) && fits_4g(M, {ldm});
}

extern "C" int dl3p_conv2d_gemm_fwd(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                    const float* wt, const float* bias, float* y, int ldy, float* stat_partials,
                                    int* rows_out, int N, int H, int W, int Cin, int Cout, int k, int stride, int rate,
                                    int pad_t, int pad_l, int Ho, int Wo, void* stream) {
  const char* fn = "dl3p_conv2d_gemm_fwd";
  int rc = conv_gemm_check(fn, N, H, W, Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  if (rc) return rc;
  DL3P_CHECK_MATS(fn, {x, ldx, Cin}, {y, ldy, Cout});
  DL3P_CHECK_ARG(wt && aligned16(wt), "%s: bad kernel pointer", fn);
  const int M = N * Ho * Wo, K = k * k * Cin;
  DL3P_CHECK_ARG(conv_fits_4g(N, H, W, ldx, M, ldy), "%s: operands of 4 GiB or more are not supported", fn);
  GemmParams p = {};
  fill_fwd(&p, x, ldx, in_scale, in_shift, in_act, bias, y, ldy, stat_partials, M, K, Cout);
  p.B = wt; p.ldb = K;
  conv_gather_fwd(&p, H, W, Cin, k, stride, rate, pad_t, pad_l, Ho, Wo);
  const GemmPlan pl = plan_conv_gemm(M, Cout);
  p.num_m_tiles = pl.m_tiles;
  if (rows_out) *rows_out = pl.gx;
  if (stat_partials) launch_gemm<false, true, false, true>(p, pl.nt, pl.mi, dim3(pl.gx, pl.gy), (hipStream_t)stream);
  else launch_gemm<false, false, false, true>(p, pl.nt, pl.mi, dim3(pl.gx, pl.gy), (hipStream_t)stream);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// wd[ci][tap * Cout + co] = w[(tap * Cin + ci) * Cout + co]: the kernel as the [Nout = Cin][Kred = taps * Cout] operand of
// the data-gradient GEMM (one launch per step and conv; the kernels are a few hundred KB)
extern "C" int dl3p_conv2d_gemm_dgrad_weights(const float* w, float* wd, int k, int Cin, int Cout, void* stream) {
  DL3P_CHECK_ARG(w && wd && k >= 1 && Cin > 0 && Cout > 0, "dl3p_conv2d_gemm_dgrad_weights: bad arguments");
  const int total = k * k * Cin * Cout;
  hipLaunchKernelGGL(conv_dgrad_weights_kernel, dim3(ceil_div(total, 256) < 1024 ? ceil_div(total, 256) : 1024), dim3(256), 0,
                     (hipStream_t)stream, w, wd, k * k, Cin, Cout);
  DL3P_CHECK_LAUNCH("dl3p_conv2d_gemm_dgrad_weights");
  return DL3P_OK;
}

extern "C" int dl3p_conv2d_gemm_bwd_data(const float* dy, int lddy, const float* wd, float* gx, int ldgx, int accumulate,
                                         int N, int H, int W, int Cin, int Cout, int k, int stride, int rate, int pad_t,
                                         int pad_l, int Ho, int Wo, void* stream) {
  const char* fn = "dl3p_conv2d_gemm_bwd_data";
  int rc = conv_gemm_check(fn, N, H, W, Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  if (rc) return rc;
  DL3P_CHECK_MATS(fn, {dy, lddy, Cout}, {gx, ldgx, Cin});
  DL3P_CHECK_ARG(wd && aligned16(wd) && (long long)k * k * Cout < 65536, "%s: bad kernel operand", fn);
  const int M = N * H * W, K = k * k * Cout;
  DL3P_CHECK_ARG(conv_fits_4g(N, Ho, Wo, lddy, M, ldgx), "%s: operands of 4 GiB or more are not supported", fn);
  GemmParams p = {};
  fill_dgrad(&p, dy, lddy, gx, ldgx, accumulate, M, Cin, K);
  p.B = wd; p.ldb = K;
  conv_gather_dgrad(&p, H, W, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  const GemmPlan pl = plan_conv_gemm(M, Cin);
  p.num_m_tiles = pl.m_tiles;
  launch_gemm<false, false, false, true>(p, pl.nt, pl.mi, dim3(pl.gx, pl.gy), (hipStream_t)stream);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

// ---- the same implicit GEMMs on the split-bf16 kernels (pw_split.hip, GA instantiations of pw_gemm_sb_kernel / GX of
// pw_wgrad_sb_kernel): fp32-accurate products on the bf16 matrix pipe, the kernel pre-split by dl3p_split_bf16x3_batch as
// [3][Cout][pitch >= k k Cin] (forward: from the transposed kernel wt) or [3][Cin][pitch >= k k Cout] (data gradient: from
// dl3p_conv2d_gemm_dgrad_weights' wd).  role 0 / 1: forward without / with BatchNorm statistics, 2: data gradient, 4: weight
// gradient; (M, K, N) = the GEMM as launched.
static int conv_sb_mode() { return opt(OPT_CONV_SB); }      // 0 off, 1 the measured rule, 2 wherever supported (tests)

extern "C" int dl3p_conv2d_gemm_sb_supported(int role, int M, int K, int N) {
  if (role < 0 || role > 4 || role == 3 || conv_sb_mode() == 0) return 0;
  if (M < 1024 || K < 32 || N < 16 || K % 4 || N % 4 || K >= 65536) return 0;
  if (role == 4) return opt(OPT_SPLIT_WGRAD) > 0 && N >= 32;
  return 1;
}

// where it pays (scripts/micro/conv_sb.py, profiles/r04_dense_conv_split.txt)
extern "C" int dl3p_conv2d_gemm_sb_pays(int role, int M, int K, int N) {
  if (!dl3p_conv2d_gemm_sb_supported(role, M, K, N)) return 0;
  if (conv_sb_mode() == 2) return 1;
  // measured (same box, fp32-input kernel -> split kernel, us): the WEIGHT gradient wins wherever both of its operands are long
  // enough to fill the tiles -- 125 -> 111 (Xception entry_flow_conv1_2, 264196 x 288 x 64), 124 -> 101 (ResNet50 stage 2), 115 ->
  // 75 / 119 -> 78 (stages 3 / 4), 626 -> 326 (stage 5 at 8712 rows: three slabs instead of one).  The FORWARD and the DATA
  // gradient are bound by the gather of their A operand, not by the matrix pipe: they win with a long reduction (K >= 1024: 141 ->
  // 126, 175 -> 131, 518 -> 460 forward; 132 -> 123, 163 -> 129, 493 -> 443 data gradient); at K = 576 onto 64 columns both lose
  // (142 -> 147, 123 -> 132), as does conv1_2's data gradient onto 32 columns (163 -> 166).  conv1_2's forward would win (150 ->
  // 127 at batch 4, 170 -> 153 at configs[3]) and stays on the fp32-input kernel all the same: its column means come out 3e-8 of
  // a standard deviation off instead of 5e-9 (same rms error per element, 2e-7) -- as the second layer of a 70-layer network on
  // batch statistics that moved every gradient of the 513 x 513 Xception parity test 1.7x further from float64 (0.0048 -> 0.0058
  // worst) for 0.03 ms of a 21.6 ms step
  if (M < 4096) return 0;
  if (role == 4) return M >= 8192 && K >= 128;
  return K >= 1024;
}

extern "C" int dl3p_conv2d_gemm_fwd_sb(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                       const void* wsp, int pitch, const float* bias, float* y, int ldy, float* stat_partials,
                                       int* rows_out, int N, int H, int W, int Cin, int Cout, int k, int stride, int rate,
                                       int pad_t, int pad_l, int Ho, int Wo, void* stream) {
  const char* fn = "dl3p_conv2d_gemm_fwd_sb";
  int rc = conv_gemm_check(fn, N, H, W, Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  if (rc) return rc;
  DL3P_CHECK_MATS(fn, {x, ldx, Cin}, {y, ldy, Cout});
  const int M = N * Ho * Wo, K = k * k * Cin;
  rc = check_sb(fn, wsp, pitch, K);
  if (rc) return rc;
  DL3P_CHECK_ARG(dl3p_conv2d_gemm_sb_supported(stat_partials ? 1 : 0, M, K, Cout), "%s: shape M=%d K=%d N=%d is not served by the split kernel", fn, M, K, Cout);
  DL3P_CHECK_ARG(conv_fits_4g(N, H, W, ldx, M, ldy), "%s: operands of 4 GiB or more are not supported", fn);
  GemmParams p = {};
  fill_fwd(&p, x, ldx, in_scale, in_shift, in_act, bias, y, ldy, stat_partials, M, K, Cout);
  fill_bsp(&p, wsp, pitch, Cout);
  conv_gather_fwd(&p, H, W, Cin, k, stride, rate, pad_t, pad_l, Ho, Wo);
  const GemmPlan pl = plan_gemm_sb_ga(M, Cout);
  p.num_m_tiles = pl.m_tiles;
  if (rows_out) *rows_out = pl.gx;
  dl3p_launch_gemm_sb(p, stat_partials != nullptr, false, true, pl.nt, pl.mi, 1, dim3(pl.gx, pl.gy), (hipStream_t)stream);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

extern "C" int dl3p_conv2d_gemm_bwd_data_sb(const float* dy, int lddy, const void* wdsp, int pitch, float* gx, int ldgx, int accumulate,
                                            int N, int H, int W, int Cin, int Cout, int k, int stride, int rate, int pad_t,
                                            int pad_l, int Ho, int Wo, void* stream) {
  const char* fn = "dl3p_conv2d_gemm_bwd_data_sb";
  int rc = conv_gemm_check(fn, N, H, W, Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  if (rc) return rc;
  DL3P_CHECK_MATS(fn, {dy, lddy, Cout}, {gx, ldgx, Cin});
  const int M = N * H * W, K = k * k * Cout;
  rc = check_sb(fn, wdsp, pitch, K);
  if (rc) return rc;
  DL3P_CHECK_ARG(dl3p_conv2d_gemm_sb_supported(2, M, K, Cin), "%s: shape M=%d K=%d N=%d is not served by the split kernel", fn, M, K, Cin);
  DL3P_CHECK_ARG(conv_fits_4g(N, Ho, Wo, lddy, M, ldgx), "%s: operands of 4 GiB or more are not supported", fn);
  GemmParams p = {};
  fill_dgrad(&p, dy, lddy, gx, ldgx, accumulate, M, Cin, K);
  fill_bsp(&p, wdsp, pitch, Cin);
  conv_gather_dgrad(&p, H, W, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  const GemmPlan pl = plan_gemm_sb_ga(M, Cin);
  p.num_m_tiles = pl.m_tiles;
  dl3p_launch_gemm_sb(p, false, false, true, pl.nt, pl.mi, 1, dim3(pl.gx, pl.gy), (hipStream_t)stream);
  DL3P_CHECK_LAUNCH(fn);
  return DL3P_OK;
}

static size_t conv_wgrad_workspace_bytes(int M, int K, int Cout) {
  const size_t a = wgrad_workspace_slabs(M, K, Cout, true) * K * Cout;
  const size_t b = (size_t)512 * Cout;   // slabs; bias column-sum partial rows
  return (a > b ? a : b) * sizeof(float);
}
extern "C" size_t dl3p_conv2d_gemm_bwd_weight_workspace(int N, int Ho, int Wo, int Cin, int Cout, int k) {
  if (N <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || k <= 0) return 0;
  return conv_wgrad_workspace_bytes(N * Ho * Wo, k * k * Cin, Cout);
}

// the plan of the gathered weight gradient for a workspace of workspace_bytes (launch and dl3p_conv2d_gemm_plan_query)
static WgradPlan plan_conv_wgrad(int M, int K, int Cout, size_t workspace_bytes) {
  WgradTraits t;
  t.max_slabs = workspace_bytes / ((size_t)K * Cout * 4);
  t.gathered = true;
  return plan_wgrad(M, K, Cout, t);
}

static int conv2d_gemm_bwd_weight_impl(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                      const float* dy, int lddy, float* gw, float* gb, float* workspace,
                                      size_t workspace_bytes, int N, int H, int W, int Cin, int Cout, int k, int stride,
                                      int rate, int pad_t, int pad_l, int Ho, int Wo, int* rows_out, void* stream) {
  const char* fn = "dl3p_conv2d_gemm_bwd_weight";
  int rc = conv_gemm_check(fn, N, H, W, Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo);
  if (rc) return rc;
  DL3P_CHECK_MATS(fn, {x, ldx, Cin}, {dy, lddy, Cout});
  DL3P_CHECK_ARG((rows_out || (gw && aligned16(gw))) && workspace && aligned16(workspace) && !(rows_out && gb), "%s: bad arguments", fn);
  const int M = N * Ho * Wo, K = k * k * Cin;
  DL3P_CHECK_ARG(conv_fits_4g(N, H, W, ldx, M, lddy), "%s: operands of 4 GiB or more are not supported", fn);
  const size_t need = dl3p_conv2d_gemm_bwd_weight_workspace(N, Ho, Wo, Cin, Cout, k);
  if (workspace_bytes < need) {
    dl3p_set_error("%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    return DL3P_EWORKSPACE;
  }
  const WgradPlan pl = plan_conv_wgrad(M, K, Cout, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (pl.form == WGRAD_SPLIT) {
    const int geo[10] = {Ho, Wo, H, W, Cin, k, stride, -pad_t, -pad_l, rate};
    dl3p_launch_wgrad_sb_gx(x, ldx, in_scale, in_shift, in_act, dy, lddy, workspace, M, K, Cout, geo, pl.kf, pl.sb_nw, pl.sb_ktiles, pl.sb_ntiles, pl.mrows, pl.slabs, st);
  } else {
    WgradParams p = {};
    fill_wgrad(&p, x, ldx, in_scale, in_shift, in_act, dy, lddy, workspace, M, K, Cout, pl);
    p.g_RH = Ho; p.g_RW = Wo; p.g_SH = H; p.g_SW = W; p.g_C = Cin; p.g_kw = k;
    p.g_mul = stride; p.g_ay = -pad_t; p.g_ax = -pad_l; p.g_d = rate;
    p.g_invRW = 1.f / (float)Wo; p.g_invRH = 1.f / (float)Ho;
    launch_wgrad_tiled<true>(p, pl, st);
  }
  DL3P_CHECK_LAUNCH(fn);
  if (rows_out) { *rows_out = pl.slabs; return DL3P_OK; }
  rc = dl3p_reduce_rows_impl(workspace, pl.slabs, (size_t)K * Cout, gw, 0, st);
  if (rc || !gb) return rc;
  DL3P_CHECK_ARG(aligned16(gb), "%s: gb must be 16-byte aligned", fn);
  return launch_colsum("dl3p_conv2d_gemm_bwd_weight(colsum)", dy, lddy, M, Cout, gb, workspace, st);
}

extern "C" int dl3p_conv2d_gemm_bwd_weight(const float* x, int ldx, const float* in_scale, const float* in_shift, int in_act,
                                           const float* dy, int lddy, float* gw, float* gb, float* workspace,
                                           size_t workspace_bytes, int N, int H, int W, int Cin, int Cout, int k, int stride,
                                           int rate, int pad_t, int pad_l, int Ho, int Wo, void* stream) {
  return conv2d_gemm_bwd_weight_impl(x, ldx, in_scale, in_shift, in_act, dy, lddy, gw, gb, workspace, workspace_bytes, N, H, W,
                                     Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo, nullptr, stream);
}

extern "C" int dl3p_conv2d_gemm_bwd_weight_slabs(const float* x, int ldx, const float* in_scale, const float* in_shift,
                                                 int in_act, const float* dy, int lddy, float* workspace,
                                                 size_t workspace_bytes, int* rows_out, int N, int H, int W, int Cin, int Cout,
                                                 int k, int stride, int rate, int pad_t, int pad_l, int Ho, int Wo,
                                                 void* stream) {
  DL3P_CHECK_ARG(rows_out != nullptr, "dl3p_conv2d_gemm_bwd_weight_slabs: rows_out is required");
  return conv2d_gemm_bwd_weight_impl(x, ldx, in_scale, in_shift, in_act, dy, lddy, nullptr, nullptr, workspace, workspace_bytes,
                                     N, H, W, Cin, Cout, k, stride, rate, pad_t, pad_l, Ho, Wo, rows_out, stream);
}

// the plans of the dense-conv entry points above, reported instead of launched (include/dl3p.h).  (M, K, N) is the GEMM as launched;
// the weight gradient is planned for the workspace dl3p_conv2d_gemm_bwd_weight_workspace asks for
extern "C" int dl3p_conv2d_gemm_plan_query(int role, int M, int K, int N, int* out6) {
  DL3P_CHECK_ARG(out6 && role >= 0 && role <= 7 && role != 3 && M > 0 && K > 0 && N > 0, "dl3p_conv2d_gemm_plan_query: bad arguments");
  for (int i = 0; i < 6; ++i) out6[i] = 0;
  if (role == 4) {
    const WgradPlan pl = plan_conv_wgrad(M, K, N, conv_wgrad_workspace_bytes(M, K, N));
    out6[0] = pl.form;
    if (pl.form == WGRAD_SPLIT) {
      out6[1] = pl.sb_nw == 16 ? 4 : (pl.kf == 2 ? 0 : 1) + (pl.sb_nw == 8 ? 0 : 2);
      out6[2] = pl.sb_ktiles * pl.sb_ntiles; out6[3] = pl.slabs; out6[4] = pl.mrows;
    } else {
      out6[1] = (pl.kw == 2 ? 1 : 0) + (pl.nw == 8 ? 2 : 0);
      out6[2] = pl.ktiles * pl.ntiles; out6[3] = pl.slabs; out6[4] = pl.mchunk;
    }
    return DL3P_OK;
  }
  if (role >= 5 && !dl3p_conv2d_gemm_sb_supported(role - 5, M, K, N)) { out6[0] = -1; return DL3P_OK; }
  const GemmPlan pl = role >= 5 ? plan_gemm_sb_ga(M, N) : plan_conv_gemm(M, N);
  out6[0] = pl.nt; out6[1] = pl.mi; out6[2] = pl.gx; out6[3] = pl.gy; out6[4] = pl.m_tiles;
  return DL3P_OK;
}

// ====================================================================================== plan query (include/dl3p.h)
// the plans the entry points above take, reported instead of launched.  The query knows the shape only: it plans with the
// permissive traits, i.e. it reports the shape-level route (a launch whose activation / bias / leading dimension the
// pinned-schedule form does not serve takes the next form instead)
extern "C" int dl3p_gemm_plan_query(int role, int M, int K, int N, int* out6) {
  DL3P_CHECK_ARG(out6 && role >= 0 && role <= 9 && M > 0 && K > 0 && N > 0, "dl3p_gemm_plan_query: bad arguments");
  for (int i = 0; i < 6; ++i) out6[i] = 0;
  if (role == 4 || role == 9) {
    WgradTraits t;
    t.split_ok = role == 9;
    const WgradPlan pl = plan_wgrad(M, K, N, t);
    if (role == 9) {      // the split-bf16 weight gradient: {4, tile index, 64-row blocks of k per tile, slabs, k tiles x n tiles, from table}; -1: not taken
      if (pl.form != WGRAD_SPLIT) { out6[0] = -1; return DL3P_OK; }
      out6[1] = pl.sb_nw == 16 ? 4 : (pl.kf == 2 ? 0 : 1) + (pl.sb_nw == 8 ? 0 : 2); out6[2] = pl.kf; out6[3] = pl.slabs;
      out6[4] = pl.sb_ktiles * pl.sb_ntiles; out6[5] = gemm_tuned_lookup(9, M, K, N) != nullptr;
    } else if (pl.form == WGRAD_STREAMING) {
      out6[1] = pl.small.kt; out6[2] = pl.small.ntn; out6[4] = pl.slabs;
    } else if (pl.form == WGRAD_TILED) {
      out6[1] = (pl.kw == 2 ? 1 : 0) + (pl.nw == 8 ? 2 : 0); out6[2] = pl.pin_per_cu;
      out6[3] = pl.ktiles * pl.ntiles; out6[4] = pl.slabs; out6[5] = pl.from_table;
    }
    out6[0] = pl.form;
    return DL3P_OK;
  }
  if (role >= 5) {      // the split-bf16 twin of role - 5: {3, nt, mi, form, workgroups, from table}
    if (!dl3p_pwconv_sb_supported(role - 5, M, K, N)) { out6[0] = -1; return DL3P_OK; }
    const GemmPlan pl = plan_gemm_sb(role - 5, M, K, N);
    out6[0] = 3; out6[1] = pl.nt; out6[2] = pl.mi; out6[3] = pl.form; out6[4] = pl.gx * pl.gy; out6[5] = pl.from_table;
    return DL3P_OK;
  }
  const GemmPlan pl = plan_gemm(role, M, K, N);
  if (pl.form == FORM_TINY) out6[0] = 2;
  else if (pl.form == FORM_STREAMING) { out6[0] = 1; out6[1] = pl.small.kt; out6[2] = pl.small.ntn; out6[3] = pl.gx; }
  else { out6[1] = pl.nt; out6[2] = pl.mi; out6[3] = pl.gx; out6[4] = pl.gy; out6[5] = pl.from_table; }
  return DL3P_OK;
}
