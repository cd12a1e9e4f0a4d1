// The library's option table: every knob that dl3p_set_option moves, one row each.
//
//   X(id, what dl3p_get_option reports, option name, environment variable (or nullptr), default, value when not set,
//     normalisation of a set value `v`)
//
// A knob has two sources that the host code reads by enum index, both O(1):
//   opt_set(id)  the value last given to dl3p_set_option, normalised by the row; the row's "not set" value before that, and
//                again after a value that normalises to it
//   opt_env(id)  the environment variable, read ONCE on the knob's first read (never at library load: tests and scripts set
//                os.environ after import); the row's default when the variable is absent
//   opt(id)      the usual precedence: the option where it is set, else the environment, else the default
// Precedence is per knob and stays as it always was; rows whose precedence is not opt() say so, and the code that reads
// them names the source it wants.  Integer environment variables without an option go through env_int (common.h).
#pragma once
#include "common.h"

// what dl3p_get_option reports for a knob (the executor records these values and pins them again, so each keeps the exact
// form it always had): nothing (INT_MIN); the option as set; the option, else the environment once a route has read it
// (GE0: only a non-negative one); the resolved value opt(id)
enum OptGet { GET_NONE, GET_SET, GET_LATCHED, GET_LATCHED_GE0, GET_RESOLVED };

#define DL3P_OPTION_TABLE(X)                                                                                                  \
  /* rows from which the streaming small-K.N kernels take over from the tiled kernel; v < 0 restores the production           \
     threshold (the literal default, not the environment) */                                                                  \
  X(PW_SMALL_MIN_ROWS, GET_NONE, "pw_small_min_rows", "DL3P_PW_SMALL_MIN_ROWS", 1 << 17, -1, v < 0 ? (1 << 17) : v)           \
  /* pin the tile of the fp32 / split GEMMs (0: automatic).  option > tuned table > heuristic */                              \
  X(GEMM_NT, GET_NONE, "gemm_nt", nullptr, 0, 0, (v >= 1 && v <= 8) ? v : 0)                                                  \
  /* SURPRISING: the environment beats the option here (gemm_grid applies DL3P_GEMM_MI / DL3P_GEMM_PER_CU last, after         \
     option > tuned table > heuristic); only the option counts as "another form is pinned" for the split routes */            \
  X(GEMM_MI, GET_NONE, "gemm_mi", "DL3P_GEMM_MI", 0, 0, (v == 1 || v == 2) ? v : 0)                                           \
  X(GEMM_PER_CU, GET_NONE, "gemm_per_cu", "DL3P_GEMM_PER_CU", 0, 0, v > 0 ? v : 0)                                            \
  /* 0 ignores gemm_tuned.h / sb_tuned.h (tiles and verdicts) */                                                              \
  X(GEMM_TUNED, GET_NONE, "gemm_tuned", "DL3P_GEMM_TUNED", 1, -1, v ? 1 : 0)                                                  \
  /* the producer / consumer form of the split kernel (opt-in); dl3p_get_option reports the resolved value */                 \
  X(SB_PIPE, GET_RESOLVED, "sb_pipe", "DL3P_SB_PIPE", 0, -1, v ? 1 : 0)                                                       \
  /* weight gradients on the split-bf16 kernel.  option > DL3P_SPLIT_WGRAD > DL3P_SPLIT_GEMM > 1; dl3p_get_option             \
     reports -1 until the first weight-gradient route has resolved it */                                                      \
  X(SPLIT_WGRAD, GET_LATCHED, "split_wgrad", "DL3P_SPLIT_WGRAD", env_int("DL3P_SPLIT_GEMM", 1), -1, v ? 1 : 0)                \
  /* pin the split weight gradient's plan (and bypass the verdicts): tile 0..4, -1 none; workgroups per CU, 0 none */         \
  X(SPLIT_WGRAD_TILE, GET_NONE, "split_wgrad_tile", nullptr, -1, -1, (v >= 0 && v <= 4) ? v : -1)                             \
  X(SPLIT_WGRAD_PER_CU, GET_NONE, "split_wgrad_per_cu", nullptr, 0, 0, v > 0 ? v : 0)                                         \
  /* split-K forward: -1 (any negative) the rule, 0 never, S > 0 that many slices where the shape is served.  The             \
     environment (0 = never) counts only while the option is negative */                                                      \
  X(SPLITK, GET_SET, "splitk", "DL3P_SPLITK", -1, -1, v)                                                                      \
  /* pin the split kernel's wide-tile family: sb_wm 1 | 2, -1 never wide, 0 automatic; sb_nt 8 | 12 | 16 */                   \
  X(SB_WM, GET_NONE, "sb_wm", nullptr, 0, 0, (v >= -1 && v <= 2) ? v : 0)                                                     \
  X(SB_NT, GET_NONE, "sb_nt", nullptr, 0, 0, (v == 8 || v == 12 || v == 16) ? v : 0)                                          \
  /* the row-stationary split kernel: 0 never, 1 wherever it serves the shape, -1 by rule.  option > environment (>= 0)       \
     > tuned table > rule; the pinned-schedule route yields to the OPTION being 1 only */                                     \
  X(SB_RS, GET_SET, "sb_rs", "DL3P_SB_RS", -1, -1, v < 0 ? -1 : (v ? 1 : 0))                                                  \
  /* the pinned-schedule split forward / data gradient: 0 never, 1 wherever supported, -1 by rule.  option > environment      \
     (>= 0); dl3p_get_option reports the environment's value once a route has read it */                                      \
  X(SB3, GET_LATCHED_GE0, "sb3", "DL3P_SB3", -1, -1, v < 0 ? -1 : (v ? 1 : 0))                                                \
  /* K groups of the bf16 GEMM: 0 the rule, 1 never, 2 / 4 wherever possible, -1 not set */                                   \
  X(BF16_KG, GET_NONE, "bf16_kg", "DL3P_BF16_KG", 0, -1, (v == 0 || v == 1 || v == 2 || v == 4) ? v : -1)                     \
  /* dense convs on the split kernels: 0 never, 1 the measured rule, 2 wherever supported, -1 not set */                      \
  X(CONV_SB, GET_SET, "conv_sb", "DL3P_CONV_SB", 1, -1, (v >= 0 && v <= 2) ? v : -1)                                          \
  /* depthwise plan pins (0: automatic).  option > dw_tuned.h > environment / heuristic */                                    \
  X(DW_PER_CU, GET_NONE, "dw_per_cu", nullptr, 0, 0, v > 0 ? v : 0)                                                           \
  X(DW_WANT, GET_NONE, "dw_want", "DL3P_DW_WANT", DL3P_NUM_CUS * 3 / 2, 0, v > 0 ? v : 0)                                     \
  X(DW_MAXTH, GET_NONE, "dw_maxth", "DL3P_DW_MAXTH", 16, 0, v > 0 ? v : 0)                                                    \
  X(DW_TW, GET_NONE, "dw_tw", nullptr, 0, 0, (v == 2 || v == 4) ? v : 0)                                                      \
  X(DW_TUNED, GET_NONE, "dw_tuned", "DL3P_DW_TUNED", 1, -1, v ? 1 : 0)                                                        \
  /* fp32 weight gradient: tile 0..3 (-1 none) and workgroups per CU (0 none).  option > tuned table > environment >          \
     heuristic */                                                                                                             \
  X(WGRAD_TILE, GET_NONE, "wgrad_tile", "DL3P_WGRAD_TILE", -1, -1, (v >= 0 && v <= 3) ? v : -1)                               \
  X(WGRAD_PER_CU, GET_NONE, "wgrad_per_cu", "DL3P_WGRAD_PER_CU", 4, 0, v > 0 ? v : 0)

enum Opt {
#define X(id, get, name, env, def, unset, norm) OPT_##id,
  DL3P_OPTION_TABLE(X)
#undef X
  OPT_COUNT
};

struct OptState { int set, env; bool env_read; };
extern OptState g_opt[OPT_COUNT];
int opt_env_read(Opt id);      // options.hip: the one getenv of this knob

static constexpr int k_opt_unset[OPT_COUNT] = {
#define X(id, get, name, env, def, unset, norm) unset,
  DL3P_OPTION_TABLE(X)
#undef X
};

static inline int opt_set(Opt id) { return g_opt[id].set; }
static inline int opt_env(Opt id) { return g_opt[id].env_read ? g_opt[id].env : opt_env_read(id); }
static inline int opt(Opt id) { return g_opt[id].set != k_opt_unset[id] ? g_opt[id].set : opt_env(id); }
