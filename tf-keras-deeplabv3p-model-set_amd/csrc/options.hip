// dl3p_set_option / dl3p_get_option and the state behind options.h: the only definition of the option table.
#include "options.h"
#include <limits.h>
#include <string.h>

struct OptRow { const char* name; const char* env; int (*def)(); int (*norm)(int); OptGet get; };

#define X(id, get, name, env, def, unset, norm) \
  static int opt_def_##id() { return def; }     \
  static int opt_norm_##id(int v) { return norm; }
DL3P_OPTION_TABLE(X)
#undef X

static const OptRow g_opt_rows[OPT_COUNT] = {
#define X(id, get, name, env, def, unset, norm) {name, env, opt_def_##id, opt_norm_##id, get},
  DL3P_OPTION_TABLE(X)
#undef X
};

OptState g_opt[OPT_COUNT] = {
#define X(id, get, name, env, def, unset, norm) {unset, 0, false},
  DL3P_OPTION_TABLE(X)
#undef X
};

int opt_env_read(Opt id) {
  const OptRow& r = g_opt_rows[id];
  const char* e = r.env ? getenv(r.env) : nullptr;
  g_opt[id].env = e ? atoi(e) : r.def();
  g_opt[id].env_read = true;
  return g_opt[id].env;
}

static int opt_find(const char* name) {
  for (int i = 0; i < OPT_COUNT; ++i)
    if (!strcmp(name, g_opt_rows[i].name)) return i;
  return -1;
}

extern "C" int dl3p_set_option(const char* name, int value) {
  DL3P_CHECK_ARG(name != nullptr, "dl3p_set_option: null name");
  const int i = opt_find(name);
  if (i < 0) {
    dl3p_set_error("dl3p_set_option: unknown option '%s'", name);
    return DL3P_EINVAL;
  }
  g_opt[i].set = g_opt_rows[i].norm(value);
  return DL3P_OK;
}

// the current value of the knobs that decide how many slabs / partial rows a traced launch writes: an executor records them
// when it traces its plans and pins them again before an eager replay; INT_MIN for an unknown name
extern "C" int dl3p_get_option(const char* name) {
  const int i = name ? opt_find(name) : -1;
  if (i < 0) return INT_MIN;
  const OptState& s = g_opt[i];
  const bool is_set = s.set != k_opt_unset[i];
  switch (g_opt_rows[i].get) {
    case GET_SET: return s.set;
    case GET_LATCHED: return (is_set || !s.env_read) ? s.set : s.env;
    case GET_LATCHED_GE0: return (is_set || !s.env_read || s.env < 0) ? s.set : s.env;
    case GET_RESOLVED: return opt((Opt)i);
    default: return INT_MIN;
  }
}
