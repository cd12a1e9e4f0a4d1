#!/usr/bin/env python3
"""Census of the host-side answers of libdl3p: which kernel, tile, grid and workspace every plan query reports, over a fixed
list of shapes and a fixed list of option / environment states.  CPU only, no launch.

  python3 scripts/plan_census.py OUT.txt [--lib PATH/libdl3p.so] [--quick]

Two trees whose host code takes the same decisions write the same file: the check of a change to the planners, the option
store or the dispatch heuristics that must not change a decision (build both trees, run this script from one of them against
each library with --lib, compare the files).  It uses the C ABI of include/dl3p.h only.

A knob's environment variable is read once per process, so every environment state runs in a fresh child process
(--child); the child's environment holds no DL3P_* variable but the ones its state names -- DL3P_PW_SMALL_MIN_ROWS is
always set explicitly.  The default state is written in full, one line per shape; every other state lists the lines that
differ from its base.  --quick: a thinned shape and state list (tests/test_plan_census_cpu.py).
"""
import ast
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, 'tf-keras-deeplabv3p-model-set_amd')
CSRC = os.path.join(PKGDIR, 'csrc')

GET_NAMES = ('split_wgrad', 'conv_sb', 'sb_rs', 'sb3', 'sb_pipe', 'splitk')
# option -> (values the tests and scripts move it through, the value that restores it)
OPTIONS = {
    'pw_small_min_rows': ((64, 0, 1 << 30), -1), 'gemm_nt': (tuple(range(1, 9)), 0), 'gemm_mi': ((1, 2), 0),
    'gemm_per_cu': ((1, 2, 3, 4, 6), 0), 'gemm_tuned': ((0,), 1), 'sb_pipe': ((1,), 0), 'split_wgrad': ((0,), 1),
    'split_wgrad_tile': ((0, 1, 2, 3, 4), -1), 'split_wgrad_per_cu': ((1, 2, 3, 4), 0), 'splitk': ((0, 2, 4, 5, 8), -1),
    'sb_wm': ((-1, 1, 2), 0), 'sb_nt': ((8, 12, 16), 0), 'sb_rs': ((0, 1), -1), 'sb3': ((0, 1), -1),
    'bf16_kg': ((0, 1, 2, 4), -1), 'conv_sb': ((0, 1, 2), -1), 'dw_per_cu': ((2, 4, 8), 0), 'dw_want': ((256, 384, 512), 0),
    'dw_maxth': ((8, 16), 0), 'dw_tw': ((2, 4), 0), 'dw_tuned': ((0,), 1), 'wgrad_tile': ((0, 1, 2, 3), -1),
    'wgrad_per_cu': ((2, 4, 8), 0),
}
# every integer environment variable the GEMM and depthwise hosts read (pwconv / pw_split* / pw_bf16 / pw_tiny / dwconv), at one
# non-default value
ENVS = {
    'DL3P_PW_SMALL': 0, 'DL3P_PW_SMALL_PER_CU': 3, 'DL3P_PW_SMALL_MIN_ROWS': 4096, 'DL3P_PW_SMALL_BNB': 0, 'DL3P_GEMM_NT_MAX': 4,
    'DL3P_GEMM_QUANT': 0, 'DL3P_GEMM_LONG_ROWS': 30000, 'DL3P_GEMM_LONG_NT': 4, 'DL3P_GEMM_MI': 1, 'DL3P_GEMM_PER_CU': 4,
    'DL3P_GEMM_TUNED': 0, 'DL3P_SB_PIPE': 1, 'DL3P_SPLIT_WGRAD': 0, 'DL3P_SPLIT_GEMM': 0, 'DL3P_SB_RS': 0, 'DL3P_SB_RS_FWD': 1,
    'DL3P_SB3': 1, 'DL3P_SB3_DGRAD': 1, 'DL3P_SPLITK': 0, 'DL3P_SPLITK_NT': 4, 'DL3P_SPLITK_MI': 2, 'DL3P_WGRAD_SMALL': 0,
    'DL3P_WGRAD_SMALL_PER_CU': 4, 'DL3P_WGRAD_TILE': 2, 'DL3P_WGRAD_PER_CU': 2, 'DL3P_CONV_GEMM': 0, 'DL3P_CONV_SB': 2,
    'DL3P_WGRAD_SB_MIXED': 1, 'DL3P_SB_RS_CPS': 2, 'DL3P_SB_RS_CG16': 1, 'DL3P_PW_TINY_ROWS': 16, 'DL3P_BF16_DBG': 1,
    'DL3P_BF16_NOSTREAM': 1, 'DL3P_BF16_MI': 1, 'DL3P_BF16_KG': 2, 'DL3P_BF16_KG_NT': 4, 'DL3P_DW_WANT': 256, 'DL3P_DW_BAND': 8,
    'DL3P_DW5_ROWS': 2, 'DL3P_DW_TUNED': 0, 'DL3P_DW_LAT3': 0, 'DL3P_DW_BALANCE': 1, 'DL3P_DW_MAXTH': 8, 'DL3P_LAT2_PER_CU': 4,
    'DL3P_LAT3_PER_CU': 4, 'DL3P_DWF_PER_CU': 4, 'DL3P_DW_NT': 0, 'DL3P_DW_FAST_ROWS': 0, 'DL3P_DWW_PER_CU': 4, 'DL3P_DW5_WROWS': 1,
    'DL3P_BF16_DW_WINDOW': 0,
}
# knobs with an option AND a variable: (variable, value, option, values set while the variable is set)
COMBOS = (
    ('DL3P_PW_SMALL_MIN_ROWS', 4096, 'pw_small_min_rows', (64, -1)), ('DL3P_GEMM_MI', 1, 'gemm_mi', (2,)),
    ('DL3P_GEMM_PER_CU', 4, 'gemm_per_cu', (2,)), ('DL3P_GEMM_TUNED', 0, 'gemm_tuned', (1, 0)),
    ('DL3P_SB_PIPE', 1, 'sb_pipe', (0, 1)), ('DL3P_SPLIT_WGRAD', 0, 'split_wgrad', (1, 0)), ('DL3P_SPLITK', 0, 'splitk', (4, -1)),
    ('DL3P_SB_RS', 0, 'sb_rs', (1, -1)), ('DL3P_SB_RS', 1, 'sb_rs', (0, -1)), ('DL3P_SB3', 1, 'sb3', (0, -1)),
    ('DL3P_SB3', 0, 'sb3', (1, -1)), ('DL3P_BF16_KG', 2, 'bf16_kg', (1, -1)), ('DL3P_CONV_SB', 2, 'conv_sb', (1, -1)),
    ('DL3P_CONV_SB', 0, 'conv_sb', (2, -1)), ('DL3P_DW_WANT', 256, 'dw_want', (512, 0)), ('DL3P_DW_MAXTH', 8, 'dw_maxth', (16, 0)),
    ('DL3P_DW_TUNED', 0, 'dw_tuned', (1, 0)), ('DL3P_WGRAD_TILE', 2, 'wgrad_tile', (1, -1)),
    ('DL3P_WGRAD_PER_CU', 2, 'wgrad_per_cu', (8, 0)),
)
ROWS = (1, 15, 16, 63, 64, 65, 255, 256, 257, 4095, 4096, 16383, 16384, 65535, 65536, 131071, 131072, 266256)
PAIRS = ((8, 8), (24, 144), (144, 24), (256, 256), (304, 256), (256, 304), (288, 256), (728, 728), (1280, 256), (2048, 1536))


def table_rows(name, n):
    pat = re.compile(r'^\s*\{' + ', '.join([r'(-?\d+)'] * n) + r'\}')
    rows = [tuple(int(v) for v in m.groups()) for m in (pat.match(line) for line in open(os.path.join(CSRC, name))) if m]
    return [r for r in rows if r[0] >= 0]


def shapes(quick):
    keys = {r[1:4] for r in table_rows('gemm_tuned.h', 7)} | {r[1:4] for r in table_rows('sb_tuned.h', 7)}
    keys |= {r[1:4] for r in table_rows('sb_tuned.h', 5)}
    keys = sorted(keys)
    if quick:
        keys = keys[::16]
    out = set()
    for M, K, N in keys:
        out.update(((M, K, N), (M - 1, K, N), (M + 1, K, N), (M, K + 4, N), (M, K, N + 4)))
    rows, pairs = (ROWS[3::4], PAIRS[1::3]) if quick else (ROWS, PAIRS)
    out.update((M, K, N) for M in rows for K, N in pairs)
    return sorted(s for s in out if s[0] > 0)


def edge_cases():
    """the geometries of the depthwise edge suite (CASES of tests/test_dw_edges_gpu.py, read from its source): gather, residue-class,
    5x5 and narrow-map plans next to the tuned production shapes.  -> (N, H, W, C, k, stride, rate, pad); pad: None = TF SAME"""
    tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_dw_edges_gpu.py')).read())
    table = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', '') == 'CASES')
    out = []
    for call in table.elts:
        kw = {k.arg: ast.literal_eval(k.value) for k in call.keywords}
        pad = kw.get('pad', 'same')
        out.append(tuple(ast.literal_eval(a) for a in call.args[1:5]) + (kw.get('k', 3), kw.get('s', 1), kw.get('r', 1),
                                                                         None if pad == 'same' else tuple(pad)))
    return out


def dw_keys(quick):
    keys = sorted({r[1:8] + (None,) for r in table_rows('dw_tuned.h', 12)})
    edges = [c for c in dict.fromkeys(edge_cases()) if c not in keys]
    return (keys[::5] if quick else keys) + edges          # (the edge geometries are few and each is there for a reason: never thinned)


def load(path):
    L = ctypes.CDLL(path)
    i, p6 = ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    for name, res, args in (('dl3p_set_option', i, [ctypes.c_char_p, i]), ('dl3p_get_option', i, [ctypes.c_char_p]),
                            ('dl3p_gemm_plan_query', i, [i] * 4 + [p6]), ('dl3p_dw_plan_query', i, [i] * 12 + [p6]),
                            ('dl3p_pwconv_sb_supported', i, [i] * 4), ('dl3p_pwconv_sb_pays', i, [i] * 4),
                            ('dl3p_conv2d_gemm_sb_supported', i, [i] * 4), ('dl3p_conv2d_gemm_sb_pays', i, [i] * 4),
                            ('dl3p_pwconv_bwd_weight_workspace', ctypes.c_size_t, [i] * 3),
                            ('dl3p_conv2d_gemm_bwd_weight_workspace', ctypes.c_size_t, [i] * 6),
                            ('dl3p_pwconv_fwd_splitk_plan', i, [i] * 3), ('dl3p_pwconv_fwd_splitk_workspace', ctypes.c_size_t, [i] * 3),
                            ('dl3p_pwconv_bwd_data_sb_apply_supported', i, [i] * 5), ('dl3p_pwconv_bwd_weight_bn_supported', i, [i] * 3),
                            ('dl3p_dwconv2d_bwd_weight_bn_supported', i, [i] * 11), ('dl3p_dw_upsampled_input_supported', i, [i] * 13),
                            ('dl3p_dwconv2d_bwd_weight_workspace', ctypes.c_size_t, [i] * 5)):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def geometry(H, W, k, stride, rate, pad):
    """Ho, Wo, pad_t, pad_l; pad: None = TF SAME, or (top, bottom, left, right)"""
    keff = k + (k - 1) * (rate - 1)
    if pad:
        return (H + pad[0] + pad[1] - keff) // stride + 1, (W + pad[2] + pad[3] - keff) // stride + 1, pad[0], pad[2]
    Ho, Wo = -(-H // stride), -(-W // stride)
    return Ho, Wo, max((Ho - 1) * stride + keff - H, 0) // 2, max((Wo - 1) * stride + keff - W, 0) // 2


def census(L, shape_list, dw_list):
    """-> the lines of one state: one per GEMM shape, one per depthwise key, one of dl3p_get_option"""
    out6 = (ctypes.c_int * 6)()
    lines = []
    for M, K, N in shape_list:
        f = ['%d %d %d' % (M, K, N)]
        for role in range(10):
            rc = L.dl3p_gemm_plan_query(role, M, K, N, out6)
            f.append('q%d=%s' % (role, ','.join(str(v) for v in out6) if rc == 0 else 'rc%d' % rc))
        f.append('sb=' + ''.join('%d' % L.dl3p_pwconv_sb_supported(r, M, K, N) for r in range(4)))
        f.append('pays=' + ','.join('%d' % L.dl3p_pwconv_sb_pays(r, M, K, N) for r in range(5)))
        f.append('csb=' + ''.join('%d%d' % (L.dl3p_conv2d_gemm_sb_supported(r, M, K, N), L.dl3p_conv2d_gemm_sb_pays(r, M, K, N))
                                  for r in (0, 1, 2, 4)))
        f.append('ws=%d' % L.dl3p_pwconv_bwd_weight_workspace(M, K, N))
        f.append('cws=%d,%d' % (L.dl3p_conv2d_gemm_bwd_weight_workspace(1, 1, M, K, N, 1),
                                L.dl3p_conv2d_gemm_bwd_weight_workspace(1, 1, M, K, N, 3) if 9 * K < 65536 else -1))
        f.append('sk=%d,%d' % (L.dl3p_pwconv_fwd_splitk_plan(M, K, N), L.dl3p_pwconv_fwd_splitk_workspace(M, K, N)))
        f.append('apply=' + ''.join('%d' % L.dl3p_pwconv_bwd_data_sb_apply_supported(M, K, N, act, s) for act in range(4) for s in (0, 1)))
        f.append('wbn=%d' % L.dl3p_pwconv_bwd_weight_bn_supported(M, K, N))
        lines.append(' '.join(f))
    for N, H, W, C, k, stride, rate, pad in dw_list:
        Ho, Wo, pt, pl = geometry(H, W, k, stride, rate, pad)
        f = ['dw %d %d %d %d %d %d %d%s' % (N, H, W, C, k, stride, rate, ' pad=%d,%d,%d,%d' % pad if pad else '')]
        for role in range(4):
            rc = L.dl3p_dw_plan_query(role, N, H, W, C, k, stride, rate, pt, pl, Ho, Wo, out6)
            f.append('q%d=%s' % (role, ','.join(str(v) for v in out6) if rc == 0 else 'rc%d' % rc))
        f.append('wbn=%d' % L.dl3p_dwconv2d_bwd_weight_bn_supported(N, H, W, C, k, stride, rate, pt, pl, Ho, Wo))
        f.append('up=' + ''.join('%d' % L.dl3p_dw_upsampled_input_supported(r, N, H, W, C, 4, k, stride, rate, pt, pl, Ho, Wo)
                                 for r in (0, 1)))
        f.append('ws=%d' % L.dl3p_dwconv2d_bwd_weight_workspace(N, Ho, Wo, C, k))
        lines.append(' '.join(f))
    lines.append('get_option ' + ' '.join('%s=%d' % (n, L.dl3p_get_option(n.encode())) for n in GET_NAMES + ('no_such_knob',)))
    return lines


def child(spec):
    """one process = one environment state: its base census, then every option step of `spec`, each followed by its restore"""
    L = load(spec['lib'])
    shape_list, dw_list = shapes(spec['quick']), dw_keys(spec['quick'])
    result = {'base': census(L, shape_list, dw_list), 'steps': []}
    base = result['base']

    def diff(lines):
        return [l for l, b in zip(lines, base) if l != b]
    for name, values, restore in spec['steps']:
        for v in list(values) + [restore]:
            rc = L.dl3p_set_option(name.encode(), v)
            label = '%s=%d%s rc%d' % (name, v, ' (restore)' if v == restore else '', rc)
            result['steps'].append((label, diff(census(L, shape_list, dw_list))))
    rc = L.dl3p_set_option(b'no_such_knob', 1)
    result['steps'].append(('no_such_knob=1 rc%d' % rc, diff(census(L, shape_list, dw_list))))
    json.dump(result, sys.stdout)


def run_child(lib, quick, env_state, steps):
    env = {k: v for k, v in os.environ.items() if not k.startswith('DL3P_')}
    env['DL3P_PW_SMALL_MIN_ROWS'] = str(1 << 17)
    env.update({k: str(v) for k, v in env_state.items()})
    spec = json.dumps({'lib': lib, 'quick': quick, 'steps': steps})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', spec], env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('census child failed (%s):\n%s' % (env_state, r.stderr))
    return json.loads(r.stdout)


def main(argv):
    if argv[:1] == ['--child']:
        return child(json.loads(argv[1]))
    quick = '--quick' in argv
    lib = os.path.join(PKGDIR, 'libdl3p.so')
    if '--lib' in argv:
        lib = os.path.abspath(argv[argv.index('--lib') + 1])
    out_path = argv[0]
    options = {k: OPTIONS[k] for k in sorted(OPTIONS)}
    envs, combos = sorted(ENVS.items()), COMBOS
    if quick:
        options = {k: (v[0][:1], v[1]) for k, v in options.items()}
        envs, combos = envs[::8], combos[::6]
    with open(out_path, 'w') as f:
        def write_steps(res):
            for label, lines in res['steps']:
                f.write('-- option %s: %d lines differ\n' % (label, len(lines)))
                f.writelines(l + '\n' for l in lines)
        d = run_child(lib, quick, {}, [(k, v[0], v[1]) for k, v in options.items()])
        f.write('== defaults\n')
        f.writelines(l + '\n' for l in d['base'])
        write_steps(d)
        for states in [({k: v}, []) for k, v in envs] + [({e: ev}, [(o, ov[:-1], ov[-1])]) for e, ev, o, ov in combos]:
            r = run_child(lib, quick, states[0], states[1])
            lines = [l for l, b in zip(r['base'], d['base']) if l != b]
            f.write('== %s: %d lines differ from the defaults\n' % (' '.join('%s=%s' % kv for kv in states[0].items()), len(lines)))
            f.writelines(l + '\n' for l in lines)
            write_steps(r)
    return 0


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1:]))
