"""The executor's switch table (exec_options.py): defaults, every spelling whose meaning differs, immutability, and that executor.py
reads the environment nowhere else.  Everything runs against a dict handed to ExecOptions.from_env, never the process environment.
The expected values are the literals executor.py had at its read sites before the table existed, written out here."""
import ast
import importlib.util
import os
import re

import pytest

from conftest import PKG_NAME, ROOT

PKG_DIR = os.path.join(ROOT, PKG_NAME)


def _load():
    """by file: the module needs neither torch nor the library"""
    spec = importlib.util.spec_from_file_location('_exec_options_under_test', os.path.join(PKG_DIR, 'exec_options.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


eo = _load()
opts = lambda **env: eo.ExecOptions.from_env({'DL3P_' + k: v for k, v in env.items()})

# every DL3P_* name executor.py handed to os.environ before the table
NAMES = (
    'DL3P_SPLIT_GEMM', 'DL3P_SPLIT_WGRAD', 'DL3P_FORCE_DIST', 'DL3P_FUSED_HEAD', 'DL3P_IRB', 'DL3P_IRB_DEBUG_Z', 'DL3P_IRB_MIN_ROWS',
    'DL3P_IRB_S1_MIN_ROWS', 'DL3P_BATCHED_WGRAD', 'DL3P_GHOST', 'DL3P_GHOST_MIN_ROWS', 'DL3P_FOLD_RESIZE', 'DL3P_STEM_DIRECT',
    'DL3P_NARROW_CONV', 'DL3P_BF16_FUSE_BN_BWD', 'DL3P_GRAD_ALIAS', 'DL3P_SPLIT_MIN_K', 'DL3P_SPLIT_MIN_N', 'DL3P_SPLIT_MIN_ROWS',
    'DL3P_SPLIT_MIN_ROWS_BN', 'DL3P_FUSE_BN_BWD', 'DL3P_FOLD_APPLY', 'DL3P_FOLD_APPLY_DGRAD', 'DL3P_FOLD_APPLY_STEM',
    'DL3P_FOLD_APPLY_DW_MIN_BYTES', 'DL3P_COLLECTIVES_IN_GRAPH', 'DL3P_BF16_DW_WINDOW')

SPELLINGS = ('', '0', '1', '2', '1single', 'rows', 'yes')
# attribute -> what the old read site made of each spelling (the old expression in the comment)
ON_UNLESS_0 = {s: s != '0' for s in SPELLINGS}                     # get(X, '1') != '0'   /   get(X, '1') == '0' -> off
ON_ONLY_1 = {s: s == '1' for s in SPELLINGS}                       # get(X, '0') == '1'
OFF_IF_EMPTY_OR_0 = {s: s not in ('', '0') for s in SPELLINGS}     # get(X, '1') not in ('', '0')
BOOLS = {
    'split_gemm': OFF_IF_EMPTY_OR_0, 'split_wgrad': OFF_IF_EMPTY_OR_0,
    'force_dist': {s: s != '' for s in SPELLINGS},                 # bool(get(X))
    'irb': ON_UNLESS_0, 'batched_wgrad': ON_UNLESS_0, 'ghost': ON_UNLESS_0, 'stem_direct': ON_UNLESS_0, 'grad_alias': ON_UNLESS_0,
    'fold_apply_dgrad': ON_UNLESS_0, 'fold_apply_stem': ON_UNLESS_0, 'collectives_in_graph': ON_UNLESS_0, 'bf16_dw_window': ON_UNLESS_0,
    'irb_debug_z': ON_ONLY_1, 'fold_resize': ON_ONLY_1, 'narrow_conv': ON_ONLY_1, 'bf16_fuse_bn_bwd': ON_ONLY_1,
}
ENUMS = {
    'fold_apply': {'0': 'off', '2': 'every_dw'},       # == '0' in three functions, != '2' in the fourth
    'fuse_bn_bwd': {'0': 'off', '1single': 'single'},  # == '0', == '1single'
    'fused_head': {'0': 'off', 'rows': 'rows'},        # == 'rows', not in ('0', 'rows')
}
ENUM_OTHER = {'fold_apply': 'default', 'fuse_bn_bwd': 'on', 'fused_head': 'tile'}
INTS = ('irb_min_rows', 'irb_s1_min_rows', 'ghost_min_rows', 'split_min_k', 'split_min_n', 'split_min_rows', 'split_min_rows_bn',
        'fold_apply_dw_min_bytes')


def test_defaults_are_the_literals_of_the_old_read_sites():
    o = opts()
    assert o.split_gemm is True and o.split_wgrad is True               # get(X, '1') not in ('', '0')
    assert o.force_dist is False                                        # bool(get(X))
    assert o.fused_head == 'rows'                                       # get(X, 'rows')
    assert o.irb is True and o.irb_debug_z is False                     # get(X, '1') == '0' -> off; get(X, '0') == '1'
    assert o.irb_min_rows is None                                       # int(get(X, '131072')), its presence asked separately
    assert o.irb_s1_min_rows == 400000
    assert o.batched_wgrad is True
    assert o.ghost is False and eo.GHOST_ON_BY_DEFAULT is False         # get(X, '1' if GHOST_ON_BY_DEFAULT else '0') == '0' -> off
    assert o.ghost_min_rows is None
    assert o.fold_resize is False and o.narrow_conv is False and o.bf16_fuse_bn_bwd is False
    assert o.stem_direct is True and o.grad_alias is True
    assert (o.split_min_k, o.split_min_n, o.split_min_rows, o.split_min_rows_bn) == (None,) * 4 and not o.split_pinned
    assert o.fuse_bn_bwd == 'on' and o.fold_apply == 'default'
    assert o.fold_apply_dgrad is True and o.fold_apply_stem is True
    assert o.fold_apply_dw_min_bytes == 250 << 20 == 262144000
    assert o.collectives_in_graph is True and o.bf16_dw_window is True


@pytest.mark.parametrize('attr', sorted(BOOLS))
def test_every_spelling_of_an_on_off_switch(attr):
    for s, want in BOOLS[attr].items():
        assert getattr(opts(**{attr.upper(): s}), attr) is want, (attr, s)


def test_the_odd_spellings():
    assert opts(FORCE_DIST='0').force_dist is True                      # any non-empty string
    assert opts(FORCE_DIST='').force_dist is False
    assert opts(SPLIT_GEMM='').split_gemm is False and opts(SPLIT_WGRAD='').split_wgrad is False
    assert opts(IRB='').irb is True and opts(GHOST='').ghost is True    # only '0' is off
    assert opts(NARROW_CONV='yes').narrow_conv is False                 # only '1' is on


@pytest.mark.parametrize('attr', sorted(ENUMS))
def test_every_spelling_of_an_enum(attr):
    for s in SPELLINGS + ('tile', '3'):
        assert getattr(opts(**{attr.upper(): s}), attr) == ENUMS[attr].get(s, ENUM_OTHER[attr]), (attr, s)


@pytest.mark.parametrize('attr', INTS)
def test_an_integer(attr):
    assert getattr(opts(**{attr.upper(): '12345'}), attr) == 12345
    assert getattr(opts(**{attr.upper(): '0'}), attr) == 0
    with pytest.raises(ValueError):
        opts(**{attr.upper(): 'yes'})


def test_presence_pins():
    for k in ('SPLIT_MIN_K', 'SPLIT_MIN_N', 'SPLIT_MIN_ROWS', 'SPLIT_MIN_ROWS_BN'):
        o = opts(**{k: '128'})
        assert o.split_pinned and getattr(o, k.lower()) == 128          # (the default value, set: still pinned)
        assert [getattr(o, j.lower()) for j in ('SPLIT_MIN_K', 'SPLIT_MIN_N', 'SPLIT_MIN_ROWS', 'SPLIT_MIN_ROWS_BN') if j != k] == [None] * 3
    assert opts(SPLIT_MIN_K='0').split_pinned
    assert opts(GHOST_MIN_ROWS='0').ghost_min_rows == 0 and opts().ghost_min_rows is None
    # the stride-1 threshold is inert while DL3P_IRB_MIN_ROWS is present: the snapshot says which case holds
    o = opts(IRB_MIN_ROWS='131072', IRB_S1_MIN_ROWS='7')
    assert o.irb_min_rows == 131072 and o.irb_s1_min_rows == 7
    assert opts(IRB_S1_MIN_ROWS='7').irb_min_rows is None


def test_the_snapshot_is_immutable_and_ignores_later_changes():
    env = {'DL3P_IRB': '0'}
    o = eo.ExecOptions.from_env(env)
    env['DL3P_IRB'] = '1'
    assert o.irb is False
    with pytest.raises(AttributeError):
        o.irb = True
    with pytest.raises(AttributeError):
        del o.irb
    with pytest.raises(AttributeError):
        o.something_new = 1
    assert not hasattr(o, '__dict__')


def test_the_table_is_complete_and_executor_reads_nothing_else():
    assert sorted(r[0] for r in eo.ROWS) == sorted(NAMES)
    assert len({r[1] for r in eo.ROWS}) == len(eo.ROWS) and all(r[4] for r in eo.ROWS)
    src = open(os.path.join(PKG_DIR, 'executor.py')).read()
    assert 'os.environ' not in src and 'getenv' not in src
    assert re.search(r'^\s*(import os\b|from os\b)', src, re.M) is None
    # the switches executor.py speaks of are rows
    assert set(re.findall(r'DL3P_[A-Z0-9_]+', src)) <= set(NAMES)
    # exec_options.py imports nothing but os
    tree = ast.parse(open(os.path.join(PKG_DIR, 'exec_options.py')).read())
    imported = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    assert imported == ['os'] and not any(isinstance(n, ast.ImportFrom) for n in ast.walk(tree))
