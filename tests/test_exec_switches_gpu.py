"""Every switch of exec_options.py still decides something: one training executor built with the switch at its default and one with it
at its other value, and the entry points of the traced plans (Plan.labels) counted.  A switch that stopped being read leaves the
two counts equal and fails here; the on/off parity tests elsewhere compare numbers and cannot see that.

The expected counts are those of the launch lists of executor.py as it was before the table existed (every model and state below was
traced with it once), not of the code under test.  No kernel output is compared here.

Models: MobileNetV2 65 x 65, batch 2, 21 classes wherever the switch decides something there -- on top of DL3P_IRB_MIN_ROWS=1
(fused inverted-residual blocks at that size) or the four DL3P_SPLIT_MIN_* pins (split GEMM at that size) where the route needs
them; PeleeNet for the narrow convs, a frozen GhostNet backbone for the ghost modules, the bf16 policy for the two bf16 switches,
the identical-ranks double of test_dist_gpu.py for the collectives.  Two switches decide nothing below 131072 rows
(DL3P_IRB_S1_MIN_ROWS, DL3P_FOLD_APPLY_DGRAD): MobileNetV2 513 x 513, batch 8, the size of
test_model_gpu.py::test_the_apply_folded_into_the_data_gradient_does_not_change_gradients.

Switches that change no entry-point name at any of these shapes, and what is asserted instead:
DL3P_SPLIT_WGRAD (the library routes the weight gradients itself: Executor._split_wgrad, the option the executor hands it),
DL3P_COLLECTIVES_IN_GRAPH (how capture() segments the plans), DL3P_BF16_DW_WINDOW (the kernel name install_probe() gives)."""
import collections

import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu

PINS = {'DL3P_SPLIT_MIN_K': '32', 'DL3P_SPLIT_MIN_N': '16', 'DL3P_SPLIT_MIN_ROWS': '64', 'DL3P_SPLIT_MIN_ROWS_BN': '64'}
IRB1 = {'DL3P_IRB_MIN_ROWS': '1'}
BASE = dict(PINS, **IRB1)


def _without(k):
    return {a: b for a, b in PINS.items() if a != k}


def _model(kind):
    pkg = load_pkg()
    loss = pkg.SparseCategoricalCrossEntropy(ignore_index=255)
    if kind in ('mnv2_dist1', 'mnv2_dist2'):
        from test_dist_gpu import _two_identical_ranks
        m = pkg.get_deeplabv3p_model('mobilenetv2', 21, (65, 65), 16, training=True)
        return m.compile(optimizer=pkg.SGD(0.01), loss=loss, distributed=_two_identical_ranks(world=int(kind[-1]))()), 2
    mt, hw, n, kw = {'mnv2': ('mobilenetv2', 65, 2, {}), 'mnv2_bf16': ('mobilenetv2', 65, 2, {}), 'mnv2_big': ('mobilenetv2', 513, 8, {}),
                     'peleenet': ('peleenet', 64, 2, {}), 'ghost_frozen': ('ghostnet', 64, 2, {'freeze_level': 1})}[kind]
    mp = pkg.mixed_precision
    try:
        if kind == 'mnv2_bf16':
            mp.set_global_policy('mixed_bfloat16')
        m = pkg.get_deeplabv3p_model(mt, 21, (hw, hw), 16, training=True, **kw)
    finally:
        mp.set_global_policy('float32')
    return m.compile(optimizer=pkg.SGD(0.01), loss=loss, distributed=False), n


def _executor(kind, env):
    """a fresh model (so that its parameter store is built under `env` too) and its training executor"""
    rows = load_pkg('exec_options').ROWS
    with pytest.MonkeyPatch.context() as mp:
        for r in rows:
            mp.delenv(r[0], raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        m, n = _model(kind)
        return m, m._executor(n, True)


_counted = {}


def _count(kind, env):
    """entry point -> launches in the three plans of that executor (cached: the default of a model serves every case on it)"""
    key = (kind, tuple(sorted(env.items())))
    if key not in _counted:
        m, ex = _executor(kind, env)
        _counted[key] = collections.Counter(name for plan in (ex.fwd, ex.bwd, ex.opt) for name, _ in plan.labels)
        del m, ex
        if kind == 'mnv2_big':
            torch.cuda.empty_cache()
    return _counted[key]


@pytest.fixture(scope='module', autouse=True)
def _drop_the_cache():
    yield
    _counted.clear()
    torch.cuda.empty_cache()


# (switch and value, model, the environment both executors share, {entry point: (launches without, launches with the value)})
CASES = [
    ('SPLIT_GEMM=0', 'mnv2', BASE, {'dl3p_pwconv_fwd_sb': (5, 0), 'dl3p_pwconv_bwd_data_sb': (4, 0), 'dl3p_split_bf16x3_batch': (2, 0)}),
    ('SPLIT_GEMM=', 'mnv2', BASE, {'dl3p_pwconv_fwd_sb': (5, 0), 'dl3p_pwconv_bwd_data_sb': (4, 0), 'dl3p_split_bf16x3_batch': (2, 0)}),
    ('FORCE_DIST=1', 'mnv2_dist1', {}, {'dl3p_bn_reduce_partials': (0, 130), 'py': (0, 182)}),
    ('FORCE_DIST=0', 'mnv2_dist1', {}, {'dl3p_bn_reduce_partials': (0, 130), 'py': (0, 182)}),        # any non-empty string
    ('FUSED_HEAD=0', 'mnv2', {}, {'dl3p_head_train_rows': (1, 0), 'dl3p_upsample_softmax_loss': (0, 1), 'dl3p_head_train': (0, 0)}),
    ('FUSED_HEAD=tile', 'mnv2', {}, {'dl3p_head_train_rows': (1, 0), 'dl3p_upsample_softmax_loss': (0, 0), 'dl3p_head_train': (0, 1)}),
    ('IRB=0', 'mnv2', BASE, {'dl3p_irb_fwd': (6, 0), 'dl3p_irb_bwd_data': (6, 0)}),
    ('IRB_DEBUG_Z=1', 'mnv2', BASE, {'dl3p_irb_fwd': (6, 6), 'dl3p_pwconv_fwd_wt': (32, 38)}),
    ('IRB_MIN_ROWS=1', 'mnv2', {}, {'dl3p_irb_fwd': (0, 6), 'dl3p_dwconv2d_fwd': (22, 16)}),
    ('IRB_S1_MIN_ROWS=1', 'mnv2_big', {}, {'dl3p_irb_fwd': (2, 3)}),
    # (both readers of the one flag: the reduction of the slabs goes, and with it the fused blocks of a training executor)
    ('BATCHED_WGRAD=0', 'mnv2', BASE, {'dl3p_reduce_rows_batched': (1, 0), 'dl3p_irb_fwd': (6, 0), 'dl3p_pwconv_bwd_weight': (28, 43)}),
    ('GHOST=1', 'ghost_frozen', {}, {'dl3p_ghost_fwd': (0, 7), 'dl3p_dwconv2d_fwd': (46, 39)}),
    ('GHOST_MIN_ROWS=999999999', 'ghost_frozen', {'DL3P_GHOST': '1'}, {'dl3p_ghost_fwd': (7, 0)}),
    ('FOLD_RESIZE=1', 'mnv2', {}, {'dl3p_dw_upsampled_input': (0, 2), 'dl3p_resize_bilinear_fwd': (2, 1)}),
    ('STEM_DIRECT=0', 'mnv2', {}, {'dl3p_stem_conv_fwd': (1, 0), 'dl3p_im2col': (0, 1)}),
    ('NARROW_CONV=1', 'peleenet', {}, {'dl3p_conv_narrow_fwd': (0, 63), 'dl3p_conv2d_gemm_fwd': (64, 1)}),
    ('BF16_FUSE_BN_BWD=1', 'mnv2_bf16', {}, {'dl3p_pwconv_bwd_data_bn_bf16': (0, 11), 'dl3p_bn_bwd_reduce_bf16': (65, 54)}),
    ('GRAD_ALIAS=0', 'mnv2', {}, {'dl3p_scale_mask_bwd': (1, 21)}),
    # each threshold of the pinned rule, against the rule with that one left at its default (128, 128, 16384, 60000) ...
    ('SPLIT_MIN_K=32', 'mnv2', _without('DL3P_SPLIT_MIN_K'), {'dl3p_pwconv_fwd_sb': (5, 8), 'dl3p_pwconv_bwd_data_sb': (5, 7)}),
    ('SPLIT_MIN_N=16', 'mnv2', _without('DL3P_SPLIT_MIN_N'), {'dl3p_pwconv_fwd_sb': (5, 8), 'dl3p_pwconv_bwd_data_sb': (4, 7)}),
    ('SPLIT_MIN_ROWS=64', 'mnv2', _without('DL3P_SPLIT_MIN_ROWS'), {'dl3p_pwconv_fwd_sb': (0, 8), 'dl3p_pwconv_bwd_data_sb': (0, 7)}),
    ('SPLIT_MIN_ROWS_BN=64', 'mnv2', _without('DL3P_SPLIT_MIN_ROWS_BN'), {'dl3p_pwconv_fwd_sb': (8, 8), 'dl3p_pwconv_bwd_data_sb': (0, 7)}),
    # ... and one of them alone, against none
    ('SPLIT_MIN_ROWS=64', 'mnv2', {}, {'dl3p_pwconv_fwd_sb': (0, 2)}),
    ('FUSE_BN_BWD=0', 'mnv2', {}, {'dl3p_pwconv_bwd_data_bn': (39, 0), 'dl3p_dwconv2d_bwd_data_bn': (19, 0), 'dl3p_bn_bwd_reduce': (7, 65)}),
    ('FUSE_BN_BWD=1single', 'mnv2', {}, {'dl3p_pwconv_bwd_data_bn': (39, 34), 'dl3p_dwconv2d_bwd_data_bn': (19, 18), 'dl3p_bn_bwd_reduce': (7, 13)}),
    ('FOLD_APPLY=0', 'mnv2', {}, {'dl3p_pwconv_bwd_weight_slabs_bn': (10, 0), 'dl3p_stem_conv_bwd_weight_slabs_bn': (1, 0), 'dl3p_bn_bwd_apply': (54, 65)}),
    ('FOLD_APPLY=2', 'mnv2', {}, {'dl3p_dwconv2d_bwd_weight_slabs_bn': (0, 8), 'dl3p_pwconv_bwd_weight_slabs_bn': (10, 10), 'dl3p_bn_bwd_apply': (54, 46)}),
    ('FOLD_APPLY_DGRAD=0', 'mnv2_big', {}, {'dl3p_pwconv_bwd_data_sb_apply': (2, 0), 'dl3p_pwconv_bwd_data_sb': (0, 2), 'dl3p_bn_bwd_apply': (48, 50)}),
    ('FOLD_APPLY_STEM=0', 'mnv2', {}, {'dl3p_stem_conv_bwd_weight_slabs_bn': (1, 0), 'dl3p_stem_conv_bwd_weight_slabs': (0, 1)}),
    ('FOLD_APPLY_DW_MIN_BYTES=1', 'mnv2', {}, {'dl3p_dwconv2d_bwd_weight_slabs_bn': (0, 8), 'dl3p_bn_bwd_apply': (54, 46)}),
]


@pytest.mark.parametrize('switch,kind,shared,want', CASES, ids=['%s-%s%s' % (c[0], c[1], '+%d' % len(c[2]) if c[2] else '') for c in CASES])
def test_the_switch_changes_the_traced_launches(switch, kind, shared, want):
    k, v = switch.split('=')
    ref, got = _count(kind, shared), _count(kind, dict(shared, **{'DL3P_' + k: v}))
    seen = {name: (ref[name], got[name]) for name in want}
    print(switch, kind, seen)
    assert seen == want
    assert any(a != b for a, b in want.values())


def test_the_stride_1_threshold_is_inert_while_the_row_threshold_is_set():
    """DL3P_IRB_MIN_ROWS at its own default value, but present: the 129 x 129 stride-1 block (133128 rows) is fused whatever
    DL3P_IRB_S1_MIN_ROWS says -- three fused blocks, against two with neither variable set"""
    assert _count('mnv2_big', {})['dl3p_irb_fwd'] == 2
    assert _count('mnv2_big', {'DL3P_IRB_MIN_ROWS': '131072'})['dl3p_irb_fwd'] == 3
    assert _count('mnv2_big', {'DL3P_IRB_MIN_ROWS': '131072', 'DL3P_IRB_S1_MIN_ROWS': '999999999'})['dl3p_irb_fwd'] == 3


def test_split_wgrad_reaches_the_option_the_library_routes_by():
    """DL3P_SPLIT_WGRAD (and DL3P_SPLIT_GEMM, which it needs): no entry-point name changes, Executor._split_wgrad does"""
    for env, want in (({}, 1), ({'DL3P_SPLIT_WGRAD': '0'}, 0), ({'DL3P_SPLIT_WGRAD': ''}, 0), ({'DL3P_SPLIT_GEMM': '0'}, 0)):
        m, ex = _executor('mnv2', env)
        assert ex._split_wgrad == want, env
        assert ex.L.get_option(b'split_wgrad') == want, env
    m, ex = _executor('mnv2', {})            # (the option is process-wide: leave the default behind)
    assert ex.L.get_option(b'split_wgrad') == 1


def test_collectives_in_graph_decides_how_capture_segments_the_plans():
    """DL3P_COLLECTIVES_IN_GRAPH, taken when the executor is built: two identical ranks with SyncBatchNorm, one hipGraph per plan
    by default, with 0 a graph per run of kernels and the collectives between them (119 and 241 segments, 60 and 118 of them graphs)"""
    segs = {}
    for v in ('1', '0'):
        m, ex = _executor('mnv2_dist2', {'DL3P_COLLECTIVES_IN_GRAPH': v})
        assert ex.sync_bn
        with pytest.MonkeyPatch.context() as mp:          # what the environment holds at capture() no longer matters
            mp.setenv('DL3P_COLLECTIVES_IN_GRAPH', '1' if v == '0' else '0')
            ex.capture()
        torch.cuda.synchronize()
        segs[v] = [(len(p.segments), sum(isinstance(s, torch.cuda.CUDAGraph) for s in p.segments)) for p in (ex.fwd, ex.bwd, ex.opt)]
        del m, ex
    print(segs)
    assert segs['1'] == [(1, 1), (1, 1), (1, 1)]
    assert segs['0'] == [(119, 60), (241, 118), (1, 1)]


def test_bf16_dw_window_decides_the_kernel_name_of_the_probe():
    """DL3P_BF16_DW_WINDOW, taken when the executor is built: the name install_probe() gives the bf16 3x3 depthwise launch"""
    names = {}
    for v in ('1', '0'):
        m, ex = _executor('mnv2_bf16', {'DL3P_BF16_DW_WINDOW': v})
        assert ex.bf16
        names[v] = [ex.install_probe(n).kernel_name for n in ('decoder_conv0_depthwise', 'expanded_conv_1_depthwise', 'aspp1_depthwise')]
    assert names['1'] == ['dwb_fwd_seg<3, 4, 1', 'dwb_fwd_seg<3, 2, 2', 'dwb_fwd_strip<8, 3']
    assert names['0'] == ['dwb_fwd_strip<8, 3', 'dwb_fwd<8, 3', 'dwb_fwd_strip<8, 3']
