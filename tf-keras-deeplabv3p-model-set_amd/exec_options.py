"""The executor's switches: one table of the DL3P_* environment variables executor.py obeys, and the immutable snapshot an Executor
takes of them when it is built (ExecOptions.from_env, the only reader).  A row: environment name, attribute of the snapshot,
parser of the variable's string, value where the variable is absent, what the switch does and where it was measured.  The names,
defaults and accepted spellings are the interface.  model.py, layers.py and the C library keep their own switches."""
import os

GHOST_ON_BY_DEFAULT = False                         # (the `ghost` row: a measured table turns it into the default rule)
# the parser kinds
unless_0 = lambda s: s != '0'                       # on unless '0'
only_1 = lambda s: s == '1'                         # on only if '1'
not_empty_or_0 = lambda s: s not in ('', '0')       # off if '' or '0'
non_empty = bool                                    # on if non-empty, '0' included
enum = lambda named, other: lambda s: named.get(s, other)

ROWS = (
    ('DL3P_SPLIT_GEMM', 'split_gemm', not_empty_or_0, True,
     'The compute-bound pointwise convs (K >= 128, N >= 128, >= 16384 rows) run as fp32-accurate split-bf16 GEMMs on the bf16 matrix '
     'pipe (csrc/pw_split.hip; DESIGN 4c): every fp32 operand split exactly into three bf16 pieces, six cross products accumulated in '
     'fp32 -- parity held at the tolerances of the fp32-input MFMA kernels (tests/test_split_gemm_gpu.py, and the whole GPU suite '
     'runs with it).  On by default since round 3; 0 (bench.py --split-gemm 0) keeps every GEMM on the fp32-input MFMA kernels.  '
     'Also taken when the parameter store is built (executor.split_gemm_enabled)'),
    ('DL3P_SPLIT_WGRAD', 'split_wgrad', not_empty_or_0, True,
     'the weight gradients pick the split kernel inside the library (fp32, with split_gemm)'),
    ('DL3P_FORCE_DIST', 'force_dist', non_empty, False, 'exercises the collective path on a single rank (plumbing test)'),
    ('DL3P_FUSED_HEAD', 'fused_head', enum({'0': 'off', 'rows': 'rows'}, 'tile'), 'rows',
     'The fused training heads (plain cross-entropy only).  rows: dl3p_head_train_rows (x / y separable: a quarter of the '
     'full-resolution gradient\'s traffic), the default where it is served; 0: the two-kernel path; anything else (tile): '
     'dl3p_head_train (one launch, no workspace, bit-identical to the two-kernel path but measured slower: 506 us vs 141 + 165 us '
     'at batch 16)'),
    ('DL3P_IRB', 'irb', unless_0, True, 'fused inverted-residual blocks (DESIGN 4e: 12.75 -> 12.22 ms on the headline step)'),
    ('DL3P_IRB_DEBUG_Z', 'irb_debug_z', only_1, False,
     'the forward ALSO writes the expand output with the unfused kernel, for tests that inspect every conv output (activation '
     'branch patterns); the fused kernels never read it'),
    ('DL3P_IRB_MIN_ROWS', 'irb_min_rows', int, None,
     'rows (N*H*W) from which a block is fused; absent: 131072, measured on the headline step (DESIGN 4e): the 257 x 257 and '
     '129 x 129 blocks pay (12.75 -> 12.22 ms), the 65 x 65 ones do not (12.47 with them).  Setting it lifts the threshold below'),
    ('DL3P_IRB_S1_MIN_ROWS', 'irb_s1_min_rows', int, 400000,
     'rows from which a block with a STRIDE-1 depthwise conv is fused, while DL3P_IRB_MIN_ROWS is absent: such a conv reaches every '
     'expanded pixel with all nine taps (a stride-2 one with 2.25 on average), and the recomputing backward then costs what the '
     'unfused kernels cost (129 x 129 x 24 -> 144: 437 against 421 us per step)'),
    ('DL3P_BATCHED_WGRAD', 'batched_wgrad', unless_0, True,
     'weight gradients leave slabs for ONE dl3p_reduce_rows_batched pair (65 reduce launches of 5-13 us each otherwise); 0, an A/B '
     'switch, also keeps a training executor off the fused inverted-residual blocks, whose backward leaves slabs'),
    ('DL3P_GHOST', 'ghost', unless_0, GHOST_ON_BY_DEFAULT,
     'ghost modules on inference coefficients as one dl3p_ghost_fwd launch, for the module shapes of executor.GHOST_DEFAULT from '
     'executor.GHOST_MIN_ROWS rows up (DESIGN 4k).  Opt-in: the fused forward has NOT been measured against the pair of launches it '
     'replaces (scripts/bench_ghost.py is the measurement; docs/experiments.md)'),
    ('DL3P_GHOST_MIN_ROWS', 'ghost_min_rows', int, None,
     'replaces executor.GHOST_MIN_ROWS AND, by being set, lifts the shape table executor.GHOST_DEFAULT'),
    ('DL3P_FOLD_RESIZE', 'fold_resize', only_1, False,
     'the decoder resize formed inside the depthwise conv that reads it (Executor._find_up).  Opt-in: built, bit-identical, and '
     'measured SLOWER on MI355X -- 12.62 against 12.02 ms per headline step (profiles/r06_resize_fold.txt): the fused forward takes '
     '468 us against 140 + 80 for the pair it replaces.  Four dependent 16-byte loads and three lerps per input vector turn an '
     'HBM-bound window kernel (2 waves per SIMD at 217-256 registers) into a latency-bound one: the compiler serialises the '
     'conditional gathers (57 s_waitcnt vmcnt(0) in the loop against 9)'),
    ('DL3P_STEM_DIRECT', 'stem_direct', unless_0, True,
     'the RGB stem as the LDS-staged implicit GEMM (csrc/stem.hip) instead of im2col + GEMM'),
    ('DL3P_NARROW_CONV', 'narrow_conv', only_1, False,
     'the direct kernels of csrc/conv_narrow.hip for PeleeNet\'s dense layers.  Opt-in: measured slower than the implicit GEMM in '
     'every role and at every PeleeNet shape (27.0 against 16.4 ms per 512 x 512 batch-16 step, DESIGN 4h)'),
    ('DL3P_BF16_FUSE_BN_BWD', 'bf16_fuse_bn_bwd', only_1, False,
     'bf16: the pointwise data gradients carry the BatchNorm-backward sums.  Opt-in: measured slower than the separate reduce pass '
     '(the epilogue meets z in 8-byte pieces: MobileNetV2 513x513 batch 16 12.37 against 11.83 ms, MobileNetV3-Large 1024x2048 '
     'batch 1 6.92 against 6.86)'),
    ('DL3P_GRAD_ALIAS', 'grad_alias', unless_0, True,
     'a residual Add hands its gradient to a BatchNorm branch unchanged: that BatchNorm\'s backward reads it where it is (no copy '
     'into the branch\'s own buffer, one launch less per Add)'),
    ('DL3P_SPLIT_MIN_K', 'split_min_k', int, None,
     'the rule of Executor._use_sb (measured: scripts/micro/sb_gemm.py): shortest reduction, 128 where absent.  Any of the four '
     'DL3P_SPLIT_MIN_* present pins the rule: the measured per-launch verdicts (csrc/sb_tuned.h) are not asked'),
    ('DL3P_SPLIT_MIN_N', 'split_min_n', int, None, '... narrowest output, 128 where absent'),
    ('DL3P_SPLIT_MIN_ROWS', 'split_min_rows', int, None, '... fewest rows, 16384 where absent'),
    ('DL3P_SPLIT_MIN_ROWS_BN', 'split_min_rows_bn', int, None,
     '... fewest rows of a data gradient that carries BatchNorm sums, 60000 where absent'),
    ('DL3P_FUSE_BN_BWD', 'fuse_bn_bwd', enum({'0': 'off', '1single': 'single'}, 'on'), 'on',
     'BatchNorm-backward sums ride on the data gradient of the first reader: 0 never, 1single only where the BatchNorm has one '
     'reader, anything else on'),
    ('DL3P_FOLD_APPLY', 'fold_apply', enum({'0': 'off', '2': 'every_dw'}, 'default'), 'default',
     'the BatchNorm-backward apply pass folded into the gradients of the conv in front: 0 never, 2 into every depthwise conv too, '
     'anything else the depthwise convs from DL3P_FOLD_APPLY_DW_MIN_BYTES up'),
    ('DL3P_FOLD_APPLY_DGRAD', 'fold_apply_dgrad', unless_0, True,
     '... into the DATA gradient of the long decoder layers (row-stationary split GEMM)'),
    ('DL3P_FOLD_APPLY_STEM', 'fold_apply_stem', unless_0, True, '... into the weight gradient of the direct stem kernel'),
    ('DL3P_FOLD_APPLY_DW_MIN_BYTES', 'fold_apply_dw_min_bytes', int, 250 << 20,
     '... tensor bytes from which a depthwise conv takes it.  Measured on MI355X: on every depthwise conv the window kernel with the '
     'fold takes as much longer as the apply pass it replaces took (MobileNetV2 step 14.12 ms against 14.05 with the pointwise '
     'folds alone, 14.25 without any).  On the two 129 x 129 decoder layers alone (324 / 272 MB tensors: the apply pass is 174 / 136 '
     'us of pure traffic) the folded weight gradient is 319 / 236 us against 329 / 264 for the pair it replaces (round 5, same '
     'box): those two take it'),
    ('DL3P_COLLECTIVES_IN_GRAPH', 'collectives_in_graph', unless_0, True,
     'capture() takes the collectives into the hipGraphs; 0 forces the segmented fallback'),
    ('DL3P_BF16_DW_WINDOW', 'bf16_dw_window', unless_0, True,
     'install_probe() names the bf16 sliding-window depthwise kernel (the library reads the variable itself, once per process)'),
)


class ExecOptions:
    """every row's value, by attribute name, fixed when it is made"""
    __slots__ = tuple(r[1] for r in ROWS)

    @classmethod
    def from_env(cls, environ=os.environ):
        self = object.__new__(cls)
        for name, attr, parser, absent, _ in ROWS:
            s = environ.get(name)
            object.__setattr__(self, attr, absent if s is None else parser(s))
        return self

    def __setattr__(self, k, v=None):
        raise AttributeError('ExecOptions is fixed when the executor is built')
    __delattr__ = __setattr__

    @property
    def split_pinned(self):
        """any DL3P_SPLIT_MIN_* present: the rule stands alone"""
        return any(v is not None for v in (self.split_min_k, self.split_min_n, self.split_min_rows, self.split_min_rows_bn))
