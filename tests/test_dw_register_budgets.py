"""Register budgets of the depthwise window kernels (csrc/dwconv.hip): the file is compiled for gfx950 here (hipcc cross-compiles
without a GPU) with build.py's flags plus -Rpass-analysis=kernel-resource-usage, and every dw_fwd_seg / dw_bwd_weight_seg
instantiation the headline step (MobileNetV2-DeepLabV3+, 513 x 513, batch 16) launches is held to a committed budget.

These are bandwidth kernels: how much memory latency they hide is the number of waves a SIMD holds, floor(512 / (VGPRs + AGPRs rounded
up to 8)) on gfx950.  Twice that number moved without anybody looking: the counted-wait rows, folded into every dw_fwd_seg
instantiation, took <3,2,1,2> from three waves to two (+150 us per step on layers that never run those rows), and the folded weight
gradient sat at 256 + 2 registers -- ONE wave -- for two rounds (docs/experiments.md, "Depthwise window kernels: register budgets").

Budget = (max VGPRs + AGPRs, min waves per SIMD); scratch is 0 everywhere.  The register figure is what the compiler gave when the
budget was committed plus two (a compiler may shuffle a register or two), never past the limit of the wave class, which is what binds.
"""
import importlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

# <KS, TW, S, PRO, BNB, UP, FAST_K> -> (max VGPRs + AGPRs, min waves per SIMD)
FWD = {
    # general rows (FAST_K = 0): the figures of the kernel before the counted-wait rows existed
    (3, 2, 1, 2, 0, 0, 0): (168, 3),       # expanded_conv_depthwise, blocks 11-16
    (3, 2, 1, 1, 0, 0, 0): (156, 3),
    (3, 2, 1, 0, 1, 0, 0): (194, 2),       # data gradient + BatchNorm-backward statistics
    (3, 2, 2, 2, 0, 0, 0): (207, 2),
    (3, 4, 1, 2, 0, 0, 0): (219, 2),
    (3, 4, 1, 0, 0, 0, 0): (190, 2),       # plain data gradient
    (3, 4, 1, 0, 1, 0, 0): (242, 2),
    # counted-wait rows: the two decoder forwards (outputs >= 200 MB)
    (3, 4, 1, 2, 0, 0, 1): (227, 2),
}
# <KS, TW, S, PRO, BNA, UP>
WGRAD = {
    (3, 4, 1, 2, 1, 0): (256, 2),          # BatchNorm-backward apply folded in: decoder_conv0 / conv1_depthwise, ~1 GB per launch
    (3, 4, 1, 1, 1, 0): (256, 2),          # (the same kernel behind a BatchNorm without activation)
    (3, 4, 1, 2, 0, 0): (207, 2),
    (3, 4, 1, 1, 0, 0): (196, 2),
    (3, 2, 2, 2, 0, 0): (200, 2),
}


def waves_per_simd(regs):
    return min(8, 512 // ((regs + 7) // 8 * 8))


def parse_remarks(text):
    """-> {(kernel, template arguments): {'VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy'}} from the resource-usage remarks"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            # _Z10dw_fwd_segILi3ELi2ELi1ELi2ELb0ELb0ELb0EEv8DwParams: integral and bool template arguments only
            mm = re.match(r'_Z\d+(dw_fwd_seg|dw_bwd_weight_seg)I((?:L[ib]\d+E)+)Ev8DwParams$', m.group(1))
            cur = None
            if mm:
                cur = out.setdefault((mm.group(1), tuple(int(v) for v in re.findall(r'L[ib](\d+)E', mm.group(2)))), {})
            continue
        m = re.search(r'remark:\s+(VGPRs|AGPRs|ScratchSize|Occupancy)(?: \[[^\]]*\])?: (\d+)', line)   # (not "VGPRs Spill")
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


@pytest.fixture(scope='module')
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    sys.path.insert(0, ROOT)
    build = importlib.import_module(PKG + '.build')
    d = tmp_path_factory.mktemp('dwru')
    src = os.path.join(build.CSRC, 'dwconv.hip')
    cmd = [HIPCC] + build.FLAGS + build.EXTRA.get('dwconv.hip', []) + [
        '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c', src, '-o', os.path.join(str(d), 'dwconv.o')]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    u = parse_remarks(r.stderr)
    assert u, 'no resource-usage remarks in the compiler output'
    return u


def _check(usage, kernel, table):
    bad = []
    for targs, (max_regs, min_waves) in sorted(table.items()):
        assert (kernel, targs) in usage, '%s<%s> is not instantiated any more: update the budget table' % (kernel, targs)
        u = usage[(kernel, targs)]
        regs = u['VGPRs'] + u['AGPRs']
        waves = min(waves_per_simd(regs), u['Occupancy'])
        print('%s<%s>: %d VGPRs + %d AGPRs, scratch %d, %d waves per SIMD (budget %d, %d)' % (
            kernel, ','.join(map(str, targs)), u['VGPRs'], u['AGPRs'], u['ScratchSize'], waves, max_regs, min_waves))
        if regs > max_regs or waves < min_waves or u['ScratchSize'] != 0:
            bad.append((targs, u))
    assert not bad, bad


def test_budgets_respect_their_wave_class():
    for table in (FWD, WGRAD):
        for targs, (max_regs, min_waves) in table.items():
            assert waves_per_simd(max_regs) >= min_waves, targs


def test_forward_window_kernels_of_the_headline_step(usage):
    _check(usage, 'dw_fwd_seg', FWD)


def test_weight_gradient_window_kernels_of_the_headline_step(usage):
    _check(usage, 'dw_bwd_weight_seg', WGRAD)


def test_the_general_forward_kernel_carries_no_counted_wait_code(usage):
    """the counted-wait rows are a kernel of their own (template argument FAST_K) and exist for forward launches only: behind a
    BatchNorm prologue, no BatchNorm-backward statistics, no upsampled input"""
    fast = [t for (k, t) in usage if k == 'dw_fwd_seg' and t[6] == 1]
    assert fast and all(t[3] != 0 and t[4] == 0 and t[5] == 0 for t in fast), fast
    for t in fast:
        assert ('dw_fwd_seg', t[:6] + (0,)) in usage, t


def test_upsampled_input_weight_gradients_do_not_spill(usage):
    """the opt-in UP instantiations keep the default occupancy bound (under two waves per SIMD they spill 28-164 bytes per lane)"""
    up = [(t, u) for (k, t), u in usage.items() if k == 'dw_bwd_weight_seg' and t[5] == 1]
    assert up and all(u['ScratchSize'] == 0 for _, u in up), up
