"""Fused ghost-module forward (csrc/ghost_fwd.hip, Executor._find_ghost): what it buys on the MI355X.

  (a) modules   each of the seven high-resolution ghost modules of a 512 x 512 GhostNet at batch 16 (K -> C on the 256 x 256 and
                128 x 128 maps): dl3p_ghost_fwd against the pair it replaces, dl3p_pwconv_fwd_wt + dl3p_dwconv2d_fwd -- kernels this
                file's subject does not touch.  Device events around windows of launches, the two arms alternated in one process,
                REPEATS windows each; the pair is also timed against ITSELF (two series of windows) to show the spread.
  (b) predict   images/s of the inference forward of ghostnet and ghostnet_lite at 16 x 512 x 512 (resident batch, hipGraph
                replay) with DL3P_GHOST=1 (every module the kernel serves: DL3P_GHOST_MIN_ROWS=0) and DL3P_GHOST=0
  (c) frozen    the freeze_level=1 train step the same way
  (d) train     the plain ghostnet train step at 16 x 512 x 512 and its launch count, for the record

    python scripts/bench_ghost.py [--modules-only] [--out FILE]

Prints a markdown table (docs/experiments.md keeps the last one)."""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PKG = 'tf-keras-deeplabv3p-model-set_amd'
REPEATS = 7
# (K, C, map size) of the ghost modules on the 256 x 256 and 128 x 128 maps of a 512 x 512 input (deeplabv3p_ghostnet.py:204-229)
MODULES = [(16, 8, 256), (16, 8, 256), (16, 24, 256), (48, 12, 128), (24, 36, 128), (24, 36, 128), (72, 12, 128)]


def window_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def spread(v):
    return statistics.median(v), min(v), max(v)


def bench_modules(pkg, lines, N=16):
    ops = importlib.import_module(PKG + '.ops')
    f = dict(dtype=torch.float32, device='cuda')
    lines.append('| module | rows | fused us (min..max) | pair us (min..max) | pair again us | spread of the pair | fused / pair | '
                 'fused GB/s |')
    lines.append('|---|---|---|---|---|---|---|---|')
    seen = set()
    for K, C, S in MODULES:
        if (K, C, S) in seen:
            continue
        seen.add((K, C, S))
        x = torch.randn((N, S, S, K), **f)
        xs, xh = torch.rand(K, **f) + 0.5, torch.randn(K, **f) * 0.1
        w1 = torch.randn((K, C), **f) / K ** 0.5
        w1t = w1.t().contiguous()
        s1, h1 = torch.rand(C, **f) + 0.5, torch.randn(C, **f) * 0.1
        wdw = torch.randn((3, 3, C), **f) / 3
        y = torch.empty((N, S, S, 2 * C), **f)
        kw = dict(in_scale=xs, in_shift=xh, in_act=ops.ACT_RELU)

        def fused():
            ops.ghost_fwd(x, w1, s1, h1, ops.ACT_RELU, wdw, out=y, **kw)

        def pair():
            ops.pwconv_fwd_wt(x, w1t, out=y[..., :C], **kw)
            ops.dwconv2d_fwd(y[..., :C], wdw, in_scale=s1, in_shift=h1, in_act=ops.ACT_RELU, out=y[..., C:])
        rows = N * S * S
        reps = max(20, int(4e9 / (rows * 4 * (K + 3 * C))))       # ~4 GB of traffic per window: well above 0.1 s
        for fn in (fused, pair):
            window_us(fn, reps)                                     # warm-up
        tf, tp, tq = [], [], []
        for _ in range(REPEATS):
            tf.append(window_us(fused, reps))
            tp.append(window_us(pair, reps))
            tq.append(window_us(pair, reps))
        (mf, lf, hf), (mp, lp, hp), (mq, _, _) = spread(tf), spread(tp), spread(tq)
        sp = max(abs(mp - mq), hp - lp) / mp
        lines.append('| %d -> %d @ %d x %d | %d | %.1f (%.1f..%.1f) | %.1f (%.1f..%.1f) | %.1f | %.1f %% | %.3f | %.0f |' % (
            K, C, S, S, rows, mf, lf, hf, mp, lp, hp, mq, sp * 100, mf / mp, rows * 4 * (K + 2 * C) / mf / 1e3))
        del x, y


def _inputs(N, H, W, C):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
    y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
    y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
    return x, y


def _executor(pkg, mt, ghost, training, freeze_level, x, y, N, H, W, C):
    """an executor built under DL3P_GHOST = ghost (with every served module fused when on), warmed up and captured"""
    old = {k: os.environ.get(k) for k in ('DL3P_GHOST', 'DL3P_GHOST_MIN_ROWS')}
    os.environ['DL3P_GHOST'] = ghost
    os.environ['DL3P_GHOST_MIN_ROWS'] = '0'
    try:
        model = pkg.get_deeplabv3p_model(mt, C, (H, W), 16, freeze_level=freeze_level, training=training)
        if training:
            model.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        ex = model._executor(N, training)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    run = ex.train_step if training else ex.forward
    if training:
        ex.set_inputs(x, y)
        ex.lr.fill_(0.01)
    else:
        ex.set_inputs(x)
    run()
    ex.capture()
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    return model, ex, run


def bench_models(pkg, lines, steps):
    N, H, W, C = 16, 512, 512, 21
    x, y = _inputs(N, H, W, C)
    lines.append('| workload | DL3P_GHOST | fused launches | launches | ms (min..max) | images/s | against 0 |')
    lines.append('|---|---|---|---|---|---|---|')
    cases = [('predict %s' % mt, mt, False, 0) for mt in ('ghostnet', 'ghostnet_lite')]
    cases += [('freeze_level=1 step %s' % mt, mt, True, 1) for mt in ('ghostnet', 'ghostnet_lite')]
    for label, mt, training, freeze in cases:
        arms = {g: _executor(pkg, mt, g, training, freeze, x, y, N, H, W, C) for g in ('1', '0')}
        arms['0 again'] = arms['0']
        times = {g: [] for g in arms}
        for _ in range(REPEATS):
            for g, (_, ex, run) in arms.items():
                times[g].append(window_us(run, steps) / 1e3)
        base = statistics.median(times['0'])
        for g, v in times.items():
            m, lo, hi = spread(v)
            ex = arms[g][1]
            n = ex.fwd.n_launches + (ex.bwd.n_launches + ex.opt.n_launches if training else 0)
            lines.append('| %s | %s | %d | %d | %.3f (%.3f..%.3f) | %.1f | %+.2f %% |' % (
                label, g, ex.ghost_launches(), n, m, lo, hi, N / m * 1e3, (m / base - 1) * 100))
        del arms
        torch.cuda.empty_cache()
    # (d) the plain train step: every BatchNorm trains, nothing is fused
    model, ex, run = _executor(pkg, 'ghostnet', '1', True, 0, x, y, N, H, W, C)
    v = [window_us(run, steps) / 1e3 for _ in range(REPEATS)]
    m, lo, hi = spread(v)
    lines.append('| train step ghostnet | 1 | %d | %d | %.3f (%.3f..%.3f) | %.1f | |' % (
        ex.ghost_launches(), ex.fwd.n_launches + ex.bwd.n_launches + ex.opt.n_launches, m, lo, hi, N / m * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modules-only', action='store_true')
    ap.add_argument('--models-only', action='store_true')
    ap.add_argument('--steps', type=int, default=10, help='forwards / train steps per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ghost.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    lines = []
    if not args.models_only:
        bench_modules(pkg, lines)
        lines.append('')
    if not args.modules_only:
        bench_models(pkg, lines, args.steps)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
