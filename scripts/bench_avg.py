"""Averaged optimisers (train.py --average_type): what the averaging costs on the MI355X.

  kernels   dl3p_{sgd_momentum,adam_step,rmsprop_step}_avg (update + ema in one pass) against the plain step followed by
            dl3p_weight_average (two launches, the weights read twice), at the ParamStore size of mobilenetv2 and of xception;
            device events around windows of launches, the two forms alternated in one process, REPEATS windows each
  steps     the MobileNetV2 513x513 batch-16 train step (bench.py's flagship, resident batch, hipGraph replay) with
            average_type None / ema / swa / lookahead in the same process; None is the path without averaging

    python scripts/bench_avg.py [--kernels-only | --steps-only] [--out FILE]

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


def store_total(pkg, model_type):
    """floats in the flat parameter buffer of a model type (no device needed)"""
    ex = importlib.import_module(PKG + '.executor')
    m = pkg.get_deeplabv3p_model(model_type, 21, (513, 513), 16, training=True)
    return ex.param_offsets(m.graph.all_params())[1]


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


def bench_kernels(pkg, lines):
    L = importlib.import_module(PKG + '._lib').lib()
    st = torch.cuda.current_stream().cuda_stream
    lines.append('| buffer | optimiser | fused us (min..max) | step + dl3p_weight_average us (min..max) | fused GB/s | two-launch GB/s |')
    lines.append('|---|---|---|---|---|---|')
    for model_type in ('mobilenetv2', 'xception'):
        n = store_total(pkg, model_type)
        f = dict(dtype=torch.float32, device='cuda')
        w, s1, s2, avg = (torch.randn(n, **f) * 0.1 for _ in range(4))
        s2.abs_()
        g = torch.randn(n, **f) * 1e-3
        l2 = torch.full((n,), 2e-5, **f)
        lre = torch.ones(n, **f)
        lr = torch.tensor([1e-3], **f)
        step = torch.ones(1, dtype=torch.int64, device='cuda')
        p = lambda t: t.data_ptr()
        a = (p(avg), 1, 0.99, 1, 0)
        forms = {
            'sgd': (lambda: L.sgd_momentum_avg(p(w), p(s1), p(g), n, p(lr), 0.9, 0.0, 1.0, p(l2), p(lre), *a, p(step), st),
                    lambda: L.sgd_momentum(p(w), p(s1), p(g), n, p(lr), 0.9, 0.0, 1.0, p(l2), p(lre), st), 36, 28 + 16),
            'adam': (lambda: L.adam_step_avg(p(w), p(s1), p(s2), p(g), n, p(lr), p(step), 0.9, 0.999, 1e-7, 1.0, p(l2), p(lre), *a, st),
                     lambda: L.adam_step(p(w), p(s1), p(s2), p(g), n, p(lr), p(step), 0.9, 0.999, 1e-7, 1.0, p(l2), p(lre), st),
                     44, 36 + 16),
            'rmsprop': (lambda: L.rmsprop_step_avg(p(w), p(s2), p(g), n, p(lr), 0.9, 1e-7, 1.0, p(l2), p(lre), *a, p(step), st),
                        lambda: L.rmsprop_step(p(w), p(s2), p(g), n, p(lr), 0.9, 1e-7, 1.0, p(l2), p(lre), st), 36, 28 + 16),
        }
        reps = max(20, int(2e9 / (40 * n)))           # ~2 GB of traffic per window
        for opt, (fused, plain, bytes_fused, bytes_two) in forms.items():
            def two():
                plain()
                L.weight_average(p(w), p(avg), n, 1, 0.99, 1, 0, p(step), p(lre), st)
            for fn in (fused, two):
                window_us(fn, reps)                     # warm-up
            tf, tt = [], []
            for _ in range(REPEATS):
                tf.append(window_us(fused, reps))
                tt.append(window_us(two, reps))
            (mf, lf, hf), (mt, lt, ht) = spread(tf), spread(tt)
            lines.append('| %s (%d floats) | %s + ema | %.1f (%.1f..%.1f) | %.1f (%.1f..%.1f) | %.0f | %.0f |' % (
                model_type, n, opt, mf, lf, hf, mt, lt, ht, bytes_fused * n / mf / 1e3, bytes_two * n / mt / 1e3))
        del w, s1, s2, avg, g, l2, lre


def bench_steps(pkg, lines, steps):
    N, H, W, C = 16, 513, 513, 21
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
    y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
    y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
    exs = {}
    for kind in (None, 'ema', 'swa', 'lookahead'):
        model = pkg.get_deeplabv3p_model('mobilenetv2', C, (H, W), 16, freeze_level=0, training=True)
        model.compile(optimizer=pkg.get_optimizer('sgd', 0.01, average_type=kind),
                      loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        ex = model._executor(N, True)
        ex.set_inputs(x, y)
        ex.lr.fill_(0.01)
        ex.train_step()
        ex.capture()
        for _ in range(5):
            ex.train_step()
        torch.cuda.synchronize()
        exs[kind] = (model, ex)
    times = {k: [] for k in exs}
    for _ in range(REPEATS):
        for kind, (_, ex) in exs.items():
            times[kind].append(window_us(ex.train_step, steps) / 1e3)
    base = statistics.median(times[None])
    lines.append('| average_type | step ms (min..max) | images/s | against None |')
    lines.append('|---|---|---|---|')
    for kind, v in times.items():
        m, lo, hi = spread(v)
        lines.append('| %s | %.3f (%.3f..%.3f) | %.1f | %+.2f %% |' % (kind, m, lo, hi, N / m * 1e3, (m / base - 1) * 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--steps-only', action='store_true')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_avg.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    lines = []
    if not args.steps_only:
        bench_kernels(pkg, lines)
        lines.append('')
    if not args.kernels_only:
        bench_steps(pkg, lines, args.steps)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
