"""Gradient clipping (clipvalue / clipnorm / global_clipnorm, csrc/grad_clip.hip): what the passes cost on the MI355X.

  kernels   dl3p_grad_clip_sumsq, _finalize and _apply on the parameter store's own variable table of mobilenetv2 and of xception
            (513 x 513 models), and the optimiser launch they stand in front of (dl3p_sgd_momentum, called as the clipped plan
            calls it and as the unclipped plan does); device events around windows of launches, REPEATS windows each
  steps     the train step of MobileNetV2 batch 16 and of Xception batch 4 at 513 x 513 (resident batch, hipGraph replay) without
            clipping and with global_clipnorm, alternated in one process

    python scripts/bench_clip.py [--kernels-only | --steps-only] [--models mobilenetv2,xception] [--out FILE]
    python scripts/bench_clip.py --steps-only --unclipped-only --root OTHER_CHECKOUT

--root imports the package from another (built) checkout and --unclipped-only times the unclipped step alone: the parent commit's
step for the comparison DESIGN asks for (the unclipped plan is launch for launch the parent's), run in the same session.

Prints markdown tables ('Gradient clipping', keeps the last ones)."""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
REPEATS = 7
BATCH = {'mobilenetv2': 16, 'xception': 4}
H = W = 513
C = 21


def window_us(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def spread(v):
    return statistics.median(v), min(v), max(v)


def bench_kernels(torch, pkg, models, lines):
    ops = importlib.import_module(PKG + '.ops')
    ex = importlib.import_module(PKG + '.executor')
    L = ops.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines.append('| buffer | launch | us (min..max) | bytes / float | GB/s |')
    lines.append('|---|---|---|---|---|')
    for model_type in models:
        m = pkg.get_deeplabv3p_model(model_type, C, (H, W), 16, training=True)
        params = m.graph.all_params()
        offset, n = ex.param_offsets(params)
        cmap = ops.GradClipMap([(offset[p], (p.dev_size + 3) // 4 * 4) for p in params], 'cuda')
        f = dict(dtype=torch.float32, device='cuda')
        w, v = torch.randn(n, **f) * 0.1, torch.zeros(n, **f)
        g0 = torch.randn(n, **f) * 1e-3
        g = g0.clone()
        l2 = torch.full((n,), 2e-5, **f)
        lre = torch.zeros(n, **f)
        for p in params:                               # the padding between variables stays frozen, as in the parameter store
            lre[offset[p]:offset[p] + p.dev_size] = 1.0 if p.trainable else 0.0
        lr = torch.tensor([0.0], **f)                  # lr 0: the optimiser launches move no weight while they are timed
        p_ = lambda t: t.data_ptr()
        kw = dict(grad_scale=1.0, l2_elem=l2, lr_scale_elem=lre)
        ops.grad_clip_sumsq(g, w, cmap, **kw)
        ops.grad_clip_finalize(cmap, 2, 1e30)          # scale 1: apply leaves g as it is, window after window
        forms = [
            ('dl3p_grad_clip_sumsq', lambda: ops.grad_clip_sumsq(g, w, cmap, **kw), 16),
            ('dl3p_grad_clip_finalize', lambda: ops.grad_clip_finalize(cmap, 2, 1e30), 0),
            ('dl3p_grad_clip_apply', lambda: ops.grad_clip_apply(g, w, cmap, **kw), 20),
            ('dl3p_sgd_momentum behind the clip (grad_scale 1, no l2 table)',
             lambda: L.sgd_momentum(p_(w), p_(v), p_(g), n, p_(lr), 0.9, 0.0, 1.0, None, p_(lre), st), 24),
            ('dl3p_sgd_momentum of the unclipped plan',
             lambda: L.sgd_momentum(p_(w), p_(v), p_(g), n, p_(lr), 0.9, 0.0, 1.0, p_(l2), p_(lre), st), 28),
        ]
        reps = max(20, int(2e9 / (24 * n)))
        times = {name: [] for name, _, _ in forms}
        for _, fn, _ in forms:
            window_us(torch, fn, reps)
        for _ in range(REPEATS):
            for name, fn, _ in forms:
                times[name].append(window_us(torch, fn, reps))
        for name, _, nbytes in forms:
            md, lo, hi = spread(times[name])
            lines.append('| %s (%d floats, %d variables, %d blocks) | %s | %.1f (%.1f..%.1f) | %d | %s |' % (
                model_type, n, cmap.nvars, cmap.nblocks, name, md, lo, hi, nbytes, ('%.0f' % (nbytes * n / md / 1e3)) if nbytes else '-'))
        del w, v, g, g0, l2, lre, cmap


def bench_steps(torch, pkg, models, lines, steps, unclipped_only):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    lines.append('| model | batch | clipping | step ms (min..max) | images/s | against unclipped | optimiser-plan launches |')
    lines.append('|---|---|---|---|---|---|---|')
    for model_type in models:
        N = BATCH.get(model_type, 4)
        x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
        y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
        y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
        exs = {}
        for kind in ((None,) if unclipped_only else (None, 'global_clipnorm')):
            model = pkg.get_deeplabv3p_model(model_type, C, (H, W), 16, freeze_level=0, training=True)
            kw = {} if kind is None else {'global_clipnorm': 1.0}
            model.compile(optimizer=pkg.SGD(0.01, momentum=0.9, **kw), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
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
                times[kind].append(window_us(torch, ex.train_step, steps) / 1e3)
        base = statistics.median(times[None])
        for kind, v in times.items():
            md, lo, hi = spread(v)
            lines.append('| %s | %d | %s | %.3f (%.3f..%.3f) | %.1f | %+.2f %% | %d |' % (
                model_type, N, kind, md, lo, hi, N / md * 1e3, (md / base - 1) * 100, exs[kind][1].opt.n_launches))
        del exs, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--steps-only', action='store_true')
    ap.add_argument('--unclipped-only', action='store_true', help='time the step without clipping alone')
    ap.add_argument('--models', default='mobilenetv2,xception')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed window')
    ap.add_argument('--root', default=ROOT, help='the (built) checkout to import the package from')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_clip.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    models = [m for m in args.models.split(',') if m]
    lines = ['package from %s' % os.path.dirname(os.path.abspath(pkg.__file__)), '']
    if not args.steps_only:
        bench_kernels(torch, pkg, models, lines)
        lines.append('')
    if not args.kernels_only:
        bench_steps(torch, pkg, models, lines, args.steps, args.unclipped_only)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
