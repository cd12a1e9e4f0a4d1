"""Hard-example mining (top_k_percent_pixels, csrc/mining.hip): what the three stages cost on the MI355X.

  steps     the MobileNetV2 513 x 513, batch 16 train step (resident batch, hipGraph replay) with mining off (the fused
            dl3p_head_train_rows head), with Keras sample weights and no mining (dl3p_upsample_softmax_loss + dl3p_resize_bilinear_bwd:
            the head path mining runs on) and with top_k_percent_pixels = 0.25, alternated in one process
  launches  dl3p_pixel_loss_map, dl3p_topk_threshold (7 launches with the first histogram taken from the map launch) and
            dl3p_mining_weights on the buffers of that step, and the weighted head launch behind them; device events around windows of
            launches, REPEATS windows each

    python scripts/bench_mining.py [--steps-only | --launches-only] [--out profiles/bench_mining.txt]
    python scripts/bench_mining.py --steps-only --baseline-only --root OTHER_CHECKOUT

--root imports the package from another (built) checkout and --baseline-only leaves the mined step out: the parent commit's plain
and sample-weighted steps, run in the same session.

Prints markdown tables (keeps the last ones)."""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
REPEATS = 7
MODEL, N, H, W, C = 'mobilenetv2', 16, 513, 513, 21
P_MINE = 0.25


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


def build(torch, pkg, kind, x, y, sw):
    model = pkg.get_deeplabv3p_model(MODEL, C, (H, W), 16, freeze_level=0, training=True)
    kw = dict(top_k_percent_pixels=P_MINE) if kind == 'mined' else {}
    model.compile(optimizer=pkg.SGD(0.01, momentum=0.9), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255, **kw),
                  sample_weight_mode='temporal' if kind == 'sample-weighted' else None)
    ex = model._executor(N, True)
    ex.set_inputs(x, y, sw if kind == 'sample-weighted' else None)
    ex.lr.fill_(0.01)
    ex.train_step()
    ex.capture()
    for _ in range(5):
        ex.train_step()
    torch.cuda.synchronize()
    return model, ex


def bench_steps(torch, pkg, kinds, steps, lines):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
    y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
    y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
    sw = torch.rand((N, H * W), device='cuda', generator=gen) * 3.8 + 0.2
    exs = {kind: build(torch, pkg, kind, x, y, sw) for kind in kinds}
    times = {k: [] for k in exs}
    for _ in range(REPEATS):
        for kind, (_, ex) in exs.items():
            times[kind].append(window_us(torch, ex.train_step, steps) / 1e3)
    lines.append('| %s %d x %d, batch %d | head launches of the forward plan | step ms (min..max) | images/s | against plain | against '
                 'sample-weighted |' % (MODEL, H, W, N))
    lines.append('|---|---|---|---|---|---|')
    plain = statistics.median(times['plain'])
    weighted = statistics.median(times['sample-weighted'])
    for kind, v in times.items():
        md, lo, hi = spread(v)
        ex = exs[kind][1]
        i0 = [i for i, (_, ctx) in enumerate(ex.fwd.labels) if ctx == 'head'][0]
        head = ', '.join(name.replace('dl3p_', '') for name, _ in ex.fwd.labels[i0:])
        lines.append('| %s | %s | %.3f (%.3f..%.3f) | %.1f | %+.2f %% | %+.2f %% |' % (
            kind, head, md, lo, hi, N / md * 1e3, (md / plain - 1) * 100, (md / weighted - 1) * 100))
    return exs


def bench_launches(torch, pkg, ex, lines):
    ops = importlib.import_module(PKG + '.ops')
    L = ops.lib()
    st = torch.cuda.current_stream().cuda_stream
    zt = ex.head.tensor
    P = N * H * W
    p, M = ex.mining
    import ctypes
    rows = ctypes.c_int(0)
    ptr = lambda t: t.data_ptr()

    def select():
        # (a select needs the first histogram of a map launch: the map launch in front of it is timed with it and subtracted below)
        L.pixel_loss_map(ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 0, None, 0.0, 0.0, None, ptr(ex.loss_map), ptr(ex.mining_ws), N,
                         zt.H, zt.W, C, H, W, st)
        L.topk_threshold(ptr(ex.loss_map), P, p, M, ptr(ex.store.opt_step), -1, 1, ptr(ex.mining_ws), ptr(ex.mining_record), st)
    forms = [
        ('dl3p_pixel_loss_map + dl3p_topk_threshold (1 + 7 launches)', select),
        ('dl3p_topk_threshold counting the first pass itself (8 launches)',
         lambda: L.topk_threshold(ptr(ex.loss_map), P, p, M, ptr(ex.store.opt_step), -1, 0, ptr(ex.mining_ws), ptr(ex.mining_record), st)),
        ('dl3p_mining_weights',
         lambda: L.mining_weights(ptr(ex.loss_map), None, ptr(ex.mining_record), ptr(ex.mining_weights), P, st)),
        ('dl3p_upsample_softmax_loss behind them (writes the (N,H,W,%d) gradient)' % ex.cpad,
         lambda: L.upsample_softmax_loss(ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 1.0 / P, 0, None, 0.0, 0.0, ptr(ex.mining_weights), None,
                                         None, ptr(ex.dlogits_big), ex.cpad, ptr(ex.loss_partials), ctypes.byref(rows), N, zt.H, zt.W,
                                         C, H, W, st)),
    ]
    select()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    # the map launch alone leaves a histogram behind that only a select clears: time it last, through a workspace of its own
    scratch = ops.mining_workspace('cuda')

    def map_only():
        L.pixel_loss_map(ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 0, None, 0.0, 0.0, None, ptr(ex.loss_map), ptr(scratch), N, zt.H, zt.W,
                         C, H, W, st)
    forms.insert(0, ('dl3p_pixel_loss_map', map_only))
    times['dl3p_pixel_loss_map'] = []
    reps = 20
    for _, fn in forms:
        window_us(torch, fn, reps)
    for _ in range(REPEATS):
        for name, fn in forms:
            times[name].append(window_us(torch, fn, reps))
    lines.append('| launch (P = %d, %d x %d logits, C = %d, k = %d) | us (min..max) |' % (P, zt.H, zt.W, C, int(p * P)))
    lines.append('|---|---|')
    for name, _ in forms:
        md, lo, hi = spread(times[name])
        lines.append('| %s | %.1f (%.1f..%.1f) |' % (name, md, lo, hi))
    m0 = statistics.median(times['dl3p_pixel_loss_map'])
    m1 = statistics.median(times[forms[1][0]])
    lines.append('| dl3p_topk_threshold behind the map launch (7 launches; the difference of the medians above) | %.1f |' % (m1 - m0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps-only', action='store_true')
    ap.add_argument('--launches-only', action='store_true')
    ap.add_argument('--baseline-only', action='store_true', help='leave the mined step out (a checkout without mining)')
    ap.add_argument('--steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--root', default=ROOT, help='the (built) checkout to import the package from')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mining.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    lines = ['package from %s' % os.path.dirname(os.path.abspath(pkg.__file__)), '']
    kinds = ['plain', 'sample-weighted'] + ([] if args.baseline_only else ['mined'])
    exs = {}
    if not args.launches_only:
        exs = bench_steps(torch, pkg, kinds, args.steps, lines)
        lines.append('')
    if not args.steps_only and not args.baseline_only:
        if 'mined' not in exs:
            gen = torch.Generator(device='cuda')
            gen.manual_seed(1234)
            x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
            y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
            exs['mined'] = build(torch, pkg, 'mined', x, y, None)
        bench_launches(torch, pkg, exs['mined'][1], lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.baseline_only else 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
