"""Region losses (SparseDiceLoss and kin, csrc/region_loss.hip): what the three stages cost on the MI355X.

  steps     the MobileNetV2 513 x 513, batch 16 train step (resident batch, hipGraph replay) with plain cross entropy (the fused
            dl3p_head_train_rows head), with Keras sample weights (dl3p_upsample_softmax_loss + dl3p_resize_bilinear_bwd: the unfused
            head path the region loss runs on, the fair baseline) and with cross entropy + Dice, alternated in one process
  launches  dl3p_region_sums, dl3p_region_finalize and dl3p_region_head_grad on the buffers of that step, and for scale
            dl3p_pixel_loss_map and dl3p_upsample_softmax_loss on the same buffers; device events around windows of launches, REPEATS
            windows each

    python scripts/bench_region.py [--steps-only | --launches-only] [--out profiles/bench_region.txt]

Prints markdown tables (keeps the last ones)."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
REPEATS = 7
MODEL, N, H, W, C = 'mobilenetv2', 16, 513, 513, 21


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
    loss = pkg.SparseCategoricalCrossEntropy(ignore_index=255)
    if kind == 'ce + dice':
        loss = pkg.SparseDiceLoss(ignore_index=255, base=loss)
    model.compile(optimizer=pkg.SGD(0.01, momentum=0.9), loss=loss,
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


def batch(torch):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
    y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
    y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
    sw = torch.rand((N, H * W), device='cuda', generator=gen) * 3.8 + 0.2
    return x, y, sw


def bench_steps(torch, pkg, steps, lines):
    x, y, sw = batch(torch)
    exs = {kind: build(torch, pkg, kind, x, y, sw) for kind in ('plain', 'sample-weighted', 'ce + dice')}
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
    lr = exs['ce + dice'][1].last_region()
    lines.append('')
    lines.append('last_region of the ce + dice step: loss %.6f, %d classes present' % (lr['loss'], lr['present']))
    return exs


def bench_launches(torch, pkg, ex, lines):
    ops = importlib.import_module(PKG + '.ops')
    L = ops.lib()
    st = torch.cuda.current_stream().cuda_stream
    zt = ex.head.tensor
    P = N * H * W
    alpha, beta, smooth, rho, base_weight, _ = ex.region
    rows, rrows = ctypes.c_int(0), ctypes.c_int(0)
    ptr = lambda t: t.data_ptr()
    loss_map = torch.empty(P, dtype=torch.float32, device='cuda')
    scratch = ops.mining_workspace('cuda')          # (the map launch alone leaves a histogram behind: a workspace of its own)

    def sums():
        L.region_sums(ex.tptr(zt), zt.ld, ptr(ex.labels), 255, ptr(ex.region_ws), ctypes.byref(rrows), N, zt.H, zt.W, C, H, W, st)
    sums()
    forms = [
        ('dl3p_region_sums', sums),
        ('dl3p_region_finalize (%d rows)' % rrows.value,
         lambda: L.region_finalize(ptr(ex.region_ws), rrows.value, C, alpha, beta, smooth, rho, ptr(ex.region_record), st)),
        ('dl3p_region_head_grad, base ce (writes the (N,H,W,%d) gradient)' % ex.cpad,
         lambda: L.region_head_grad(ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 1.0 / P, 0, None, 0.0, 0.0, None, base_weight,
                                    ptr(ex.region_record), ptr(ex.dlogits_big), ex.cpad, ptr(ex.loss_partials), ctypes.byref(rows), N,
                                    zt.H, zt.W, C, H, W, st)),
        ('dl3p_region_head_grad, no base', lambda: L.region_head_grad(
            ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 1.0 / P, -1, None, 0.0, 0.0, None, 1.0, ptr(ex.region_record), ptr(ex.dlogits_big),
            ex.cpad, ptr(ex.loss_partials), ctypes.byref(rows), N, zt.H, zt.W, C, H, W, st)),
        ('dl3p_pixel_loss_map (for scale)', lambda: L.pixel_loss_map(
            ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 0, None, 0.0, 0.0, None, ptr(loss_map), ptr(scratch), N, zt.H, zt.W, C, H, W, st)),
        ('dl3p_upsample_softmax_loss (for scale; writes the same gradient)', lambda: L.upsample_softmax_loss(
            ex.tptr(zt), zt.ld, ptr(ex.labels), 255, 1.0 / P, 0, None, 0.0, 0.0, None, None, None, ptr(ex.dlogits_big), ex.cpad,
            ptr(ex.loss_partials), ctypes.byref(rows), N, zt.H, zt.W, C, H, W, st)),
    ]
    times = {name: [] for name, _ in forms}
    reps = 20
    for _, fn in forms:
        window_us(torch, fn, reps)
    for _ in range(REPEATS):
        for name, fn in forms:
            times[name].append(window_us(torch, fn, reps))
    lines.append('| launch (P = %d, %d x %d logits, C = %d) | us (min..max) |' % (P, zt.H, zt.W, C))
    lines.append('|---|---|')
    for name, _ in forms:
        md, lo, hi = spread(times[name])
        lines.append('| %s | %.1f (%.1f..%.1f) |' % (name, md, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps-only', action='store_true')
    ap.add_argument('--launches-only', action='store_true')
    ap.add_argument('--steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_region.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    lines = []
    exs = {}
    if not args.launches_only:
        exs = bench_steps(torch, pkg, args.steps, lines)
        lines.append('')
    if not args.steps_only:
        if 'ce + dice' not in exs:
            x, y, _ = batch(torch)
            exs['ce + dice'] = build(torch, pkg, 'ce + dice', x, y, None)
        bench_launches(torch, pkg, exs['ce + dice'][1], lines)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
