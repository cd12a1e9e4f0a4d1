"""Multi-scale / mirrored evaluation (dl3p_tta_accumulate, DeeplabModel.evaluate_miou(scales=..., flip=...)) on the MI355X.

  1. the head launch alone, N = 16, 513 x 513, 21 classes (sum rows of 24 floats), logits 129 x 129, between device events:
       paired   plain + mirrored pass added into the sum in place: one read and one write of the sum
       final    the same, sum not written, mask + confusion counters instead: one read of the sum
     against the bytes of the sum they move (N H W 24 floats per direction; the logits, 2 x 25 MB, stay in L2 / Infinity Cache and
     are not counted) at COPY_RATE, the one-read-one-write copy rate DESIGN.md section 5 uses as the yardstick of an HBM-bound pass.
     The sum (404 MB) is larger than the Infinity Cache, so every launch streams it from HBM.
  2. evaluate_miou in images / s, mobilenetv2 513 x 513 (output stride 16, float32), batch 16, the batch resident on the device:
       default    one scale, unmirrored (Executor.eval_step)
       fused      scales 0.5 .. 1.75 and the mirror image: twelve passes, six dl3p_tta_accumulate launches per batch
       composed   the same twelve forward passes, the head put together from the entry points that existed before
                  dl3p_tta_accumulate: ops.upsample_softmax_ce(want_probs=True) per pass (a full (N,H,W,C) probability tensor), a
                  mirror copy (torch.flip), a weighted add into a running sum (torch add_) and a final torch.argmax; no confusion
                  counting, which favours it
     host clock around whole calls, each ending in a device synchronise.
Every figure is the median (min..max) of WINDOWS windows.

    python scripts/bench_tta.py [--windows 5] [--out profiles/bench_tta.txt]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
COPY_RATE = 5.4e12          # B/s read + write, DESIGN.md section 5 (scripts/micro/fill_rate.py, 272 MB tensors)
N, HW, C, LOGITS = 16, 513, 21, 129
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def spread(v, fmt='%.3f'):
    return (fmt + ' (' + fmt + '..' + fmt + ')') % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10, help='head launches per window')
    ap.add_argument('--batches', type=int, default=2, help='batches per evaluate_miou call')
    ap.add_argument('--model', default='mobilenetv2')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_tta.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    ops = importlib.import_module(PKG + '.ops')
    aug = importlib.import_module(PKG + '.augment')
    sync = torch.cuda.synchronize
    lines = []

    # ---- 1. the head launch
    g = torch.Generator(device='cuda').manual_seed(0)
    z = torch.randn((N, LOGITS, LOGITS, 24), device='cuda', generator=g)
    zm = torch.randn((N, LOGITS, LOGITS, 24), device='cuda', generator=g)
    labels = torch.randint(0, C, (N * HW * HW,), device='cuda', generator=g).float()
    cm = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    acc, _, _ = ops.tta_accumulate(z, zm, C, HW, HW, 1.0 / 12)
    one_way = acc.numel() * 4

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        sync()
        return a.elapsed_time(b) * 1e-3 / args.calls

    def paired():
        ops.tta_accumulate(z, zm, C, HW, HW, 1.0 / 12, acc=acc)

    def final():
        ops.tta_accumulate(z, zm, C, HW, HW, 1.0 / 12, acc=acc, write=False, labels=labels, confusion=cm, want_mask=True)

    paired(), final()
    tp, tf = [], []
    for _ in range(args.windows):
        tp.append(events(paired))
        tf.append(events(final))
    lines += ['dl3p_tta_accumulate, N = %d, %d x %d, C = %d (rows of 24 floats), logits %d x %d; %d windows of %d launches; the sum is '
              '%.0f MB' % (N, HW, HW, C, LOGITS, LOGITS, args.windows, args.calls, one_way / 1e6), '',
              '| launch | bytes of the sum moved | ms, median (min..max) | achieved TB/s | time at %.1f TB/s / time |' % (COPY_RATE / 1e12),
              '|---|---|---|---|---|']
    for name, t, nbytes in (('paired (read + write)', tp, 2 * one_way), ('final (read, mask + counters)', tf, one_way)):
        med = statistics.median(t)
        lines.append('| %s | %.0f MB | %s | %.2f | %.2f |' % (name, nbytes / 1e6, spread([v * 1e3 for v in t]), nbytes / med / 1e12,
                                                            nbytes / COPY_RATE / med))
    del acc, z, zm, labels
    torch.cuda.empty_cache()

    # ---- 2. evaluate_miou
    model = pkg.get_deeplabv3p_model(args.model, C, (HW, HW), 16, training=False)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, (N, HW, HW, 3)).astype(np.uint8)).cuda()
    y = torch.from_numpy(rng.integers(0, C, (N, HW * HW, 1)).astype(np.uint8)).cuda()
    gen = [(x, y)] * args.batches
    T = 2 * len(SCALES)
    ones = torch.ones(N, dtype=torch.int32, device='cuda')
    L = importlib.import_module(PKG + '._lib').lib()

    def composed():
        for bx, _ in gen:
            acc = None
            for m in model._tta_siblings(SCALES):
                xs = bx if m is model else aug.pil_resize(bx, m.input_shape_hw)
                ex = m._executor(N, False)
                for mirrored in (False, True):
                    if mirrored:
                        xm = torch.empty_like(xs)
                        hs, ws = m.input_shape_hw
                        L.aug_flip_crop_u8(xs.data_ptr(), xm.data_ptr(), None, None, ones.data_ptr(), None, N, hs, ws, hs, ws,
                                           torch.cuda.current_stream().cuda_stream)
                    ex.set_inputs(xm if mirrored else xs)
                    p = ops.upsample_softmax_ce(ex.eval_logits(), C, HW, HW, want_probs=True)['probs']
                    if mirrored:
                        p = torch.flip(p, dims=[2])
                    acc = p.mul_(1.0 / T) if acc is None else acc.add_(p, alpha=1.0 / T)
            pred = torch.argmax(acc, dim=-1)
        return pred

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return args.batches * N / (time.perf_counter() - t0)

    configs = (('default (one scale, unmirrored)', lambda: model.evaluate_miou(gen)),
               ('fused: scales %s + mirror, dl3p_tta_accumulate' % (SCALES,), lambda: model.evaluate_miou(gen, scales=SCALES, flip=True)),
               ('composed: the same passes, upsample_softmax_ce(want_probs) + flip + add + argmax', composed))
    rates = {k: [] for k, _ in configs}
    for _, fn in configs:           # warm-up: siblings, executors of this batch size, code objects, allocator blocks
        fn()
    for _ in range(args.windows):
        for k, fn in configs:       # alternating, in one session
            rates[k].append(clock(fn))
    lines += ['', 'evaluate_miou, %s %d x %d, batch %d resident on the device, %d batches per call, %d windows; images / s, median '
              '(min..max)' % (args.model, HW, HW, N, args.batches, args.windows), '', '| configuration | images / s |', '|---|---|']
    lines += ['| %s | %s |' % (k, spread(rates[k], '%.1f')) for k, _ in configs]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
