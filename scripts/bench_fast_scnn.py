"""The Fast-SCNN family and its nearest-upsampling kernels (csrc/nearest.hip, csrc/nearest_head.hip) on the MI355X.

  (a) kernels  the four new kernel groups at the shapes of the model at 8 x 512 x 512 and 1 x 2048 x 1024 (the reference's default
               input, fast_scnn.py:87): fused upsample-add with BatchNorm statistics (r = 4, 128 channels), block sum, window
               average pooling forward / backward (the bin-2 window of the pyramid pooling block), nearest head (training kernel
               and probabilities, 21 classes in 24-float rows).  Device events around windows of calls of the ops.py wrappers,
               REPEATS windows each: a CALL time -- for kernels of a few microseconds it is the host's enqueue rate (the head-train
               wrapper also fills its partial rows and launches the loss reduction).  Kernel times come from a kernel trace of
               this file, one run per size (rocprofv3 --kernel-trace --stats -- python scripts/bench_fast_scnn.py --kernels-only
               --size i).  Bytes are what the algorithm has to move (every operand once), computed from the shapes here; the
               share is bytes / time over the 8 TB/s HBM peak.
  (b) step     images/s and launch count of one train step (SGD, sparse cross-entropy) at the same two sizes, hipGraph replay.

  (c) trace    --ingest-trace STATS0.csv STATS1.csv: no device needed.  Reads the *_kernel_stats.csv files of the two kernel-trace runs
               (one per entry of SIZES, in that order), keeps this file's kernels and writes their average durations with the same
               algorithmic bytes as (a) -> profiles/bench_fast_scnn_kernel_trace.json, the kernel times DESIGN 4n quotes.

    python scripts/bench_fast_scnn.py [--kernels-only | --models-only] [--size 0|1] [--out profiles/bench_fast_scnn.json]
    python scripts/bench_fast_scnn.py --ingest-trace size0_kernel_stats.csv size1_kernel_stats.csv --out profiles/bench_fast_scnn_kernel_trace.json

Prints markdown tables and writes the numbers as JSON."""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PKG = 'tf-keras-deeplabv3p-model-set_amd'
REPEATS = 7
PEAK_HBM = 8.0e12
SIZES = [(8, 512, 512), (1, 2048, 1024)]
C, CP = 21, 24


# kernel name in a trace -> the entry point that launches it
TRACE_KERNELS = {'upsample_add_kernel': 'upsample_add_fwd', 'block_sum_kernel': 'block_sum_bwd', 'winpool_fwd_small_kernel': 'winpool2d_fwd',
                 'winpool_fwd_block_kernel': 'winpool2d_fwd', 'winpool_bwd_kernel': 'winpool2d_bwd',
                 'nearest_head_train_kernel': 'nearest_head_train', 'nearest_probs_kernel': 'nearest_softmax_probs'}


def algorithmic_bytes(N, H, W):
    """entry point -> the bytes it has to move at the model's shapes for an (N, H, W) input: every operand once"""
    M, m = N * (H // 8) * (W // 8), N * (H // 32) * (W // 32)
    return {'upsample_add_fwd': 4.0 * 128 * (2 * M + m), 'block_sum_bwd': 4.0 * 128 * (M + m), 'winpool2d_fwd': 4.0 * 128 * (m + N * 4),
            'winpool2d_bwd': 4.0 * 128 * (m + N * 4), 'nearest_head_train': 4.0 * (N * H * W + 2 * M * CP),
            'nearest_softmax_probs': 4.0 * (N * H * W * C + M * CP)}


def ingest_trace(paths, lines, out):
    assert len(paths) == len(SIZES), 'one kernel-stats file per entry of SIZES'
    lines.append('| shape | kernel | kernel time, us (trace average) | calls | bytes | TB/s | of 8 TB/s |')
    lines.append('|---|---|---|---|---|---|---|')
    for (N, H, W), path in zip(SIZES, paths):
        byts = algorithmic_bytes(N, H, W)
        with open(path, newline='') as fh:
            rows = [r for r in csv.DictReader(l for l in fh if l.startswith('"'))]
        for r in rows:
            kn = [k for k in TRACE_KERNELS if '::%s(' % k in r['Name'] or r['Name'].startswith(k)]
            if not kn:
                continue
            b, us = byts[TRACE_KERNELS[kn[0]]], float(r['AverageNs']) / 1e3
            out['kernel_trace'].append(dict(shape='%d x %d x %d' % (N, H, W), kernel=kn[0], entry_point='dl3p_' + TRACE_KERNELS[kn[0]],
                                            calls=int(r['Calls']), avg_us=round(us, 2), min_us=int(r['MinNs']) / 1e3,
                                            max_us=int(r['MaxNs']) / 1e3, bytes=int(b), tb_per_s=round(b / us / 1e6, 3),
                                            share_of_hbm_peak=round(b / us / 1e6 / (PEAK_HBM / 1e12), 3)))
            lines.append('| %d x %d x %d | %s | %.1f | %d | %d | %.2f | %.1f %% |' % (
                N, H, W, kn[0], us, int(r['Calls']), b, b / us / 1e6, 100 * b / us / 1e6 / (PEAK_HBM / 1e12)))


def window_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def timed(fn, byts):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    one = max(window_us(fn, 5), 1.0)
    reps = max(10, int(0.2e6 / one))                       # ~0.2 s windows
    v = [window_us(fn, reps) for _ in range(REPEATS)]
    m = statistics.median(v)
    return dict(us=round(m, 2), us_min=round(min(v), 2), us_max=round(max(v), 2), bytes=int(byts),
                tb_per_s=round(byts / (m * 1e-6) / 1e12, 3), share_of_hbm_peak=round(byts / (m * 1e-6) / PEAK_HBM, 3))


def bench_kernels(lines, out, sizes):
    ops = importlib.import_module(PKG + '.ops')
    f = dict(dtype=torch.float32, device='cuda')
    lines.append('| shape | kernel | us (min..max) | bytes | TB/s | of 8 TB/s |')
    lines.append('|---|---|---|---|---|---|')
    for N, H, W in sizes:
        h8, w8, h32, w32 = H // 8, W // 8, H // 32, W // 32
        a = torch.randn((N, h8, w8, 128), **f)
        b = torch.randn((N, h32, w32, 128), **f)
        o = torch.empty_like(a)
        gl = torch.empty_like(b)
        sc, sh = torch.rand(128, **f) + 0.5, torch.randn(128, **f)
        part = ops.new_partials(128, 'cuda')
        kh, kw = h32 // 2, w32 // 2
        py = torch.empty((N, 2, 2, 128), **f)
        z = torch.randn((N, h8, w8, CP), **f)
        z[..., C:] = 0
        lab = torch.randint(0, C, (N, H * W, 1), device='cuda').float()
        gz = torch.zeros_like(z)
        B = algorithmic_bytes(N, H, W)
        arms = [
            ('upsample_add_fwd r=4 C=128 + statistics', B['upsample_add_fwd'],
             lambda: ops.upsample_add_fwd(a, b, 4, sc, sh, 0, None, None, 0, out=o, partials=part)),
            ('block_sum_bwd r=4 C=128', B['block_sum_bwd'], lambda: ops.block_sum_bwd(a, 4, out=gl)),
            ('winpool2d_fwd %dx%d C=128' % (kh, kw), B['winpool2d_fwd'], lambda: ops.winpool2d_fwd(b, kh, kw, out=py)),
            ('winpool2d_bwd %dx%d C=128' % (kh, kw), B['winpool2d_bwd'],
             lambda: ops.winpool2d_bwd(py, (N, h32, w32, 128), kh, kw, out=gl)),
            ('nearest_head_train r=8 C=21', B['nearest_head_train'], lambda: ops.nearest_head_train(z, C, H, W, lab, 255, out=gz)),
            ('nearest_softmax_probs r=8 C=21', B['nearest_softmax_probs'], lambda: ops.nearest_softmax_probs(z, C, H, W)),
        ]
        for name, byts, fn in arms:
            r = timed(fn, byts)
            out['kernels'].append(dict(shape='%d x %d x %d' % (N, H, W), kernel=name, **r))
            lines.append('| %d x %d x %d | %s | %.1f (%.1f..%.1f) | %d | %.2f | %.1f %% |' % (
                N, H, W, name, r['us'], r['us_min'], r['us_max'], r['bytes'], r['tb_per_s'], 100 * r['share_of_hbm_peak']))
        del a, b, o, gl, z, lab, gz
        torch.cuda.empty_cache()


def bench_models(lines, out, steps, sizes):
    pkg = importlib.import_module(PKG)
    lines.append('| workload | launches | ms (min..max) | images/s |')
    lines.append('|---|---|---|---|')
    for N, H, W in sizes:
        gen = torch.Generator(device='cuda')
        gen.manual_seed(1234)
        x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
        y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
        y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
        model = pkg.get_fast_scnn_model('fast_scnn', C, (H, W))
        model.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        ex = model._executor(N, True)
        ex.set_inputs(x, y)
        ex.lr.fill_(0.01)
        ex.train_step()
        ex.capture()
        for _ in range(3):
            ex.train_step()
        torch.cuda.synchronize()
        v = [window_us(ex.train_step, steps) / 1e3 for _ in range(REPEATS)]
        ms = statistics.median(v)
        n = ex.fwd.n_launches + ex.bwd.n_launches + ex.opt.n_launches
        out['train_step'].append(dict(shape='%d x %d x %d' % (N, H, W), launches=n, ms=round(ms, 3), ms_min=round(min(v), 3),
                                      ms_max=round(max(v), 3), images_per_s=round(N / ms * 1e3, 1)))
        lines.append('| fast_scnn train step, %d x %d x %d, hipGraph replay | %d | %.2f (%.2f..%.2f) | %.1f |' % (
            N, H, W, n, ms, min(v), max(v), N / ms * 1e3))
        del model, ex
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--models-only', action='store_true')
    ap.add_argument('--steps', type=int, default=20, help='train steps per timed window')
    ap.add_argument('--size', type=int, default=None, help='index into SIZES: that size only (a kernel-trace run per size)')
    ap.add_argument('--ingest-trace', nargs='+', default=None, metavar='STATS.csv',
                    help='kernel-stats files of the kernel-trace runs, one per size: write their figures, run nothing')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.ingest_trace:
        lines, out = [], dict(source='rocprofv3 --kernel-trace --stats -- python scripts/bench_fast_scnn.py --kernels-only --size i',
                              kernel_trace=[])
        ingest_trace(args.ingest_trace, lines, out)
        print('\n'.join(lines))
        if args.out:
            with open(args.out, 'w') as fh:
                json.dump(out, fh, indent=1)
                fh.write('\n')
        return
    if not torch.cuda.is_available():
        raise SystemExit('bench_fast_scnn.py measures on the MI355X; no device found')
    sizes = SIZES if args.size is None else [SIZES[args.size]]
    lines, out = [], dict(device=torch.cuda.get_device_name(0), repeats=REPEATS, kernels=[], train_step=[])
    if not args.models_only:
        bench_kernels(lines, out, sizes)
        lines.append('')
    if not args.kernels_only:
        bench_models(lines, out, args.steps, sizes)
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
