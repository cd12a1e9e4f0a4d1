"""Dense-CRF post-processing (csrc/crf.hip, ops.dense_crf) on the MI355X, one 513 x 513 image.

  1. the kernels alone, between device events: the bilateral message (v_mfma_f32_32x32x2_f32 over all n^2 pixel pairs), the
     Gaussian message (row + column pass), the update.  The bilateral kernel's pair rate is set against one pair per cycle per SIMD,
     the rate of the fp32 MFMA with 32 label columns: SIMDS x CLOCK pairs / s.  DESIGN.md section 7 records the estimate made
     before anything was measured (6.9e10 pairs, roughly 30 ms per pass) next to these figures.
  2. ops.dense_crf, 5 iterations (6 bilateral passes: the normaliser and one per iteration), ms per image at C = 21 and C = 2, host
     clock around calls that end in a device synchronise, next to one forward pass of the model at that size (DeeplabModel.class_ids).
Every figure is the median (min..max) of WINDOWS windows.

    python scripts/bench_crf.py [--windows 5] [--out profiles/bench_crf.txt]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
SIMDS, CLOCK = 1024, 2.4e9          # 256 CUs x 4 SIMDs, peak engine clock
HW = 513
ESTIMATE_MS = 30.0                  # per bilateral pass, from the MFMA rate alone


def spread(v, fmt='%.3f'):
    return (fmt + ' (' + fmt + '..' + fmt + ')') % (statistics.median(v), min(v), max(v))


def scene(C, rng):
    """a block scene of all C classes with soft colours, noise and 35 % of the labels redrawn"""
    blocks = rng.permutation(64) % C
    truth = blocks.reshape(8, 8)[(np.arange(HW) * 8 // HW)[:, None], (np.arange(HW) * 8 // HW)[None, :]]
    colours = 128 + rng.integers(-40, 41, (C, 3))
    img = np.clip(np.rint(colours[truth] + rng.normal(0, 10, (HW, HW, 3))), 0, 255).astype(np.uint8)
    mask = truth.copy()
    redraw = rng.uniform(size=mask.shape) < 0.35
    mask[redraw] = rng.integers(0, C, int(redraw.sum()))
    return img, mask.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3, help='launches / calls per window')
    ap.add_argument('--model', default='mobilenetv2')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_crf.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    ops = importlib.import_module(PKG + '.ops')
    L = importlib.import_module(PKG + '._lib').lib()
    sync = torch.cuda.synchronize
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    n = HW * HW
    lines = []

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        sync()
        return a.elapsed_time(b) / args.calls

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    # ---- 1. the kernels
    img, mask = scene(21, rng)
    img_d, mask_d = torch.from_numpy(img)[None].cuda(), torch.from_numpy(mask)[None].cuda()
    _, q = ops.dense_crf(img_d, mask_d, 21, want_q=True)
    v = torch.zeros((1, n, ops.CRF_LP), device='cuda')
    v[..., :21] = q.view(1, n, 21)
    out, tmp = torch.empty_like(v), torch.empty_like(v)
    norm, census = torch.ones(n, device='cuda'), torch.zeros((1, 2), dtype=torch.int32, device='cuda')
    refined = torch.empty_like(mask_d)
    L.crf_unary(mask_d.data_ptr(), census.data_ptr(), out.data_ptr(), ops.CRF_LP, 0.7, 1, n, 21, st)
    kernels = (
        ('bilateral message (MFMA)', lambda: L.crf_bilateral_message(img_d.data_ptr(), v.data_ptr(), ops.CRF_LP, norm.data_ptr(),
                                                                     out.data_ptr(), ops.CRF_LP, None, 1, HW, HW, 80.0, 13.0, st)),
        ('Gaussian message (row + column pass)', lambda: L.crf_gauss_message(v.data_ptr(), ops.CRF_LP, norm.data_ptr(), tmp.data_ptr(),
                                                                             out.data_ptr(), ops.CRF_LP, 1, HW, HW, 3.0, 3.0, st)),
        ('update (softmax, argmax)', lambda: L.crf_update(mask_d.data_ptr(), census.data_ptr(), out.data_ptr(), norm.data_ptr(),
                                                          out.data_ptr(), norm.data_ptr(), 3.0, 10.0, 0.7, tmp.data_ptr(), ops.CRF_LP,
                                                          refined.data_ptr(), 1, n, 21, st)),
    )
    times = {k: [] for k, _ in kernels}
    for _, fn in kernels:
        fn()
    for _ in range(args.windows):
        for k, fn in kernels:
            times[k].append(events(fn))
    tb = statistics.median(times[kernels[0][0]]) * 1e-3
    lines += ['dense CRF kernels, one %d x %d image (n = %d pixels, n^2 = %.2e pairs), 32 label columns; %d windows of %d launches'
              % (HW, HW, n, float(n) * n, args.windows, args.calls), '', '| kernel | ms, median (min..max) |', '|---|---|']
    lines += ['| %s | %s |' % (k, spread(times[k])) for k, _ in kernels]
    lines += ['', 'bilateral pair rate: %.3e pairs / s = %.3f of %d SIMDs x %.1f GHz (one pair per cycle per SIMD); estimate before '
              'measuring: %.0f ms per pass, measured %.1f ms' % (float(n) * n / tb, float(n) * n / tb / (SIMDS * CLOCK), SIMDS, CLOCK / 1e9,
                                                                ESTIMATE_MS, tb * 1e3)]

    # ---- 2. the whole post-processing next to a forward pass
    model = pkg.get_deeplabv3p_model(args.model, 21, (HW, HW), 16, training=False)
    configs = [('forward pass, %s (class_ids)' % args.model, lambda: model.class_ids(img_d))]
    for C in (21, 2):
        im, mk = scene(C, rng)
        im_d, mk_d = torch.from_numpy(im)[None].cuda(), torch.from_numpy(mk)[None].cuda()
        configs.append(('dense_crf, C = %d, 5 iterations' % C, lambda im_d=im_d, mk_d=mk_d, C=C: ops.dense_crf(im_d, mk_d, C)))
    rates = {k: [] for k, _ in configs}
    for _, fn in configs:
        fn()
    for _ in range(args.windows):
        for k, fn in configs:
            rates[k].append(clock(fn))
    lines += ['', 'per image, %d x %d, batch 1, %d windows of %d calls; ms, median (min..max)' % (HW, HW, args.windows, args.calls), '',
              '| step | ms per image |', '|---|---|']
    lines += ['| %s | %s |' % (k, spread(rates[k])) for k, _ in configs]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
