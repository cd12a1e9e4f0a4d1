"""The 2x2 stride-2 transposed conv (csrc/deconv.hip) and the U-Net family on the MI355X.

  (a) layers   the four up-path layers of a U-Net at 8 x 512 x 512 (M x Cin -> Cout: 8*32^2 x 1024 -> 512 ... 8*256^2 x 128 -> 64) in
               their three roles, against kernels this file's subject does not touch:
                 forward        dl3p_conv2d_gemm_bwd_data at k = 2, stride 2 (the same operator as a masked data gradient; no bias,
                                no prologue), and dl3p_pwconv_fwd_wt into an [M][4 Cout] scratch + a torch permute-copy
                 data gradient  dl3p_conv2d_gemm_fwd at k = 2, stride 2
                 weight grad.   dl3p_conv2d_gemm_bwd_weight at k = 2, stride 2 with the roles of x and dy swapped
               Device events around windows of launches, arms alternated in one process, REPEATS windows each; the first
               comparator is also timed against ITSELF (two series of windows) to show the spread.  The achieved fraction of the
               fp32 matrix peak counts 2 M Cin 4 Cout flops.
  (b) step     images/s and launch count of one train step and of predict for unet_standard and unet_lite at 8 x 512 x 512,
               hipGraph replay.

    python scripts/bench_unet.py [--layers-only | --models-only] [--out FILE]

Prints markdown tables (docs/experiments.md keeps the last ones)."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PKG = 'tf-keras-deeplabv3p-model-set_amd'
REPEATS = 7
PEAK_F32_MATRIX = 157.3e12        # MI355X: 256 CUs x 4 SIMDs x 64 flop/clk (v_mfma_f32_16x16x4_f32) x 2.4 GHz
LAYERS = [(32, 1024, 512), (64, 512, 256), (128, 256, 128), (256, 128, 64)]      # (map size, Cin, Cout) of up6 .. up9


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


def fmt(v):
    return '%.1f (%.1f..%.1f)' % spread(v)


def bench_layers(lines, N=8):
    ops = importlib.import_module(PKG + '.ops')
    L = importlib.import_module(PKG + '._lib').lib()
    f = dict(dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    lines.append('| layer | role | new us (min..max) | comparator | comparator us (min..max) | again us | its spread | new / comparator | '
                 'of fp32 matrix peak | bound |')
    lines.append('|---|---|---|---|---|---|---|---|---|---|')
    for S, Cin, Cout in LAYERS:
        M = N * S * S
        x = torch.randn((N, S, S, Cin), **f)
        dy = torch.randn((N, 2 * S, 2 * S, Cout), **f)
        w = torch.randn((2, 2, Cout, Cin), **f) / Cin ** 0.5          # the Keras kernel; as HWIO it is the k = 2 conv dy -> x
        bias = torch.randn(Cout, **f)
        y = torch.empty((N, 2 * S, 2 * S, Cout), **f)
        gx = torch.empty((N, S, S, Cin), **f)
        flat = torch.empty((M, 4 * Cout), **f)
        wd = torch.empty(4 * Cout * Cin, **f)                         # the comparator's re-laid kernels, made once
        L.conv2d_gemm_dgrad_weights(w.data_ptr(), wd.data_ptr(), 2, Cout, Cin, st)
        wt = w.reshape(4 * Cout, Cin).t().contiguous()                # [Cin][4 Cout] = the conv's [k k Cin'][Cout'] transposed: (Cin, 4 Cout)
        wflat = w.reshape(4 * Cout, Cin).contiguous()                 # [N = 4 Cout][K = Cin]: what dl3p_pwconv_fwd_wt takes
        wsb = max(L.conv2d_gemm_bwd_weight_workspace(N, S, S, Cout, Cin, 2), L.deconv2x2_bwd_weight_workspace(N, S, S, Cin, Cout))
        ws = torch.empty(wsb // 4 + 4, **f)
        gw, gb = torch.empty((2, 2, Cout, Cin), **f), torch.empty(Cout, **f)
        rows = ctypes.c_int(0)
        xp, dp, yp, gp = x.data_ptr(), dy.data_ptr(), y.data_ptr(), gx.data_ptr()

        arms = {
            'forward': (lambda: L.deconv2x2_fwd(xp, Cin, None, None, 0, w.data_ptr(), bias.data_ptr(), yp, Cout, N, S, S, Cin, Cout, st), [
                ('conv2d_gemm_bwd_data k2 s2', lambda: L.conv2d_gemm_bwd_data(xp, Cin, wd.data_ptr(), yp, Cout, 0, N, 2 * S, 2 * S, Cout, Cin,
                                                                            2, 2, 1, 0, 0, S, S, st)),
                ('pwconv_fwd_wt + permute-copy', lambda: (L.pwconv_fwd_wt(xp, Cin, None, None, 0, wflat.data_ptr(), None, flat.data_ptr(), 4 * Cout,
                                                                         None, ctypes.byref(rows), M, Cin, 4 * Cout, st),
                                                          y.view(N, S, 2, S, 2, Cout).copy_(flat.view(N, S, S, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5))))]),
            'data gradient': (lambda: L.deconv2x2_bwd_data(dp, Cout, w.data_ptr(), gp, Cin, 0, N, S, S, Cin, Cout, st), [
                ('conv2d_gemm_fwd k2 s2', lambda: L.conv2d_gemm_fwd(dp, Cout, None, None, 0, wt.data_ptr(), None, gp, Cin, None, ctypes.byref(rows),
                                                                   N, 2 * S, 2 * S, Cout, Cin, 2, 2, 1, 0, 0, S, S, st))]),
            'weight gradient': (lambda: L.deconv2x2_bwd_weight(xp, Cin, None, None, 0, dp, Cout, gw.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                                               wsb, N, S, S, Cin, Cout, st), [
                ('conv2d_gemm_bwd_weight k2 s2', lambda: L.conv2d_gemm_bwd_weight(dp, Cout, None, None, 0, xp, Cin, gw.data_ptr(), None,
                                                                                 ws.data_ptr(), wsb, N, 2 * S, 2 * S, Cout, Cin, 2, 2, 1, 0, 0,
                                                                                 S, S, st))]),
        }
        flops = 2.0 * M * Cin * 4 * Cout
        byts = 4.0 * (M * Cin + 4 * M * Cout + 4 * Cin * Cout)
        for role, (new, comps) in arms.items():
            reps = max(5, int(0.03 / (flops / 40e12)))                  # ~30 ms windows at 40 Tflop/s
            for fn in [new] + [c for _, c in comps]:
                window_us(fn, 2)
            tn, tc, tq = [], {n: [] for n, _ in comps}, []
            for _ in range(REPEATS):
                tn.append(window_us(new, reps))
                for n, c in comps:
                    tc[n].append(window_us(c, reps))
                tq.append(window_us(comps[0][1], reps))
            mn = statistics.median(tn)
            frac = flops / (mn * 1e-6) / PEAK_F32_MATRIX
            bw = byts / (mn * 1e-6) / 1e12
            bound = 'matrix issue' if frac > 0.25 else ('HBM (%.1f TB/s)' % bw if bw > 2.0 else 'neither: latency / occupancy')
            for i, (n, _) in enumerate(comps):
                mc, lc, hc = spread(tc[n])
                mq = statistics.median(tq) if i == 0 else float('nan')
                sp = max(abs(mc - mq), hc - lc) / mc if i == 0 else (hc - lc) / mc
                lines.append('| %d x %d -> %d | %s | %s | %s | %s | %s | %.1f %% | %.3f | %.1f %% | %s |' % (
                    M, Cin, Cout, role, fmt(tn), n, fmt(tc[n]), '%.1f' % mq if i == 0 else '', sp * 100, mn / mc, frac * 100, bound))
        del x, dy, y, gx, flat, ws
        torch.cuda.empty_cache()


def _inputs(N, H, W, C):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    x = torch.rand((N, H, W, 3), device='cuda', generator=gen) * 2 - 1
    y = torch.randint(0, C, (N, H * W, 1), device='cuda', generator=gen).float()
    y[torch.rand(y.shape, device='cuda', generator=gen) < 0.05] = 255.0
    return x, y


def bench_models(pkg, lines, steps):
    N, H, W, C = 8, 512, 512, 21
    x, y = _inputs(N, H, W, C)
    lines.append('| workload | launches | ms (min..max) | images/s | parent commit |')
    lines.append('|---|---|---|---|---|')
    for mt in ('unet_standard', 'unet_lite'):
        for training in (True, False):
            model = pkg.get_unet_model(mt, C, (H, W), training=training)
            if training:
                model.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
            ex = model._executor(N, training)
            run = ex.train_step if training else ex.forward
            if training:
                ex.set_inputs(x, y)
                ex.lr.fill_(0.01)
            else:
                ex.set_inputs(x)
            run()
            ex.capture()
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            v = [window_us(run, steps) / 1e3 for _ in range(REPEATS)]
            m, lo, hi = spread(v)
            n = ex.fwd.n_launches + (ex.bwd.n_launches + ex.opt.n_launches if training else 0)
            lines.append('| %s %s, 8 x 512 x 512, hipGraph replay | %d | %.2f (%.2f..%.2f) | %.1f | n/a (model type absent) |' % (
                mt, 'train step' if training else 'predict', n, m, lo, hi, N / m * 1e3))
            del model, ex, run
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers-only', action='store_true')
    ap.add_argument('--models-only', action='store_true')
    ap.add_argument('--steps', type=int, default=3, help='forwards / train steps per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_unet.py measures on the MI355X; no device found')
    pkg = importlib.import_module(PKG)
    lines = []
    if not args.models_only:
        bench_layers(lines)
        lines.append('')
    if not args.layers_only:
        bench_models(pkg, lines, args.steps)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
