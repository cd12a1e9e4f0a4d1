"""robustness sweep (GPU): every model type x odd / even input sizes x batch sizes x class counts through one eager
train step, one graph-replayed step and one predict; reports anything that raises or is not finite.
`--bf16`: the same under the mixed_bfloat16 policy (train.py:37-46 applies it to every model type); a type that refuses the
policy when it is built (ghostnet, ghostnet_lite: DESIGN 4k) is reported as refused, not as a failure"""
import importlib, os, sys, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module('tf-keras-deeplabv3p-model-set_amd')
rng = np.random.default_rng(0)
bad = 0
BF16 = '--bf16' in sys.argv
mp = pkg.mixed_precision
cases = []
for mt in sorted(pkg.deeplab_model_map):
    for (H, W), B, C, OS in [((64, 64), 1, 2, 16), ((97, 65), 3, 21, 16), ((128, 160), 2, 19, 8), ((33, 33), 5, 7, 16),
                             ((224, 224), 1, 32, 16)]:
        if OS == 8 and 'lite' in mt and False:
            continue
        cases.append((mt, H, W, B, C, OS))
for mt, H, W, B, C, OS in cases:
    tag = '%-22s %3dx%-3d B=%d C=%-2d OS=%-2d' % (mt, H, W, B, C, OS)
    try:
        if BF16:
            mp.set_policy(mp.Policy('mixed_bfloat16'))
        try:
            m = pkg.get_deeplabv3p_model(mt, C, (H, W), OS, training=True)
        except ValueError as e:
            if BF16 and 'mixed_bfloat16' in str(e):
                print(tag, 'refused under the policy:', str(e)[:120], flush=True)
                continue
            raise
        finally:
            mp.set_policy(mp.Policy('float32'))
        assert bool(m.bf16) == BF16
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
        x = rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)
        y = rng.integers(0, C, (B, H * W, 1)).astype(np.float32)
        y[rng.uniform(size=y.shape) < 0.05] = 255
        losses = [m.train_on_batch(x, y) for _ in range(3)]          # eager, then captured + replayed
        p = m.predict(x)
        ok = all(np.isfinite(l) for l in losses) and np.isfinite(p).all() and abs(p.sum(-1) - 1).max() < 1e-4
        cm = m.evaluate_miou([(x, y)], steps=1)
        ok = ok and np.isfinite(cm['mIoU'])
        print(tag, 'ok  ' if ok else 'BAD ', ['%.4f' % l for l in losses], flush=True)
        bad += 0 if ok else 1
        del m
        torch.cuda.empty_cache()
    except Exception as e:  # noqa: BLE001
        bad += 1
        print(tag, 'RAISED', type(e).__name__, str(e)[:200], flush=True)
print('failures:', bad)
