"""SegmentationGenerator (data.py): what one batch costs on the MI355X and where the time goes.

16 synthetic 375 x 500 JPEGs with palette-PNG labels are written to a temporary directory; batches of 16 go to 512 x 512.
  batch   ms per __getitem__ (host clock, ending in a device synchronise) with augment=True and augment=False
  split   the same batch in its parts: PIL decode (host clock), upload (host clock to a synchronise), and the device chain -- the
          twelve augmentations plus the resize, N = 1 launches per image -- between two device events
  chain   that chain enqueued back to back (16 images, no synchronise between them) against idle-queued (a synchronise before
          every image, so every launch meets an idle queue): what the small launches cost when nothing hides their latency
Every figure is the median (min..max) of WINDOWS windows; the random draws of a window are seeded, so all windows do the same work.

    python scripts/bench_generator.py [--windows 7] [--calls 3] [--out FILE]

Prints a markdown table (DESIGN.md section 7 keeps the last one)."""
import argparse
import importlib
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'tf-keras-deeplabv3p-model-set_amd'
BATCH, SRC, DST = 16, (375, 500), (512, 512)


def write_dataset(root):
    from PIL import Image
    os.makedirs(os.path.join(root, 'images'))
    os.makedirs(os.path.join(root, 'labels'))
    rng = np.random.default_rng(0)
    h, w = SRC
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(BATCH):
        base = np.stack([(yy * (k + 3)) % 256, (xx * 255) // w, ((yy + xx) * 255) // (h + w)], -1)
        img = np.clip(base + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, 'images', '%02d.jpg' % k), quality=90)
        lab = rng.integers(0, 21, (h // 25 + 1, w // 25 + 1)).astype(np.uint8).repeat(25, 0).repeat(25, 1)[:h, :w]
        lab[rng.uniform(size=lab.shape) < 0.03] = 255
        p = Image.fromarray(np.ascontiguousarray(lab), mode='P')
        p.putpalette([v for c in range(256) for v in (c, 255 - c, (7 * c) % 256)])
        p.save(os.path.join(root, 'labels', '%02d.png' % k))
    return ['%02d' % k for k in range(BATCH)]


def seed(k):
    np.random.seed(k)
    random.seed(k)


def spread(v):
    return '%.2f (%.2f..%.2f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3, help='__getitem__ calls per window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_generator.py measures on the MI355X; no device found')
    D = importlib.import_module(PKG + '.data')
    A = importlib.import_module(PKG + '.augment')
    sync = torch.cuda.synchronize
    with tempfile.TemporaryDirectory() as root:
        ids = write_dataset(root)
        gen = D.SegmentationGenerator(root, ids, batch_size=BATCH, input_shape=DST)
        paths = list(zip(gen.image_path_list, gen.label_path_list))

        def getitem_ms(augment):
            gen.augment = augment
            sync()
            t0 = time.perf_counter()
            for c in range(args.calls):
                seed(c)
                gen[0]
            sync()
            return (time.perf_counter() - t0) * 1e3 / args.calls

        def decode_ms():
            t0 = time.perf_counter()
            out = [gen.decode(*p) for p in paths]
            return (time.perf_counter() - t0) * 1e3, out

        def upload_ms(decoded):
            sync()
            t0 = time.perf_counter()
            out = [gen.upload(*d) for d in decoded]
            sync()
            return (time.perf_counter() - t0) * 1e3, out

        oi = torch.empty((BATCH,) + DST + (3,), dtype=torch.uint8, device='cuda')
        ol = torch.empty((BATCH, DST[0] * DST[1], 1), dtype=torch.uint8, device='cuda')

        def one(n, image, label, augment):
            if augment:
                image, label = gen.augment_chain(image, label)
            A.resize(image, label, DST, out=(oi[n], ol[n]))

        def chain_ms(uploaded, augment, idle):
            """(device ms between events, host ms of the enqueue) for the 16 chains"""
            seed(0)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(BATCH if idle else 1)]
            sync()
            t0 = time.perf_counter()
            if idle:
                for n, (im, lb) in enumerate(uploaded):
                    sync()
                    ev[n][0].record()
                    one(n, im, lb, augment)
                    ev[n][1].record()
            else:
                ev[0][0].record()
                for n, (im, lb) in enumerate(uploaded):
                    one(n, im, lb, augment)
                ev[0][1].record()
            host = (time.perf_counter() - t0) * 1e3
            sync()
            return sum(a.elapsed_time(b) for a, b in ev), host

        # warm-up: code objects, the allocator's blocks, PIL's decoders
        for augment in (True, False):
            getitem_ms(augment)
        _, decoded = decode_ms()
        _, uploaded = upload_ms(decoded)
        for augment in (True, False):
            for idle in (False, True):
                chain_ms(uploaded, augment, idle)
        names = ['__getitem__, augment=True', '__getitem__, augment=False', 'PIL decode (host)', 'upload (16 copies)',
                 'device chain, augment=True, back to back', 'device chain, augment=True, idle-queued',
                 'host time to enqueue that chain', 'device chain, augment=False (16 resizes), back to back',
                 'device chain, augment=False, idle-queued']
        t = {k: [] for k in names}
        for _ in range(args.windows):
            t[names[0]].append(getitem_ms(True))
            t[names[1]].append(getitem_ms(False))
            ms, decoded = decode_ms()
            t[names[2]].append(ms)
            ms, uploaded = upload_ms(decoded)
            t[names[3]].append(ms)
            dev, host = chain_ms(uploaded, True, False)
            t[names[4]].append(dev)
            t[names[6]].append(host)
            t[names[5]].append(chain_ms(uploaded, True, True)[0])
            t[names[7]].append(chain_ms(uploaded, False, False)[0])
            t[names[8]].append(chain_ms(uploaded, False, True)[0])
        seed(0)
        gen.augment = True
        rec = []
        orig = A.lib

        class Count:
            def __getattr__(self, name):
                fn = getattr(orig(), name)
                return lambda *a: (rec.append(name), fn(*a))[1]
        A.lib = lambda: Count()
        gen[0]
        A.lib = orig
        sync()
    lines = ['batch %d, %d x %d JPEG -> %d x %d, %d windows of %d calls; ms per batch, median (min..max); %d library calls in the seeded '
             'augment=True batch' % (BATCH, SRC[0], SRC[1], DST[0], DST[1], args.windows, args.calls, len(rec)), '',
             '| part | ms per batch of 16 |', '|---|---|']
    lines += ['| %s | %s |' % (k, spread(t[k])) for k in names]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
