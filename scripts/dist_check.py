"""single-rank check of the data-parallel plumbing: with DL3P_FORCE_DIST=1 (RCCL collectives captured into the graphs,
deferred weight gradients) the loss trajectory must equal the plain single-GPU run bit for bit.  The single-GPU run it
is compared with has DL3P_FOLD_APPLY=0: its default folds some BatchNorm-backward apply passes into weight-gradient
kernels (dz = A*g*m - C*z + D instead of c0*(g*m - c1 - xhat*c2): equal to rounding, not bit for bit), which the
data-parallel path (SyncBatchNorm: apply after the all-reduce) does not; the default run is held to rounding distance."""
import importlib, os, subprocess, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == 'child':
    sys.path.insert(0, ROOT)
    import torch
    if os.environ.get('DL3P_FORCE_DIST'):
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29533')
        os.environ.setdefault('RANK', '0'); os.environ.setdefault('WORLD_SIZE', '1')
        dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    pkg = importlib.import_module('tf-keras-deeplabv3p-model-set_amd')
    model = pkg.get_deeplabv3p_model('mobilenetv2', 21, (129, 129), 16, training=True)
    model.compile(optimizer=pkg.SGD(0.05, momentum=0.9), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    gen = torch.Generator(device='cuda'); gen.manual_seed(7)
    x = torch.rand((4, 129, 129, 3), device='cuda', generator=gen) * 2 - 1
    y = torch.randint(0, 21, (4, 129 * 129, 1), device='cuda', generator=gen).float()
    if os.environ.get('DL3P_CHECK_PERTURB'):       # how fast does a rounding-sized change of the input grow? (chaos yardstick)
        x = x * (1 + float(os.environ['DL3P_CHECK_PERTURB']) * torch.randn(x.shape, device='cuda', generator=gen))
    ex = model._executor(4, True); ex.set_inputs(x, y); ex.lr.fill_(0.05)
    ex.train_step(); ex.capture()
    losses = []
    for _ in range(5):
        ex.train_step(); losses.append(float(ex.loss.item()))
    print('LOSSES ' + json.dumps(losses))
    if os.environ.get('DL3P_FORCE_DIST'):
        dist.destroy_process_group()
else:
    out = {}
    for tag, env in (('single', {'DL3P_FOLD_APPLY': '0'}), ('single_default', {}), ('forced_dist', {'DL3P_FORCE_DIST': '1'}),
                     ('forced_dist_segmented', {'DL3P_FORCE_DIST': '1', 'DL3P_COLLECTIVES_IN_GRAPH': '0'})):
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, __file__, 'child'], env=e, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith('LOSSES')]
        if not line:
            # the error line first: a C++ backtrace after it can fill the tail on its own
            errs = [l for l in r.stderr.splitlines() if 'rror' in l and not l.lstrip().startswith('frame #')][:5]
            print(tag, 'FAILED rc=%d' % r.returncode, '\n'.join(errs), r.stderr[-2000:]); sys.exit(1)
        out[tag] = json.loads(line[0][7:])
        print(tag, out[tag])
    assert out['single'] == out['forced_dist'] == out['forced_dist_segmented'], 'trajectories differ'
    # yardstick: a 1-ulp perturbation of the input (DL3P_CHECK_PERTURB=1e-7) moves the first of these losses by 2.6e-4
    # and the later ones by up to 2e-3 (lr 0.05 on a fresh initialisation, batch 4); the fold moves the first by 7e-8
    a, b = out['single'], out['single_default']
    assert abs(a[0] - b[0]) <= 1e-5 * abs(a[0]) and all(abs(u - v) <= 5e-3 * abs(u) for u, v in zip(a, b)), 'folded apply drifts'
    print('OK identical')
