"""The model front end on the device: no call adds an attribute to a model or to an executor, evaluate() fetches every batch once and
pairs its images with its own labels, the three ways to class ids agree for every kind of input, and each executor is captured into
a graph on its second training step.  Sizes: the smallest the model tests of each family use."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu

# family -> (factory name, arguments in front of `training`, batch size)
FAMILIES = {'deeplabv3p': ('get_deeplabv3p_model', ('mobilenetv2_lite', 21, (65, 65), 16), 2),
            'unet': ('get_unet_model', ('unet_lite', 21, (32, 32)), 2),
            'fast_scnn': ('get_fast_scnn_model', ('fast_scnn', 21, (256, 256)), 1)}


def _batch(N, H, W, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    y = rng.integers(0, C, (N, H * W, 1)).astype(np.uint8)
    y[rng.uniform(size=y.shape) < 0.05] = 255
    return x, y


def _randomise(m, seed=42):
    """non-trivial BatchNorm parameters, moving statistics and biases (test_tta_gpu._randomise): a freshly initialised network gives
    every class the same float32 probability, and then neither a loss nor an argmax of probabilities tells two inputs apart"""
    rng = np.random.default_rng(seed)
    w = m.get_weights_by_name()
    for k, v in w.items():
        if k.endswith('/gamma') or k.endswith('/moving_variance'):
            w[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith('/beta') or k.endswith('/moving_mean') or k.endswith('/bias'):
            w[k] = (rng.standard_normal(v.shape) * 0.1).astype(np.float32)
    m.set_weights_by_name(w)


class _Gen:
    def __init__(self, *batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        return self.batches[i % len(self.batches)]


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_no_call_adds_an_attribute(family):
    pkg = load_pkg()
    factory, args, N = FAMILIES[family]
    C, (H, W) = args[1], args[2]
    m = getattr(pkg, factory)(*args, training=True)
    built = set(vars(m))
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255), metrics={'pred_mask': pkg.Jaccard})
    x, y = _batch(N, H, W, C, seed=1)
    gen = _Gen((x, y), _batch(N, H, W, C, seed=2))
    m.train_on_batch(x, y)
    assert set(vars(m)) == built
    m.fit(gen, steps_per_epoch=2, epochs=1, validation_data=gen, validation_steps=1, verbose=0)
    assert set(vars(m)) == built and 'Jaccard' in m.last_val_metrics and 'Jaccard' in m.last_metrics
    m.predict(x)
    m.predict_mask(x)
    m.evaluate_miou(gen)
    if family == 'deeplabv3p':
        m.predict_tta(x, scales=(0.5, 1.0), flip=True)
        assert list(m._tta_cache) == [(33, 33)]
    assert set(vars(m)) == built

    # the executors: an inference one over its three entry points, a fresh training one over two eager steps
    ex = m._executor(N, False)
    traced = set(vars(ex))
    ex.set_inputs(x, y)
    ex.eval_step(torch.zeros(C * C, dtype=torch.int64, device='cuda'))
    ex.eval_logits()
    ex.eval_loss_step(torch.zeros((N, 3, C), dtype=torch.int32, device='cuda'))
    assert set(vars(ex)) == traced and ex._eval_plan is not None
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    ex = m._executor(N, True)
    traced = set(vars(ex))
    ex.set_inputs(x, y)
    ex.lr.fill_(0.01)
    ex.train_step()
    ex.train_step()
    assert np.isfinite(float(ex.loss.item()))
    assert set(vars(ex)) == traced and ex.steps_run == 0 and ex._eval_plan is None


def test_evaluate_fetches_each_batch_once_and_pairs_it_with_its_own_labels():
    """a generator that draws per fetch (every augmenting one does): its labels differ on every fetch of the same index.  evaluate()
    takes images and labels from ONE fetch per batch, so its loss is, bit for bit, that of the same bytes handed over as CUDA uint8
    tensors -- the path that always fetched once"""
    pkg = load_pkg()
    N, C, H, W = 2, 21, 65, 65
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', C, (H, W), 16, training=False, seed=3)
    _randomise(m)
    m.compile(optimizer=None, loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255), metrics={'pred_mask': pkg.Jaccard})
    images = [_batch(N, H, W, C, seed=10 + i)[0] for i in range(2)]

    class Drawing:
        def __init__(self):
            self.fetches, self.served = 0, []

        def __len__(self):
            return 2

        def __getitem__(self, i):
            y = _batch(N, H, W, C, seed=100 + self.fetches)[1]         # other labels on every fetch
            self.fetches += 1
            self.served.append((i, y))
            return images[i], y

    gen = Drawing()
    loss = m.evaluate(gen)
    assert gen.fetches == 2 and [i for i, _ in gen.served] == [0, 1]
    jaccard = m.last_val_metrics['Jaccard']
    assert not np.array_equal(gen.served[0][1], gen.served[1][1])
    on_device = _Gen(*[(torch.from_numpy(images[i]).cuda(), torch.from_numpy(y).cuda()) for i, y in gen.served])
    assert m.evaluate(on_device) == loss and m.last_val_metrics['Jaccard'] == jaccard


def test_the_three_ways_to_class_ids_agree(tmp_path):
    inf = load_pkg('inference')
    p = tmp_path / 'classes.txt'
    p.write_text('\n'.join('class%d' % i for i in range(21)) + '\n')
    d = inf.DeepLab(model_type='mobilenetv2_lite', model_input_shape=(65, 65), output_stride=16, classes_path=str(p), weights_path=None)
    m = d.deeplab_model
    _randomise(m)
    u8 = _batch(2, 65, 65, 21, seed=5)[0]
    inputs = {'host float32': u8.astype(np.float32) / 127.5 - 1, 'host uint8': u8, 'CUDA uint8': torch.from_numpy(u8).cuda()}
    masks = {}
    for kind, x in inputs.items():
        mask = m.predict_mask(x)
        ids = d._class_ids(x)
        assert mask.shape == (2, 65, 65) and mask.dtype == np.int32, kind
        assert ids.is_cuda and ids.dtype == torch.int32 and tuple(ids.shape) == (2, 65, 65), kind
        assert torch.equal(m.class_ids(x), ids), kind
        assert np.array_equal(ids.cpu().numpy(), mask), kind
        assert np.array_equal(m.predict(x).argmax(-1), mask), kind
        masks[kind] = mask
    assert np.array_equal(masks['host uint8'], masks['CUDA uint8'])    # the same bytes, normalised by the same kernel


def test_each_executor_is_captured_on_its_second_step():
    pkg = load_pkg()
    C, H, W = 21, 65, 65
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', C, (H, W), 16, training=True)
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    two, one = _batch(2, H, W, C, seed=7), _batch(1, H, W, C, seed=8)
    state = lambda: [(m._executor(n, True).graphed, m._executor(n, True).steps_run) for n in (2, 1) if (n, True) in m._exec]
    m.train_on_batch(*two)
    assert state() == [(False, 1)]
    m.train_on_batch(*one)
    assert state() == [(False, 1), (False, 1)]
    m.train_on_batch(*two)
    assert state() == [(True, 2), (False, 1)]
    m.train_on_batch(*one)
    assert state() == [(True, 2), (True, 2)]
    assert np.isfinite(m.train_on_batch(*two)) and state() == [(True, 3), (True, 2)]
    m.use_graphs = False                                # ... and never without use_graphs
    m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    for _ in range(3):
        m.train_on_batch(*one)
    assert state() == [(False, 3)]
