"""Region losses without a device: the rule of DESIGN section 7 (tests/region_rules.py) against central differences and hand-worked
answers, and the constructors, loss_spec and mining_spec of losses.py."""
import numpy as np
import pytest

from conftest import load_pkg
import region_rules as R

PARAMS = {'dice': (0.5, 0.5), 'jaccard': (1.0, 1.0), 'tversky': (0.3, 0.7)}


def _case(C, n=40, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, C)) * 2.0
    y = rng.integers(0, C, n)
    y[rng.uniform(size=n) < 0.2] = 255
    return z, y


@pytest.mark.parametrize('C', [5, 21, 40])
@pytest.mark.parametrize('kind', sorted(PARAMS))
def test_the_gradient_matches_central_differences(kind, C):
    alpha, beta = PARAMS[kind]
    z, y = _case(C, seed=C)
    out = R.region(z, y, alpha, beta, smooth=1.0, rho=0.7)
    assert out['present'] >= 2
    rng = np.random.default_rng(1)
    eps, worst = 1e-5, 0.0
    for _ in range(60):
        i, k = rng.integers(0, z.shape[0]), rng.integers(0, C)
        zp, zm = z.copy(), z.copy()
        zp[i, k] += eps
        zm[i, k] -= eps
        num = (R.value(zp, y, alpha, beta, 1.0, 0.7) - R.value(zm, y, alpha, beta, 1.0, 0.7)) / (2 * eps)
        worst = max(worst, abs(num - out['grad'][i, k]))
    scale = np.abs(out['grad']).max()
    print('%s C %d: worst |numeric - rule| = %.3g of scale %.3g' % (kind, C, worst, scale))
    assert worst <= 1e-6 * scale          # central differences at eps = 1e-5 in float64: O(eps^2) truncation + 1e-16 / eps rounding


def test_dice_is_tversky_at_one_half_and_jaccard_is_the_soft_iou():
    z, y = _case(7, seed=3)
    I, P, Y, _ = R.sums(z, y)
    S = Y > 0
    d = R.region(z, y, 0.5, 0.5, smooth=1.0)
    assert np.allclose(d['score'][S], (2 * I[S] + 2.0) / (P[S] + Y[S] + 2.0), rtol=1e-14, atol=0)
    j = R.region(z, y, 1.0, 1.0, smooth=0.5)
    assert np.allclose(j['score'][S], (I[S] + 0.5) / (P[S] + Y[S] - I[S] + 0.5), rtol=1e-14, atol=0)
    assert abs(d['loss'] - np.mean(1 - d['score'][S])) < 1e-15


def test_a_two_pixel_case_by_hand():
    # two pixels, two classes, uniform probabilities; labels 0 and 0: I = (1, 0), P = (1, 1), Y = (2, 0); S = {0}
    z = np.zeros((2, 2))
    out = R.region(z, [0, 0], 0.5, 0.5, smooth=0.0)
    assert out['present'] == 1 and np.isnan(out['score'][1])
    assert out['score'][0] == 1.0 / 1.5 and abs(out['loss'] - (1 - 1.0 / 1.5)) < 1e-16
    assert out['A'][1] == 0 and out['B'][1] == 0


def test_an_absent_class_with_large_probabilities_gets_no_gradient_of_its_own():
    z, y = _case(5, seed=4)
    y[y == 3] = 1
    z[:, 3] += 8.0                       # class 3 takes nearly all the probability and is in no label
    out = R.region(z, y, 0.5, 0.5)
    assert out['Y'][3] == 0 and out['P'][3] > 0.9 * (y != 255).sum()
    assert np.isnan(out['score'][3]) and out['A'][3] == 0 and out['B'][3] == 0 and out['present'] == 4
    # g_i3 = 0: moving class 3's probabilities changes R only through the other classes' P_c
    prob = R.softmax(z)
    g = out['B'][None] - np.eye(5)[np.where(y == 255, 0, y)] * out['A'][None]
    assert np.allclose(out['grad'][y != 255, 3], (prob * (0 - (prob * g).sum(axis=1, keepdims=True)))[y != 255, 3])


def test_all_labels_ignored_is_zero_with_zero_gradient():
    z, _ = _case(5, seed=5)
    out = R.region(z, np.full(z.shape[0], 255), 1.0, 1.0)
    assert out['loss'] == 0.0 and out['present'] == 0 and not out['grad'].any() and np.isnan(out['score']).all()


def test_labels_outside_the_classes_count_nowhere():
    z, y = _case(5, seed=6)
    y2 = y.copy()
    y2[:4] = [-1, 5, -1, 5]
    keep = np.ones(y.size, bool)
    keep[:4] = False
    a, b = R.region(z, y2, 0.3, 0.7), R.region(z[keep], y[keep], 0.3, 0.7)
    for k in ('I', 'P', 'Y', 'A', 'B'):
        assert np.array_equal(a[k], b[k]), k
    assert a['loss'] == b['loss'] and not a['grad'][:4].any() and np.array_equal(a['grad'][4:], b['grad'])
    # ignore_index 0 (or None) masks nothing: loss.py's truthiness
    assert R.sums(z, np.zeros(y.size, int), ignore_index=0)[2][0] == y.size


def test_the_base_gradient_matches_central_differences():
    z, y = _case(6, n=12, seed=7)
    z[3, 0], y[3] = 60.0, 2              # a saturated pixel with another label: p_y = e^-60 lies below both clips
    pw = np.random.default_rng(8).uniform(0.5, 2.0, 12)
    for spec in (('ce',), ('weighted', np.linspace(0.5, 2.0, 6)), ('focal', 2.0, 0.25)):
        _, grad = R.base_gradient(z, y, spec, 255, pw)
        for i, k in ((0, 0), (3, 2), (11, 5)):
            zp, zm = z.copy(), z.copy()
            zp[i, k] += 1e-5
            zm[i, k] -= 1e-5
            num = (R.base_gradient(zp, y, spec, 255, pw)[0] - R.base_gradient(zm, y, spec, 255, pw)[0]) / 2e-5
            assert abs(num - grad[i, k]) <= 1e-6 * np.abs(grad).max(), (spec[0], i, k)


# ------------------------------------------------------------------------------------------------ losses.py
BAD = [dict(from_logits=True), dict(alpha=0.0), dict(alpha=-1.0), dict(beta=0.0), dict(beta=-0.5), dict(smooth=-1e-3),
       dict(alpha=float('nan')), dict(beta=float('inf')), dict(smooth=float('nan')), dict(region_weight=float('inf')),
       dict(base_weight=float('nan')), dict(region_weight=0.0), dict(region_weight=-1.0), dict(base_weight=-0.1),
       dict(base='ce'), dict(base=object()), dict(alpha='0.5')]


def _bad_id(kw):
    """the case's arguments as its id; a bare object() by name, not by its address (which differs from run to run)"""
    return str(sorted((n, 'object()' if type(v) is object else v) for n, v in kw.items()))


@pytest.mark.parametrize('kw', BAD, ids=[_bad_id(k) for k in BAD])
def test_bad_arguments_are_refused_with_their_value(kw):
    pkg = load_pkg()
    with pytest.raises(ValueError) as e:
        pkg.SparseTverskyLoss(**kw)
    value = list(kw.values())[0]
    assert repr(value) in str(e.value), (kw, str(e.value))
    if set(kw) & {'alpha', 'beta'}:
        return                                      # Dice and Jaccard fix alpha and beta
    for cls in (pkg.SparseDiceLoss, pkg.SparseJaccardLoss):
        with pytest.raises(ValueError):
            cls(**kw)


def test_a_base_must_share_the_label_rule_and_be_a_per_pixel_loss():
    pkg = load_pkg()
    with pytest.raises(ValueError) as e:
        pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy(ignore_index=254))
    assert '254' in str(e.value) and '255' in str(e.value)
    with pytest.raises(ValueError):
        pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy())
    with pytest.raises(ValueError):
        pkg.SparseDiceLoss(base=pkg.SparseDiceLoss())             # a region loss is no base
    with pytest.raises(TypeError):
        pkg.SparseDiceLoss(1.0, 255, False, pkg.SparseCategoricalCrossEntropy(ignore_index=255))      # keyword-only
    ok = pkg.SparseJaccardLoss(ignore_index=255, base=pkg.SparseSoftmaxFocalLoss(ignore_index=255), base_weight=0.0)
    assert ok.base_weight == 0.0 and ok.ignore_index == 255 and (ok.alpha, ok.beta) == (1.0, 1.0)


def test_loss_spec_and_mining_spec():
    pkg, losses = load_pkg(), load_pkg('losses')
    from deeplabv3p import loss as shim
    for name in ('SparseTverskyLoss', 'SparseDiceLoss', 'SparseJaccardLoss'):
        assert getattr(shim, name) is getattr(pkg, name) is getattr(losses, name) and name in pkg.__all__
    assert losses.loss_spec(pkg.SparseDiceLoss()) == ('region', 0.5, 0.5, 1.0, 1.0, 1.0, None)
    assert losses.loss_spec(pkg.SparseJaccardLoss(smooth=0, region_weight=2)) == ('region', 1.0, 1.0, 0.0, 2.0, 1.0, None)
    focal = pkg.SparseSoftmaxFocalLoss(ignore_index=255, top_k_percent_pixels=0.25, hard_example_mining_step=3)
    t = pkg.SparseTverskyLoss(0.3, 0.7, 0.5, 255, base=focal, base_weight=0.5, region_weight=2.0)
    assert losses.loss_spec(t) == ('region', 0.3, 0.7, 0.5, 2.0, 0.5, ('focal', 2.0, 0.25))
    assert losses.mining_spec(t) == (0.25, 3)                     # read through to the base
    assert losses.mining_spec(pkg.SparseDiceLoss()) is None
    assert losses.mining_spec(pkg.SparseDiceLoss(ignore_index=255, base=pkg.SparseCategoricalCrossEntropy(ignore_index=255))) is None
    wce = pkg.WeightedSparseCategoricalCrossEntropy([1.0, 2.0], ignore_index=255)
    spec = losses.loss_spec(pkg.SparseDiceLoss(ignore_index=255, base=wce))
    assert spec[6][0] == 'weighted' and spec[6][1] is wce.weights
    # the existing classes answer what they answered
    assert losses.loss_spec(pkg.SparseCategoricalCrossEntropy(ignore_index=255)) == ('ce',)
    assert losses.loss_spec(focal) == ('focal', 2.0, 0.25) and losses.mining_spec(focal) == (0.25, 3)
    assert losses.loss_spec(wce)[0] == 'weighted' and losses.loss_spec(None) == ('ce',) and losses.mining_spec(None) is None


def test_the_nearest_head_refuses_a_region_loss_before_any_launch():
    pkg = load_pkg()
    m = pkg.get_fast_scnn_model('fast_scnn', 21, (256, 256))
    with pytest.raises(ValueError, match='nearest') as e:
        m.compile(optimizer=pkg.SGD(0.01), loss=pkg.SparseDiceLoss(ignore_index=255))
    assert 'dl3p_nearest_region_sums' in str(e.value)
    assert m.last_region is None
