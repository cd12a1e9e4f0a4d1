"""Hard-example mining without a device: the rule of DESIGN section 7 (tests/mining_rules.py) against hand-worked answers, and the
keywords, mining_spec and loss_spec of losses.py."""
import numpy as np
import pytest

from conftest import load_pkg
import mining_rules as R


@pytest.mark.parametrize('P,p,k', [(1, 0.25, 1), (1, 1.0, 1),                          # int(0.25) = 0 -> clamped to 1
                                   (3, 0.1, 1), (3, 0.5, 1), (3, 0.9, 2), (3, 1.0, 3),    # 0.3 -> 0 -> 1; 1.5 -> 1; 2.7 -> 2
                                   (7, 0.25, 1), (7, 0.5, 3), (7, 0.99, 6), (7, 1.0, 7)])  # 1.75 -> 1; 3.5 -> 3; 6.93 -> 6
def test_k_truncates_and_is_clamped(P, p, k):
    assert R.kept_count(P, p, 0, 0) == k
    assert R.kept_count(P, p, 0, 12345) == k        # without a ramp the step does not matter


@pytest.mark.parametrize('s,k', [(0, 1000), (5, 625), (10, 250), (20, 250)])       # r = 0, 0.5, 1, min(1, 2): (r/4 + 1 - r) * 1000
def test_k_follows_the_ramp(s, k):
    assert R.kept_count(1000, 0.25, 10, s) == k


def test_the_ramp_is_evaluated_in_the_order_written():
    # (r p + (1 - r)) P with r = 1/3, p = 0.1, P = 30: 0.0333.. + 0.6666.. = 0.7000000000000001, times 30 = 21.000000000000004 -> 21
    assert R.kept_count(30, 0.1, 3, 1) == 21
    assert R.kept_count(3, 0.7, 0, 0) == 2         # 0.7 * 3 = 2.0999999999999996 in float64


def test_all_tied_maps_keep_everything():
    k, theta, keep, m, m_plus, scale = R.rule(np.full(4, 2.0, np.float32), 0.25, 0, 0)
    assert (k, float(theta), m, m_plus, float(scale)) == (1, 2.0, 4, 4, 1.0) and keep.all()
    assert R.mined_loss(np.full(4, 2.0, np.float32), 0.25, 0, 0) == 2.0


def test_fewer_than_k_nonzero_losses():
    l = np.array([0, 0, 0.5, 0, 0, 0, 1.5, 0], np.float32)
    k, theta, keep, m, m_plus, scale = R.rule(l, 0.5, 0, 0)
    assert (k, float(theta), m, m_plus, float(scale)) == (4, 0.0, 8, 2, 4.0) and keep.all()
    assert R.mined_loss(l, 0.5, 0, 0) == 1.0        # (0.5 + 1.5) / 2: DeepLab's num_present normaliser


def test_negative_zero_is_zero():
    l = np.array([-0.0, 0.0, 1.0], np.float32)
    k, theta, keep, m, m_plus, scale = R.rule(l, 0.7, 0, 0)          # 2.1 -> 2
    assert (k, float(theta), m, m_plus, float(scale)) == (2, 0.0, 3, 1, 3.0) and keep.all()
    assert not np.signbit(theta)


def test_infinity_sorts_above_every_finite_loss():
    l = np.array([1.0, np.inf, 3.0], np.float32)
    k, theta, keep, m, m_plus, scale = R.rule(l, 0.34, 0, 0)         # 1.02 -> 1
    assert (k, m, m_plus, float(scale)) == (1, 1, 1, 3.0) and np.isposinf(theta) and keep.tolist() == [False, True, False]
    k, theta, keep, m, m_plus, _ = R.rule(l, 0.67, 0, 0)             # 2.01 -> 2
    assert (k, float(theta), m, m_plus) == (2, 3.0, 2, 2) and keep.tolist() == [False, True, True]


def test_a_plain_selection():
    l = np.array([0.5, 4.0, 1.0, 3.0, 3.0, 2.0, 0.0, 0.25], np.float32)
    k, theta, keep, m, m_plus, scale = R.rule(l, 0.25, 0, 0)         # k = 2: 4.0 and a 3.0 -> both 3.0s stay
    assert (k, float(theta), m, m_plus) == (2, 3.0, 3, 3) and keep.tolist() == [False, True, False, True, True, False, False, False]
    assert scale == np.float32(8.0 / 3.0)
    assert R.mined_loss(l, 0.25, 0, 0) == 10.0 / 3.0


def _losses(pkg):
    return [lambda **kw: pkg.SparseCategoricalCrossEntropy(ignore_index=255, **kw),
            lambda **kw: pkg.WeightedSparseCategoricalCrossEntropy([1.0, 2.0], ignore_index=255, **kw),
            lambda **kw: pkg.SparseSoftmaxFocalLoss(ignore_index=255, **kw)]


@pytest.mark.parametrize('kw', [dict(top_k_percent_pixels=0.0), dict(top_k_percent_pixels=-0.5), dict(top_k_percent_pixels=1.5),
                                dict(top_k_percent_pixels=float('nan')), dict(top_k_percent_pixels='0.5'),
                                dict(top_k_percent_pixels=None), dict(hard_example_mining_step=-1),
                                dict(hard_example_mining_step=2.5), dict(hard_example_mining_step=10.0),
                                dict(hard_example_mining_step=None)])
def test_bad_keywords_are_refused(kw):
    for make in _losses(load_pkg()):
        with pytest.raises(ValueError):
            make(**kw)


def test_the_keywords_are_keyword_only():
    pkg = load_pkg()
    with pytest.raises(TypeError):
        pkg.SparseCategoricalCrossEntropy(255, False, 0.5)
    with pytest.raises(TypeError):
        pkg.WeightedSparseCategoricalCrossEntropy([1.0, 2.0], 255, False, 0.5)
    with pytest.raises(TypeError):
        pkg.SparseSoftmaxFocalLoss(2.0, 0.25, 255, False, 0.5)


def test_mining_spec_and_loss_spec():
    pkg, losses = load_pkg(), load_pkg('losses')
    for make in _losses(pkg):
        assert losses.mining_spec(make()) is None
        assert losses.mining_spec(make(top_k_percent_pixels=1.0, hard_example_mining_step=100)) is None      # p == 1.0 means off
        assert losses.mining_spec(make(top_k_percent_pixels=0.25)) == (0.25, 0)
        assert losses.mining_spec(make(top_k_percent_pixels=0.25, hard_example_mining_step=np.int64(7))) == (0.25, 7)
        assert losses.mining_spec(make(top_k_percent_pixels=1)) is None
    assert losses.mining_spec(None) is None
    # loss_spec returns what it returned before the keywords existed, with and without them
    for kw in ({}, dict(top_k_percent_pixels=0.25, hard_example_mining_step=3)):
        ce, wce, focal = [make(**kw) for make in _losses(pkg)]
        assert losses.loss_spec(ce) == ('ce',)
        spec = losses.loss_spec(wce)
        assert spec[0] == 'weighted' and len(spec) == 2 and spec[1] is wce.weights and spec[1].dtype == np.float32
        assert losses.loss_spec(focal) == ('focal', 2.0, 0.25)
    assert losses.loss_spec(None) == ('ce',)
