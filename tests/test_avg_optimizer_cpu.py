"""Averaged optimisers (train.py --average_type, common/model_utils.py:133-172) without a device: the get_optimizer surface,
the wrappers' delegation, the argument checks of the dl3p_*_avg entry points and the step schedule of the float64
restatement the GPU tests are checked against (tests/avg_rules.py)."""
import numpy as np
import pytest

import avg_rules as R
from conftest import load_pkg

BASES = ('sgd', 'adam', 'rmsprop')


@pytest.mark.parametrize('base', BASES)
def test_get_optimizer_returns_the_wrappers_with_the_reference_constants(base):
    pkg = load_pkg()
    cls = {'sgd': pkg.SGD, 'adam': pkg.Adam, 'rmsprop': pkg.RMSprop}[base]
    plain = pkg.get_optimizer(base, 1e-2)
    ema = pkg.get_optimizer(base, 1e-2, average_type='ema')
    assert type(ema) is pkg.MovingAverage and ema.avg_spec() == ('ema', 0.99)
    swa = pkg.get_optimizer(base, 1e-2, average_type='swa')
    assert type(swa) is pkg.SWA and swa.avg_spec() == ('swa', 0, 10)
    la = pkg.get_optimizer(base, 1e-2, average_type='lookahead')
    assert type(la) is pkg.Lookahead and la.avg_spec() == ('lookahead', 6, 0.5)
    for o in (ema, swa, la):
        assert type(o._optimizer) is cls and o.spec() == plain.spec()
        assert o.iterations == 0 and o.learning_rate == 1e-2
    assert type(pkg.get_optimizer(base, 1e-2, average_type='EMA')) is pkg.MovingAverage      # (the reference lower-cases it)
    assert not hasattr(plain, 'avg_spec')


def test_unknown_average_type_and_unbuilt_arguments_raise():
    pkg = load_pkg()
    with pytest.raises(ValueError, match='Unsupported average type'):
        pkg.get_optimizer('sgd', 1e-2, average_type='polyak')
    with pytest.raises(ValueError, match='Unsupported optimizer type'):
        pkg.get_optimizer('adagrad', 1e-2, average_type='ema')
    sgd = pkg.SGD(0.01)
    with pytest.raises(ValueError):
        pkg.MovingAverage(sgd, num_updates=100)
    with pytest.raises(ValueError):
        pkg.MovingAverage(sgd, dynamic_decay=True)
    with pytest.raises(ValueError):
        pkg.MovingAverage(sgd, start_step=5)
    assert pkg.MovingAverage(sgd, start_step=0).avg_spec() == ('ema', 0.99)
    with pytest.raises(ValueError):
        pkg.SWA(sgd, average_period=0)
    with pytest.raises(ValueError):
        pkg.Lookahead(sgd, sync_period=0)
    with pytest.raises(ValueError):
        pkg.Lookahead(sgd, name='Lookahead')
    with pytest.raises(ValueError):
        pkg.SWA(pkg.SWA(sgd))


@pytest.mark.parametrize('kind', ['ema', 'swa', 'lookahead'])
def test_schedules_and_iterations_pass_through_the_wrapper(kind):
    pkg = load_pkg()
    for decay in ('cosine', 'exponential', 'polynomial', 'piecewise_constant'):
        plain = pkg.get_optimizer('sgd', 1e-2, decay_type=decay, decay_steps=1000)
        avg = pkg.get_optimizer('sgd', 1e-2, average_type=kind, decay_type=decay, decay_steps=1000)
        for s in (0, 1, 499, 501, 900, 1000, 2500):
            assert avg.lr_at(s) == plain.lr_at(s)
    avg.iterations += 3
    assert avg._optimizer.iterations == 3 and avg.iterations == 3
    avg.learning_rate = 0.5
    assert avg._optimizer.learning_rate == 0.5 and avg.lr_at(7) == 0.5


def test_models_without_an_averaged_optimizer_refuse_the_average_calls():
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', 21, (65, 65), 16)
    m.compile(optimizer=pkg.SGD(0.01))
    with pytest.raises(RuntimeError, match='does not average'):
        m.get_average_weights()
    with pytest.raises(RuntimeError, match='does not average'):
        m.assign_average_vars()


def test_entry_points_check_their_arguments_before_any_launch():
    """bad avg_mode, bad period, null / misaligned avg: refused with DL3P_EINVAL and a message, no device needed"""
    L = load_pkg('_lib').lib()
    n = 64
    bufs = [np.zeros(n + 4, np.float32) for _ in range(5)]
    ptr = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]        # 16-byte aligned host addresses: never dereferenced
    w, s1, s2, g, avg = ptr
    lr = np.zeros(4, np.float32).ctypes.data
    step = np.ones(2, np.int64).ctypes.data

    def calls(avg, mode, period, step=step):
        tail = (avg, mode, 0.99, period, 0)
        return [('sgd_momentum_avg', (w, s1, g, n, lr, 0.9, 0.0, 1.0, None, None) + tail + (step, None)),
                ('adam_step_avg', (w, s1, s2, g, n, lr, step, 0.9, 0.999, 1e-7, 1.0, None, None) + tail + (None,)),
                ('rmsprop_step_avg', (w, s2, g, n, lr, 0.9, 1e-7, 1.0, None, None) + tail + (step, None)),
                ('weight_average', (w, avg, n, mode, 0.99, period, 0, step, None, None))]

    bad = [('avg_mode', calls(avg, 0, 1)), ('avg_mode', calls(avg, 4, 1)), ('avg_period', calls(avg, 2, 0)),
           ('avg_period', calls(avg, 3, -6)), ('null', calls(None, 1, 1)), ('aligned', calls(avg + 4, 1, 1)),
           ('null', calls(avg, 1, 1, step=None))]
    for word, group in bad:
        for name, args in group:
            fn = getattr(L, name)
            assert fn.raw(*args) == -1, (name, word)                      # DL3P_EINVAL
            with pytest.raises(load_pkg('_lib').Dl3pError, match=word):
                fn(*args)


def test_header_declares_the_four_entry_points():
    protos = load_pkg('_lib').parse_header()
    for name in ('dl3p_sgd_momentum_avg', 'dl3p_adam_step_avg', 'dl3p_rmsprop_step_avg', 'dl3p_weight_average'):
        ret, args = protos[name]
        assert ret == 'int' and args[-1] == 'void*'
    sib = protos['dl3p_sgd_momentum'][1]
    assert protos['dl3p_sgd_momentum_avg'][1] == sib[:-1] + ['float*', 'int', 'float', 'int', 'int', 'const int64_t*', 'void*']
    sib = protos['dl3p_rmsprop_step'][1]
    assert protos['dl3p_rmsprop_step_avg'][1] == sib[:-1] + ['float*', 'int', 'float', 'int', 'int', 'const int64_t*', 'void*']
    sib = protos['dl3p_adam_step'][1]
    assert protos['dl3p_adam_step_avg'][1] == sib[:-1] + ['float*', 'int', 'float', 'int', 'int', 'void*']


def test_helper_schedule():
    """with the reference's constants SWA takes its snapshots at steps 1, 11, 21 (the next one is step 31: iteration 30)
    and Lookahead syncs at 6, 12, 18"""
    assert [t for t in range(1, 32) if R.swa_snapshot(t) is not None] == [1, 11, 21, 31]
    assert [R.swa_snapshot(t) for t in (1, 11, 21, 31)] == [0, 1, 2, 3]
    assert [t for t in range(1, 31) if R.swa_snapshot(t) is not None] == [1, 11, 21]
    assert [t for t in range(1, 24) if R.lookahead_syncs(t)] == [6, 12, 18]
    assert [t for t in range(1, 40) if R.swa_snapshot(t, start=5, period=7) is not None] == [6, 13, 20, 27, 34]


def test_helper_rules_on_known_numbers():
    w = np.array([2.0, -4.0, 8.0])
    a = np.array([1.0, 1.0, 1.0])
    act = np.array([True, True, False])
    assert np.allclose(R.ema_step(a, w, 0.99), [1.01, 0.95, 1.07], rtol=0, atol=1e-15)
    assert np.array_equal(R.ema_step(a, w, 0.99, active=act)[2:], [1.0])
    assert np.array_equal(R.swa_step(a, w, 1), w)                       # the first snapshot is the weights themselves
    assert np.array_equal(R.swa_step(a, w, 2), a)
    assert np.array_equal(R.swa_step(a, w, 11), (a + w) / 2)
    assert np.array_equal(R.swa_step(a, w, 21, active=act), [(2 + 2.0) / 3, (2 - 4.0) / 3, 1.0])
    s, f = R.lookahead_step(a, w, 5)
    assert np.array_equal(s, a) and np.array_equal(f, w)
    s, f = R.lookahead_step(a, w, 6, active=act)
    assert np.array_equal(s, [1.5, -1.5, 1.0]) and np.array_equal(f, [1.5, -1.5, 8.0])
    avg = R.Averager('swa', a)
    for t in range(1, 12):
        out = avg.step(w * t)
    assert np.array_equal(out, (w * 1 + w * 11) / 2)
