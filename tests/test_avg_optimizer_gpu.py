"""Averaged optimisers on the device (train.py --average_type {ema,swa,lookahead}): the fused dl3p_*_avg kernels and the
standalone dl3p_weight_average against the plain entry points (bitwise) and the float64 restatement of the rules
(tests/avg_rules.py), then the same through compile / train_on_batch / graph replay / recompile / fit.

Bound (e) on an average: steps * 2^-23 * M, M the largest magnitude seen in the weights or the slot.  Each update is three
or four rounded float32 operations on values of at most 2 M; ema and lookahead are contractions and swa is a convex
combination, so the errors of earlier steps are not amplified."""
import numpy as np
import pytest
import torch

import avg_rules as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-3                      # the fp32 predict tolerance of tests/test_model_gpu.py
# mixed_bfloat16: both sides of the comparison run the same kernels on mirrors of the same fp32 master weights; one bf16
# ulp of a probability near 1 is the rounding step of the format the activations are stored in
TOL_BF16 = 2.0 ** -8
MODES = {'ema': (1, 0.99, 1, 0), 'swa': (2, 0.0, 10, 0), 'lookahead': (3, 0.5, 6, 0)}
STEPS = {'ema': 25, 'swa': 31, 'lookahead': 25}
HELPER_KW = {'ema': dict(decay=0.99), 'swa': dict(start=0, period=10), 'lookahead': dict(sync_period=6, alpha=0.5)}
SIZES = [3, 10007, 4096 * 256 * 4 + 1029]


def _acts(mode, t):
    if mode == 'ema':
        return True
    if mode == 'swa':
        return R.swa_snapshot(t) is not None
    return R.lookahead_syncs(t)


class _Buffers:
    def __init__(self, opt, w0, l2, lre):
        self.opt = opt
        self.w = w0.clone()
        self.s1 = torch.zeros_like(w0)
        self.s2 = torch.zeros_like(w0)
        self.l2, self.lre = l2, lre
        self.lr = torch.tensor([1e-2 if opt == 'sgd' else 1e-3], dtype=torch.float32, device=DEV)

    def plain(self, L, g, step, st):
        n, p = self.w.numel(), lambda t: t.data_ptr()
        if self.opt == 'sgd':
            L.sgd_momentum(p(self.w), p(self.s1), p(g), n, p(self.lr), 0.9, 0.0, 0.5, p(self.l2), p(self.lre), st)
        elif self.opt == 'adam':
            L.adam_step(p(self.w), p(self.s1), p(self.s2), p(g), n, p(self.lr), p(step), 0.9, 0.999, 1e-7, 0.5, p(self.l2),
                        p(self.lre), st)
        else:
            L.rmsprop_step(p(self.w), p(self.s2), p(g), n, p(self.lr), 0.9, 1e-7, 0.5, p(self.l2), p(self.lre), st)

    def fused(self, L, g, step, avg, mode, st):
        n, p = self.w.numel(), lambda t: t.data_ptr()
        a = (p(avg),) + MODES[mode]
        if self.opt == 'sgd':
            L.sgd_momentum_avg(p(self.w), p(self.s1), p(g), n, p(self.lr), 0.9, 0.0, 0.5, p(self.l2), p(self.lre), *a, p(step), st)
        elif self.opt == 'adam':
            L.adam_step_avg(p(self.w), p(self.s1), p(self.s2), p(g), n, p(self.lr), p(step), 0.9, 0.999, 1e-7, 0.5, p(self.l2),
                            p(self.lre), *a, st)
        else:
            L.rmsprop_step_avg(p(self.w), p(self.s2), p(g), n, p(self.lr), 0.9, 1e-7, 0.5, p(self.l2), p(self.lre), *a, p(step), st)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('mode', ['ema', 'swa', 'lookahead'])
@pytest.mark.parametrize('opt', ['sgd', 'adam', 'rmsprop'])
def test_fused_and_standalone_kernels(ops, opt, mode, n):
    """every optimiser x rule at a size without a vector body, one with body and tail, and one past the grid cap: (a) the
    weights are bitwise the plain entry point's, (b) frozen slots never move, (c) / (d) the swa and lookahead schedules hold
    bitwise, (e) the slot follows the float64 rules driven by the observed weights, (f) the same for dl3p_weight_average
    behind the plain step"""
    L = ops.lib()
    st = ops._stream()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 * n % 7919 + 17)
    w0 = torch.randn(n, device=DEV, generator=gen)
    l2 = torch.where(torch.rand(n, device=DEV, generator=gen) < 0.5, 2e-5, 0.0).float()
    frozen = torch.rand(n, device=DEV, generator=gen) < 0.1
    frozen[1] = True
    lre = torch.where(frozen, 0.0, 1.0).float()
    active = ~frozen
    active_h = active.cpu().numpy()
    fu, tw = _Buffers(opt, w0, l2, lre), _Buffers(opt, w0, l2, lre)
    avg_f, avg_s = w0.clone(), w0.clone()                     # slots start from the weights
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    helper = R.Averager(mode, w0.cpu().numpy(), active=active_h, **HELPER_KW[mode])
    m_seen, steps = float(w0.abs().max()), STEPS[mode]
    for t in range(1, steps + 1):
        g = torch.randn(n, device=DEV, generator=gen) * 10.0 ** (torch.rand(n, device=DEV, generator=gen) * 6 - 6)
        step += 1
        prev_f, prev_s = avg_f.clone(), avg_s.clone()
        fu.fused(L, g, step, avg_f, mode, st)
        tw.plain(L, g, step, st)
        wp = tw.w.clone()                                      # w' of this step: after the update, before any sync
        L.weight_average(tw.w.data_ptr(), avg_s.data_ptr(), n, *MODES[mode], step.data_ptr(), lre.data_ptr(), st)
        acts = _acts(mode, t)
        # (a)
        if mode != 'lookahead' or not acts:
            assert torch.equal(fu.w, wp), (t, 'weights differ from the plain entry point')
        assert torch.equal(fu.s1, tw.s1) and torch.equal(fu.s2, tw.s2), t
        assert torch.equal(tw.w, fu.w), (t, 'standalone pass and fused kernel leave different weights')
        assert torch.equal(fu.w[frozen], w0[frozen])
        # (b)
        assert torch.equal(avg_f[frozen], w0[frozen]) and torch.equal(avg_s[frozen], w0[frozen]), t
        # (c), (d)
        if not acts:
            assert torch.equal(avg_f, prev_f) and torch.equal(avg_s, prev_s), (t, 'slot touched on an idle step')
        if mode == 'swa' and t == 1:
            assert torch.equal(avg_f[active], fu.w[active]) and torch.equal(avg_s[active], tw.w[active])
        if mode == 'lookahead' and acts:
            assert torch.equal(fu.w, avg_f) and torch.equal(tw.w, avg_s), (t, 'weights are not the slow weights after a sync')
        if mode == 'lookahead' and not acts:
            assert not torch.equal(fu.w[active], avg_f[active])
        # (e), (f)
        m_seen = max(m_seen, float(wp.abs().max()), float(avg_f.abs().max()), float(avg_s.abs().max()))
        if acts:
            ref = helper.step(wp.cpu().numpy())
            bound = steps * 2.0 ** -23 * m_seen
            for name, got in (('fused', avg_f), ('standalone', avg_s)):
                err = float(np.abs(got.cpu().numpy() - ref).max())
                assert err <= bound, (name, t, err, bound)
        else:
            helper.step(None)                                  # (an idle step reads no weights)
    assert torch.equal(avg_f, avg_s)


# ------------------------------------------------------------------------------------------------------------ model level
N, H, W, C = 2, 65, 65, 21


def _data(seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (N, H, W, 3)).astype(np.float32)
    y = rng.integers(0, C, (N, H * W, 1)).astype(np.float32)
    y[rng.uniform(size=y.shape) < 0.05] = 255
    return x, y


def _model(optimizer, freeze_level=0, bf16=False):
    pkg = load_pkg()
    if bf16:
        mp = pkg.mixed_precision
        mp.set_policy(mp.Policy('mixed_bfloat16'))
    try:
        m = pkg.get_deeplabv3p_model('mobilenetv2_lite', C, (H, W), 16, freeze_level=freeze_level, seed=0)
    finally:
        if bf16:
            mp.set_policy(mp.Policy('float32'))
    if optimizer is not None:
        m.compile(optimizer=optimizer, loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    return m


def _flat(ws):
    return np.concatenate([np.asarray(w, np.float32).ravel() for w in ws])


def _slot_mask(m):
    """per element of _flat(get_weights()): does the optimiser update it (has it a slot)"""
    return np.concatenate([np.full(int(np.prod(p.shape)), bool(p.trainable)) for p in m._keras_params()])


def _bound(steps, *arrays):
    return steps * 2.0 ** -23 * max(float(np.abs(a).max()) for a in arrays)


def test_ema_over_sgd_eager_capture_and_replays():
    """8 steps = the eager step, the capture and six replays: the device average follows the rule on the observed weights;
    entries without a slot (freeze_level=1 backbone, every BatchNorm moving statistic) keep the initial weights bitwise"""
    pkg = load_pkg()
    m = _model(pkg.get_optimizer('sgd', 1e-2, average_type='ema'), freeze_level=1)
    x, y = _data()
    w0 = _flat(m.get_weights())
    assert np.array_equal(_flat(m.get_average_weights()), w0)          # before the first step: the weights
    mask = _slot_mask(m)
    assert 0 < mask.sum() < mask.size
    helper = R.Averager('ema', w0, active=mask, decay=0.99)
    for t in range(1, 9):
        m.train_on_batch(x, y)
        ws, av = _flat(m.get_weights()), _flat(m.get_average_weights())
        ref = helper.step(ws)
        err, bound = float(np.abs(av - ref).max()), _bound(8, ws, av)
        assert err <= bound, (t, err, bound)
        assert np.array_equal(av[~mask], w0[~mask]), t
        assert not np.array_equal(av[mask], ws[mask]) and not np.array_equal(av[mask], w0[mask])
    assert m._executor(N, True).graphed


def test_swa_over_sgd_snapshots_at_steps_1_and_11():
    pkg = load_pkg()
    m = _model(pkg.get_optimizer('sgd', 1e-2, average_type='swa'))
    x, y = _data()
    mask = _slot_mask(m)
    ws, av = {}, {}
    for t in range(1, 13):
        m.train_on_batch(x, y)
        ws[t], av[t] = _flat(m.get_weights()), _flat(m.get_average_weights())
    assert np.array_equal(av[1][mask], ws[1][mask])
    for t in range(2, 11):
        assert np.array_equal(av[t], av[1]), t
    assert not np.array_equal(av[11][mask], av[10][mask])
    ref = (ws[1].astype(np.float64) + ws[11].astype(np.float64)) / 2
    err, bound = float(np.abs(av[11] - ref)[mask].max()), _bound(12, ws[1], ws[11], av[11])
    assert err <= bound, (err, bound)
    assert np.array_equal(av[12], av[11])


@pytest.mark.parametrize('bf16', [False, True], ids=['float32', 'mixed_bfloat16'])
def test_lookahead_over_adam_syncs_weights_and_mirrors(bf16):
    """the weights equal the slow weights after steps 6 and 12 only, and after the sync of step 6 every weight mirror the
    kernels read (transposes, bf16 copies, split-bf16 planes) is the one made from the synced weights"""
    pkg = load_pkg()
    m = _model(pkg.get_optimizer('adam', 1e-3, average_type='lookahead'), bf16=bf16)
    x, y = _data()
    xp, _ = _data(5)
    mask = _slot_mask(m)
    m.predict(xp)                    # the inference executor exists before training: it reads the mirrors the steps leave
    for t in range(1, 14):
        m.train_on_batch(x, y)
        ws, slow = _flat(m.get_weights()), _flat(m.get_average_weights())
        assert np.array_equal(ws[mask], slow[mask]) == (t in (6, 12)), t
        if t == 6:
            st, ex = m._store, m._executor(N, True)
            mirrors = {'Pt': st.Pt, 'Pb': st.Pb, 'Pbt': st.Pbt}
            mirrors.update({'split fwd ' + op.name: st.sb_fwd[op][0] for op in ex._sb_used_f if op in st.sb_fwd})
            mirrors.update({'split bwd ' + op.name: st.sb_bwd[op][0] for op in ex._sb_used_b if op in st.sb_bwd})
            left = {k: v.clone() for k, v in mirrors.items() if v is not None}
            p = m.predict(xp)
            st.transpose()           # every mirror again, from the weights as they are now
            torch.cuda.synchronize()
            for k, v in left.items():
                assert torch.equal(v, mirrors[k]), 'mirror %s was not made from the synced weights' % k
            fresh = _model(None, bf16=bf16)
            fresh.set_weights(m.get_weights())
            p_ref = fresh.predict(xp)
            worst = float(np.abs(p - p_ref).max())
            assert worst <= (TOL_BF16 if bf16 else TOL), worst
    with pytest.raises(RuntimeError, match='Lookahead'):
        m.assign_average_vars()


def test_recompile_new_object_restarts_the_slot_same_object_keeps_it():
    pkg = load_pkg()
    loss = pkg.SparseCategoricalCrossEntropy(ignore_index=255)
    m = _model(pkg.get_optimizer('sgd', 1e-2, average_type='ema'))
    x, y = _data()
    mask = _slot_mask(m)
    for _ in range(3):
        m.train_on_batch(x, y)
    old_slot = _flat(m.get_average_weights()).astype(np.float64)
    # a new optimizer object: its slot is created at ITS first step, from the weights as they are then -- here weights set
    # after compile(), as a load_weights between compile and fit would
    opt2 = pkg.get_optimizer('sgd', 1e-2, average_type='ema')
    m.compile(optimizer=opt2, loss=loss)
    start = [w * np.float32(0.9) for w in m.get_weights()]
    m.set_weights(start)
    m.train_on_batch(x, y)
    ws, av = _flat(m.get_weights()), _flat(m.get_average_weights())
    ref = R.ema_step(_flat(start), ws, 0.99, active=mask)
    bound = _bound(1, ws, av)
    assert float(np.abs(av - ref).max()) <= bound
    stale = R.ema_step(old_slot, ws, 0.99, active=mask)
    assert float(np.abs(av - stale).max()) > 1e3 * bound               # (the old slot would be told apart)
    # the same object again (train.py:224 after unfreezing): the average continues
    m.compile(optimizer=opt2, loss=loss)
    m.train_on_batch(x, y)
    ws2, av2 = _flat(m.get_weights()), _flat(m.get_average_weights())
    ref2 = R.ema_step(av, ws2, 0.99, active=mask)
    assert float(np.abs(av2 - ref2).max()) <= _bound(1, ws2, av2)
    assert float(np.abs(av2 - R.ema_step(ws, ws2, 0.99, active=mask)).max()) > 10 * _bound(1, ws2, av2)
    # a plain optimizer has no slot
    m.compile(optimizer=pkg.SGD(0.01), loss=loss)
    assert m._store.A is None
    with pytest.raises(RuntimeError, match='does not average'):
        m.get_average_weights()


def test_assign_average_vars_and_predict_follow_the_averages():
    pkg = load_pkg()
    m = _model(pkg.get_optimizer('sgd', 1e-2, average_type='ema'))
    x, y = _data()
    xp, _ = _data(5)
    mask = _slot_mask(m)
    for _ in range(3):
        m.train_on_batch(x, y)
    before, av = _flat(m.get_weights()), _flat(m.get_average_weights())
    p_before = m.predict(xp)
    m.assign_average_vars()
    after = m.get_weights()
    assert np.array_equal(_flat(after), _flat(m.get_average_weights()))
    assert np.array_equal(_flat(after)[mask], av[mask]) and not np.array_equal(av[mask], before[mask])
    # entries without a slot (BatchNorm moving statistics) are not assigned: tfa has no average for them
    assert np.array_equal(_flat(after)[~mask], before[~mask])
    p = m.predict(xp)
    fresh = _model(None)
    fresh.set_weights(after)
    assert float(np.abs(p - fresh.predict(xp)).max()) <= TOL
    assert not np.array_equal(p, p_before)


@pytest.mark.parametrize('update_weights', [False, True])
def test_average_model_checkpoint_in_fit(tmp_path, update_weights):
    """two epochs of two steps: the file of the last epoch holds the averages; the model keeps its own weights with
    update_weights=False (bitwise those of the same run without the callback) and takes the averages with True"""
    pkg = load_pkg()
    batches = [_data(1), _data(2)]

    def run(callbacks):
        m = _model(pkg.get_optimizer('sgd', 1e-2, average_type='ema'))
        m.fit(batches, steps_per_epoch=2, epochs=2, verbose=0, callbacks=callbacks)
        return m

    cb = pkg.AverageModelCheckpoint(str(tmp_path / 'ep{epoch:03d}-loss{loss:.3f}.h5'), update_weights=update_weights,
                                    monitor='loss', mode='min', save_best_only=False, period=1)
    m = run([cb])
    assert len(cb.saved) == 2 and cb.saved[0] != cb.saved[1] and '/ep002-loss' in cb.saved[1].replace('\\', '/')
    mask = _slot_mask(m)
    ws, av = _flat(m.get_weights()), _flat(m.get_average_weights())
    fresh = _model(None)
    fresh.load_weights(cb.saved[1])
    saved = _flat(fresh.get_weights())
    assert np.array_equal(saved, av)
    if update_weights:
        assert np.array_equal(ws, av)
    else:
        twin = run([])
        assert np.array_equal(ws, _flat(twin.get_weights()))
        assert np.array_equal(av[mask], _flat(twin.get_average_weights())[mask])
        assert not np.array_equal(ws[mask], av[mask])
