"""Gradient clipping (clipvalue, clipnorm, global_clipnorm) without a device: the optimiser keywords of
common/model_utils.py:117-123, their validation, the delegation through the averaged wrappers, the launches the optimiser plan
gains, the argument checks of the dl3p_grad_clip_* entry points, and the NumPy restatement (tests/clip_rules.py) against
torch.nn.utils where the two definitions coincide."""
import types

import numpy as np
import pytest
import torch

import clip_rules as R
from conftest import load_pkg


# ------------------------------------------------------------------------------------------------------------ keywords
def test_the_reference_constructor_lines_work_verbatim():
    """common/model_utils.py:119, :121, :123 with our classes in place of the Keras ones"""
    pkg = load_pkg()
    Adam, RMSprop, SGD = pkg.Adam, pkg.RMSprop, pkg.SGD
    lr_scheduler = 0.01
    optimizer = Adam(learning_rate=lr_scheduler, epsilon=1e-7, amsgrad=False, clipnorm=None, clipvalue=None)
    assert optimizer.clip_spec() is None
    optimizer = RMSprop(learning_rate=lr_scheduler, rho=0.9, momentum=0.0, centered=False, clipnorm=None, clipvalue=None)
    assert optimizer.clip_spec() is None
    optimizer = SGD(learning_rate=lr_scheduler, momentum=0.9, nesterov=False, clipnorm=None, clipvalue=None)
    assert optimizer.clip_spec() is None


@pytest.mark.parametrize('cls', ['SGD', 'Adam', 'RMSprop'])
def test_validation(cls):
    ctor = getattr(load_pkg(), cls)
    with pytest.raises(ValueError, match='both'):
        ctor(0.01, clipnorm=1.0, global_clipnorm=1.0)
    for key in ('clipnorm', 'clipvalue', 'global_clipnorm'):
        for bad in (0, 0.0, -1.0, float('nan'), float('inf'), -float('inf'), 'one'):
            with pytest.raises(ValueError, match=key):
                ctor(0.01, **{key: bad})
    assert ctor(0.01, clipvalue=0.5).clip_spec() == (0.5, None, None)
    assert ctor(0.01, clipnorm=2).clip_spec() == (None, 2.0, None)
    assert ctor(0.01, global_clipnorm=3.0, clipvalue=1e-3).clip_spec() == (1e-3, None, 3.0)
    assert ctor(0.01, clipnorm=1.0, clipvalue=0.25).clip_spec() == (0.25, 1.0, None)


def test_spec_is_unchanged_and_clip_spec_goes_through_the_wrappers():
    pkg = load_pkg()
    assert pkg.SGD(0.01, clipnorm=1.0).spec() == pkg.SGD(0.01).spec() == ('sgd', 0.9)
    assert pkg.Adam(0.01, clipvalue=1.0).spec() == pkg.Adam(0.01).spec() == ('adam', 0.9, 0.999, 1e-7)
    assert pkg.RMSprop(0.01, global_clipnorm=1.0).spec() == pkg.RMSprop(0.01).spec() == ('rmsprop', 0.9, 1e-7)
    for wrap in (pkg.MovingAverage, pkg.SWA, pkg.Lookahead):
        assert wrap(pkg.Adam(0.01, global_clipnorm=5.0)).clip_spec() == (None, None, 5.0)
        assert wrap(pkg.SGD(0.01)).clip_spec() is None
    for base in ('sgd', 'adam', 'rmsprop'):
        assert pkg.get_optimizer(base, 1e-2).clip_spec() is None
        assert pkg.get_optimizer(base, 1e-2, clipnorm=1.0, clipvalue=0.5).clip_spec() == (0.5, 1.0, None)
        for avg in ('ema', 'swa', 'lookahead'):
            o = pkg.get_optimizer(base, 1e-2, average_type=avg, decay_type='cosine', global_clipnorm=2.0)
            assert o.clip_spec() == (None, None, 2.0) and o.spec() == pkg.get_optimizer(base, 1e-2).spec()
    with pytest.raises(TypeError):
        pkg.get_optimizer('sgd', 1e-2, None, None, 1000, 1.0)          # the clipping arguments are keyword-only
    with pytest.raises(ValueError, match='both'):
        pkg.get_optimizer('sgd', 1e-2, clipnorm=1.0, global_clipnorm=1.0)


def test_compile_hands_the_spec_to_the_executor_key():
    pkg = load_pkg()
    m = pkg.get_deeplabv3p_model('mobilenetv2_lite', 21, (65, 65), 16)
    m.compile(optimizer=pkg.SGD(0.01))
    assert m._clip_spec() is None and m.last_grad_norm is None
    m.compile(optimizer=pkg.Lookahead(pkg.Adam(1e-3, global_clipnorm=1.0)))
    assert m._clip_spec() == (None, None, 1.0) and m.last_grad_norm is None


# ------------------------------------------------------------------------------------------------------------ the plan
class _Recorder:
    """stands in for the library while Executor._trace_sgd runs: every entry point records its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
        fn.__name__ = 'dl3p_' + name
        return fn


class _Param:
    def __init__(self, dev_size):
        self.dev_size = dev_size


def _trace_optimizer_plan(monkeypatch, optimizer, clip, averaging=None, world=1):
    """Executor._trace_sgd on host tensors with a recording library: [(entry point, args)] of the optimiser plan"""
    E = load_pkg('executor')
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda: types.SimpleNamespace(cuda_stream=0))
    sizes = [32, 6, 4096 * 3 + 8, 16]
    params = [_Param(n) for n in sizes]
    offset, total = E.param_offsets(params)
    store = types.SimpleNamespace(params=params, offset=offset, total=total, device=torch.device('cpu'), _clip_map=None,
                                  tr_table=None, Sb=None, opt_step=torch.zeros(1, dtype=torch.int64))
    for name in ('P', 'G', 'V', 'V2', 'A', 'l2', 'lr_scale'):
        setattr(store, name, torch.zeros(total))
    store.clip_map = types.MethodType(E.ParamStore.clip_map, store)
    ex = object.__new__(E.Executor)
    ex.L, ex.store, ex.optimizer, ex.averaging, ex.clip = _Recorder(), store, optimizer, averaging, clip
    ex.momentum = optimizer[1] if optimizer[0] == 'sgd' else 0.0
    ex.dist = types.SimpleNamespace(world_size=world) if world > 1 else None
    ex.bf16, ex.lr, ex.g, ex.dev = False, torch.zeros(1), types.SimpleNamespace(ops=[]), store.device
    plan = ex._trace_sgd()
    assert [l[0] for l in plan.labels] == ['dl3p_' + c[0] for c in ex.L.calls]
    return ex.L.calls, store


OPTS = {'sgd': (('sgd', 0.9), 'sgd_momentum'), 'adam': (('adam', 0.9, 0.999, 1e-7), 'adam_step'),
        'rmsprop': (('rmsprop', 0.9, 1e-7), 'rmsprop_step')}


@pytest.mark.parametrize('avg', [None, (1, 0.99, 1, 0)], ids=['plain', 'ema'])
@pytest.mark.parametrize('opt', sorted(OPTS))
def test_optimizer_plan_gains_three_launches_one_or_none(monkeypatch, opt, avg):
    E = load_pkg('executor')
    spec, entry = OPTS[opt]
    entry += '_avg' if avg else ''
    base, store = _trace_optimizer_plan(monkeypatch, spec, None, avg, world=8)
    assert [c[0] for c in base] == [entry]                               # as before: the optimiser launch alone
    args = base[0][1]
    assert 0.125 in args and store.l2.data_ptr() in args                 # grad_scale = 1 / world, the l2 table
    assert E.clip_launches(None) == ()
    for clip, extra in (((None, None, 2.0), 3), ((0.5, 1.0, None), 3), ((0.5, None, None), 1)):
        calls, store = _trace_optimizer_plan(monkeypatch, spec, clip, avg, world=8)
        names = [c[0] for c in calls]
        assert names == list(E.clip_launches(clip)) + [entry] and len(names) == 1 + extra
        # the optimiser launch takes the finished gradient: grad_scale 1, no l2 table, every other number as before (the two
        # traces have buffers of their own, so addresses are not compared)
        got = calls[-1][1]
        assert len(got) == len(args)
        for a, b in zip(args, got):
            if a == 0.125:
                assert b == 1.0
            elif isinstance(a, float) or a is None:
                assert a == b
        assert store.l2.data_ptr() not in got and got.count(None) == args.count(None) + 1
        # the clip launches read the regulariser and 1 / world themselves, on G in place
        for name, cargs in calls[:-1]:
            if name != 'grad_clip_finalize':
                assert cargs[0] == store.G.data_ptr() and cargs[1] == store.P.data_ptr() and cargs[2] == store.l2.data_ptr()
                assert cargs[3] == store.lr_scale.data_ptr() and cargs[4] == store.total and cargs[5] == 0.125
                assert cargs[6] == (clip[0] or 0.0)
        if extra == 3:
            mode, threshold = calls[1][1][5], calls[1][1][6]
            assert (mode, threshold) == ((1, clip[1]) if clip[1] is not None else (2, clip[2]))
            assert calls[2][1][7] == store.clip_map().scale.data_ptr() and calls[2][1][-2] is None
        else:
            assert calls[0][1][7] is None and calls[0][1][-2] == store.clip_map().partials.data_ptr()      # ([-1]: the stream)


def test_clip_map_covers_every_variable_once():
    ops = load_pkg('ops')
    per = ops.lib().grad_clip_block_elements()
    assert per == 4096
    m = ops.GradClipMap([(0, 32), (32, 8), (40, 3 * per + 8), (40 + 3 * per + 8, 16)], 'cpu')
    assert m.nvars == 4 and m.nblocks == 1 + 1 + 4 + 1
    assert m.vars_host.tolist() == [[0, 32, 0], [32, 8, 1], [40, 3 * per + 8, 2], [40 + 3 * per + 8, 16, 6]]
    assert m.blockmap_host.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [2, 3], [3, 0]]
    assert m.partials.dtype == torch.float64 and m.norm.numel() == 5 and m.scale.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_refuse_bad_arguments_without_a_device():
    libm = load_pkg('_lib')
    L = libm.lib()
    per = L.grad_clip_block_elements()
    n = 2 * per + 64
    bufs = [np.zeros(n + 4, np.float32) for _ in range(4)]
    g, w, l2, lr = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]            # aligned host addresses, never dereferenced
    part = np.zeros(8, np.float64).ctypes.data
    scale = np.zeros(8, np.float32).ctypes.data
    norm = np.zeros(8, np.float64).ctypes.data

    def tables(vars_, blocks):
        v = np.array(vars_, np.int64).reshape(-1, 3)
        b = np.array(blocks, np.int32).reshape(-1, 2)
        return v, b

    good_v, good_b = tables([[0, 32, 0], [32, per + 32, 1]], [[0, 0], [1, 0], [1, 1]])
    keep = []

    def sumsq(g=g, w=w, l2=l2, lr=lr, n=n, gs=1.0, cv=0.0, v=good_v, b=good_b, nvars=None, part=part, vdev=1):
        keep.extend([v, b])
        vp, bp = (v.ctypes.data if v is not None else None), (b.ctypes.data if b is not None else None)
        return ('grad_clip_sumsq', (g, w, l2, lr, n, gs, cv, vp if vdev else None, vp, len(v) if nvars is None else nvars,
                                    bp, bp, len(b) if b is not None else 0, part, None))

    def apply(g=g, w=w, l2=l2, lr=lr, n=n, gs=1.0, cv=0.5, scale=scale, v=good_v, b=good_b, part=None):
        keep.extend([v, b])
        return ('grad_clip_apply', (g, w, l2, lr, n, gs, cv, scale, v.ctypes.data, v.ctypes.data, len(v), b.ctypes.data,
                                    b.ctypes.data, len(b), part, None))

    def finalize(part=part, v=good_v, nvars=None, nblocks=3, mode=2, c=1.0, scale=scale, norm=norm):
        keep.append(v)
        return ('grad_clip_finalize', (part, v.ctypes.data, v.ctypes.data, len(v) if nvars is None else nvars, nblocks, mode, c,
                                       scale, norm, None))

    past_v, past_b = tables([[0, 32, 0], [32, per + 32, 1]], [[0, 0], [1, 0], [1, 2]])        # block 2 of a two-block variable
    over_v, over_b = tables([[0, 32, 0], [32, 2 * per + 64, 1]], [[0, 0], [1, 0], [1, 1], [1, 2]])   # ends 32 floats past n
    odd_v, odd_b = tables([[0, 30, 0]], [[0, 0]])
    gap_v, gap_b = tables([[0, 32, 0], [32, 64, 2]], [[0, 0], [1, 0]])
    many_v = np.zeros((65537, 3), np.int64)
    bad = [('null', sumsq(g=None)), ('null', sumsq(w=None)), ('null', sumsq(part=None)), ('null', sumsq(vdev=0)),
           ('aligned', sumsq(g=g + 4)), ('aligned', sumsq(w=w + 4)), ('aligned', sumsq(l2=l2 + 8)), ('aligned', sumsq(lr=lr + 12)),
           ('clip_value', sumsq(cv=-1.0)), ('clip_value', sumsq(cv=float('inf'))), ('clip_value', sumsq(cv=float('nan'))),
           ('runs past its variable', sumsq(v=past_v, b=past_b)), ('aligned range', sumsq(v=over_v, b=over_b)),
           ('aligned range', sumsq(v=odd_v, b=odd_b)), ('starts at block', sumsq(v=gap_v, b=gap_b)),
           ('blocks', sumsq(b=good_b[:2])), ('nvars', sumsq(v=many_v, nvars=65537)), ('nvars', sumsq(nvars=0)),
           ('null', apply(g=None)), ('aligned', apply(g=g + 4)), ('nothing to apply', apply(scale=None, cv=0.0)),
           ('runs past its variable', apply(v=past_v, b=past_b)), ('aligned range', apply(v=over_v, b=over_b)),
           ('nvars', apply(v=many_v)), ('misaligned', apply(part=part + 4)),
           ('null', finalize(part=None)), ('null', finalize(scale=None)), ('null', finalize(norm=None)),
           ('mode', finalize(mode=0)), ('mode', finalize(mode=3)), ('threshold', finalize(c=0.0)),
           ('threshold', finalize(c=-1.0)), ('threshold', finalize(c=float('nan'))), ('threshold', finalize(c=float('inf'))),
           ('nvars', finalize(v=many_v, nvars=65537)), ('blocks', finalize(nblocks=2)), ('misaligned', finalize(norm=norm + 4))]
    for word, (name, args) in bad:
        fn = getattr(L, name)
        assert fn.raw(*args) == -1, (name, word)                          # DL3P_EINVAL
        with pytest.raises(libm.Dl3pError, match=word):
            fn(*args)


def test_header_declares_the_entry_points():
    protos = load_pkg('_lib').parse_header()
    for name in ('dl3p_grad_clip_sumsq', 'dl3p_grad_clip_finalize', 'dl3p_grad_clip_apply'):
        ret, args = protos[name]
        assert ret == 'int' and args[-1] == 'void*'
    assert protos['dl3p_grad_clip_block_elements'] == ('int', [])
    assert protos['dl3p_grad_clip_finalize'][1][-3:-1] == ['float*', 'double*']


# ------------------------------------------------------------------------------------------------------------ the oracle
def _vars(seed, sizes=(4, 8, 20, 1028, 3001)):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32) for n in sizes]


def test_oracle_global_norm_against_torch():
    """torch.nn.utils.clip_grad_norm_ is c / (norm + 1e-6) clamped at 1 on one global norm: with float64 parameters the two differ
    by the 1e-6 in the denominator (relative 1e-6 / norm) and our single float32 rounding of the scale (2^-24)"""
    gs = _vars(1)
    on = [np.ones(g.shape, bool) for g in gs]
    for c in (1.0, 1e3):
        params = [torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64)) for g in gs]
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.astype(np.float64))
        total = float(torch.nn.utils.clip_grad_norm_(params, c))
        out = R.clip(gs, on, global_clipnorm=c)
        assert abs(out['norm'][-1] - total) <= 1e-14 * total
        assert abs(out['norm'][-1] - np.sqrt(sum(float(n) ** 2 for n in out['norm'][:-1]))) <= 1e-14 * total
        if c > total:
            assert np.all(out['scale'] == np.float32(1.0))
        else:
            assert len(set(out['scale'].tolist())) == 1 and out['scale'][0] < 1
        for p, prod in zip(params, out['product']):
            got = p.grad.numpy()
            assert np.all(np.abs(prod - got) <= (1e-6 / total + 2.0 ** -23) * np.abs(got))


def test_oracle_value_clipping_against_torch():
    gs = _vars(2)
    on = [np.ones(g.shape, bool) for g in gs]
    params = [torch.nn.Parameter(torch.zeros(g.size)) for g in gs]
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_value_(params, 0.05)
    out = R.clip(gs, on, clipvalue=0.05)
    for p, c, prod, g in zip(params, out['clipped'], out['product'], gs):
        assert np.array_equal(c, p.grad.numpy()) and np.array_equal(prod, c.astype(np.float64))
    assert any(np.any(c != g) for c, g in zip(out['clipped'], gs))
    assert np.all(out['scale'] == np.float32(1.0))


def test_oracle_rules_on_known_numbers():
    g = [np.array([3.0, 4.0, 0.0, 0.0], np.float32), np.zeros(4, np.float32), np.array([6.0, 8.0, 1e3, -1e3], np.float32)]
    on = [np.ones(4, bool), np.ones(4, bool), np.array([True, True, False, False])]
    out = R.clip(g, on, clipnorm=5.0)
    assert out['norm'].tolist() == [5.0, 0.0, 10.0, np.sqrt(125.0)] and out['scale'].tolist() == [1.0, 1.0, 0.5]
    out = R.clip(g, on, global_clipnorm=1.0)
    assert np.all(out['scale'] == np.float32(1.0 / np.sqrt(125.0)))
    out = R.clip(g, on, clipvalue=3.5, clipnorm=1.0)                    # the clamp comes first: (3, 3.5) and (3.5, 3.5)
    assert out['norm'][0] == np.sqrt(9 + 3.5 ** 2) and out['norm'][2] == np.sqrt(2 * 3.5 ** 2)
    bad = [np.array([1.0, np.inf, 0, 0], np.float32), np.ones(4, np.float32)]
    on2 = [np.ones(4, bool)] * 2
    out = R.clip(bad, on2, clipnorm=1.0)
    assert out['scale'][0] == 0 and out['scale'][1] == np.float32(0.5) and np.isnan(out['product'][0][1]) and out['product'][0][0] == 0
    out = R.clip(bad, on2, global_clipnorm=1.0)
    assert np.all(np.isnan(out['scale']))
    gp = R.loss_gradient(np.array([1.0], np.float32), np.array([0.5], np.float32), np.array([0.25], np.float32), 0.125)
    assert gp.dtype == np.float32 and gp[0] == 0.125 + 0.25
