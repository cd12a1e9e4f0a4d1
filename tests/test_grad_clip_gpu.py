"""Gradient clipping on the device (csrc/grad_clip.hip): the three dl3p_grad_clip_* passes against the float64 restatement of the
rules (tests/clip_rules.py), then clipvalue / clipnorm / global_clipnorm through compile / train_on_batch / graph replay.

Op level, for each rule and each combination, at grad_scale 1 and 1/8 (powers of two: the oracle's g' is then bit-exact):
  norm   1e-12 relative: both sides sum exact float64 squares, only the order differs (<= ~40 additions deep on the device,
         pairwise in NumPy: a few 1e-16 each);
  scale  2^-23 relative: one float32 rounding of a float64 quotient on each side;
  g      2 ulp of float32(g') * scale: the scale's rounding and the product's;
  frozen elements bit-identical, two runs bit-identical, scale == 1.0 exactly under the threshold.
Model level: mobilenetv2_lite at 65 x 65, batch 2, dropout off; the bound of one SGD step (momentum 0, lr = 2^-6 exactly) is four
float32 roundings -- the scale, the product, lr * g, and the update: 4 * 2^-24 * lr * max|g'_v| + ulp(w)."""
import numpy as np
import pytest
import torch

import clip_rules as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ------------------------------------------------------------------------------------------------------------ op level
# name, length: every size of the issue, an entirely frozen variable, one with an all-zero gradient, one with a frozen range inside,
# and the two sides of the block count at which the finalize kernel hands a variable from one lane to a whole wave (16 blocks of 4096)
SIZES = [('v4', 4), ('v8', 8), ('v20', 20), ('v1028', 1028), ('big', 300004), ('frozen', 64), ('zero', 128), ('holes', 2048),
         ('b16', 16 * 4096), ('b17', 16 * 4096 + 4)]
WITH_L2 = {'v8': 2e-5, 'v1028': 1e-2, 'big': 2e-5, 'holes': 0.25}


class _Flat:
    def __init__(self):
        ops = load_pkg('ops')
        rng = np.random.default_rng(20)
        self.names = [n for n, _ in SIZES]
        self.ranges, off = [], 0
        for _, n in SIZES:
            self.ranges.append((off, n))
            off += n
        self.total = off
        self.g = (rng.standard_normal(off) * 10.0 ** rng.uniform(-4, 1, off)).astype(np.float32)
        self.w = rng.standard_normal(off).astype(np.float32)
        self.l2 = np.zeros(off, np.float32)
        self.on = np.ones(off, bool)
        for (o, n), name in zip(self.ranges, self.names):
            self.l2[o:o + n] = WITH_L2.get(name, 0.0)
            if name == 'frozen':
                self.on[o:o + n] = False
            if name == 'zero':
                self.g[o:o + n] = 0.0
            if name == 'holes':
                self.on[o + 101:o + 614] = False                  # starts and ends inside a 16-byte group
            if name == 'big':
                self.on[o + 4090:o + 4103] = False                # across the edge of the first block
                self.on[o + 8192:o + 8192 + 4096] = False         # a whole block
        self.g[~self.on] = rng.standard_normal(int((~self.on).sum())).astype(np.float32) * 1e3     # must never be read into a norm
        self.map = ops.GradClipMap(self.ranges, DEV)
        t = lambda a: torch.from_numpy(a).to(DEV)
        self.w_d, self.l2_d, self.on_d = t(self.w), t(self.l2), t(self.on.astype(np.float32))
        self._oracle = {}

    def split(self, a):
        return [a[o:o + n] for o, n in self.ranges]

    def gp(self, grad_scale, g=None):
        return R.loss_gradient(self.g if g is None else g, self.w, self.l2, grad_scale)

    def oracle(self, grad_scale, **rule):
        key = (grad_scale,) + tuple(sorted(rule.items()))
        if key not in self._oracle:
            self._oracle[key] = R.clip(self.split(self.gp(grad_scale)), self.split(self.on), **rule)
        return self._oracle[key]

    def run(self, ops, grad_scale, g=None, clipvalue=None, clipnorm=None, global_clipnorm=None):
        """-> (finished g, partials, scale, norm) as host arrays"""
        g_d = torch.from_numpy(self.g if g is None else g).to(DEV)
        kw = dict(grad_scale=grad_scale, clip_value=clipvalue or 0.0, l2_elem=self.l2_d, lr_scale_elem=self.on_d)
        m = self.map
        m.partials.fill_(-1.0)
        m.scale.fill_(-1.0)
        m.norm.fill_(-1.0)
        if clipnorm is None and global_clipnorm is None:
            ops.grad_clip_apply(g_d, self.w_d, m, scaled=False, partials=True, **kw)
        else:
            ops.grad_clip_sumsq(g_d, self.w_d, m, **kw)
            ops.grad_clip_finalize(m, 1 if clipnorm is not None else 2, clipnorm if clipnorm is not None else global_clipnorm)
            ops.grad_clip_apply(g_d, self.w_d, m, **kw)
        torch.cuda.synchronize()
        return g_d.cpu().numpy(), m.partials.cpu().numpy().copy(), m.scale.cpu().numpy().copy(), m.norm.cpu().numpy().copy()


@pytest.fixture(scope='module')
def flat(ops):
    return _Flat()


def _thresholds(flat, grad_scale):
    """inputs of the cases, from the unclipped oracle: a clamp at the median |g'|, a per-variable threshold between the variables'
    norms, a global threshold at half the global norm"""
    gp = flat.gp(grad_scale)
    base = flat.oracle(grad_scale)
    cv = float(np.float32(np.median(np.abs(gp[flat.on]))))
    per = np.sort(base['norm'][:-1][base['norm'][:-1] > 0])
    return cv, float(per[len(per) // 2] * 0.75), float(base['norm'][-1] * 0.5)


def _rules(flat, grad_scale):
    cv, cn, gn = _thresholds(flat, grad_scale)
    out = {'value': dict(clipvalue=cv), 'norm': dict(clipnorm=cn), 'global': dict(global_clipnorm=gn)}
    # combined with the clamp the norms shrink: thresholds from the clamped oracle, so that the norm rules still bite
    clamped = flat.oracle(grad_scale, clipvalue=cv)
    per = np.sort(clamped['norm'][:-1][clamped['norm'][:-1] > 0])
    out['value+norm'] = dict(clipvalue=cv, clipnorm=float(per[len(per) // 2] * 0.75))
    out['value+global'] = dict(clipvalue=cv, global_clipnorm=float(clamped['norm'][-1] * 0.5))
    return out


def _ulp(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _check(flat, got, ref, rule, g_in):
    g_out, partials, scale, norm = got
    nv = len(flat.ranges)
    has_norm = 'clipnorm' in rule or 'global_clipnorm' in rule
    if has_norm:
        print('norm rel err', np.max(np.abs(norm - ref['norm']) / np.maximum(ref['norm'], 1e-300)))
        assert np.all(np.abs(norm - ref['norm']) <= 1e-12 * ref['norm']), (norm, ref['norm'])
        print('scale', scale, ref['scale'])
        assert np.all(np.abs(scale.astype(np.float64) - ref['scale']) <= 2.0 ** -23 * ref['scale'])
    else:
        gn = np.sqrt(np.sum(partials[:flat.map.nblocks]))
        assert abs(gn - ref['norm'][-1]) <= 1e-12 * ref['norm'][-1]
    worst = 0.0
    for (o, n), on, prod in zip(flat.ranges, flat.split(flat.on), ref['product']):
        d = np.abs(g_out[o:o + n].astype(np.float64) - prod)[on]
        if d.size:
            worst = max(worst, float(np.max(d / _ulp(prod[on]))))
            assert np.all(d <= 2 * _ulp(prod[on]))
    print('worst g error in ulp', worst)
    assert np.array_equal(g_out[~flat.on].view(np.int32), g_in[~flat.on].view(np.int32)), 'a frozen element was written'
    return nv


@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
@pytest.mark.parametrize('name', ['value', 'norm', 'global', 'value+norm', 'value+global'])
def test_rules_against_the_oracle(ops, flat, name, grad_scale):
    rule = _rules(flat, grad_scale)[name]
    ref = flat.oracle(grad_scale, **rule)
    got = flat.run(ops, grad_scale, **rule)
    _check(flat, got, ref, rule, flat.g)
    if 'clipnorm' in rule:
        s = ref['scale']
        assert (s < 1).any() and (s == 1).any(), 'the per-variable threshold should clip some variables and spare others'
        z, f = flat.names.index('zero'), flat.names.index('frozen')
        assert got[3][z] == 0.0 and got[2][z] == 1.0 and got[3][f] == 0.0 and got[2][f] == 1.0       # norm 0: s = 1, not NaN
    if 'global_clipnorm' in rule:
        assert np.all(got[2] == got[2][0]) and got[2][0] < 1
    if 'clipvalue' in rule:
        assert any(np.any(c != g) for c, g in zip(ref['clipped'], flat.split(flat.gp(grad_scale))))
    again = flat.run(ops, grad_scale, **rule)
    for a, b, what in zip(got, again, ('g', 'partials', 'scale', 'norm')):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), 'two runs differ in ' + what


@pytest.mark.parametrize('mode', ['norm', 'global'])
def test_threshold_above_every_norm_is_scale_one_exactly(ops, flat, mode):
    top = float(flat.oracle(1.0)['norm'][-1])
    rule = {'clipnorm' if mode == 'norm' else 'global_clipnorm': top * 1.0000001}
    g_out, _, scale, norm = flat.run(ops, 1.0, **rule)
    assert np.all(scale == np.float32(1.0))
    gp = flat.gp(1.0)
    assert np.array_equal(g_out[flat.on].view(np.int32), gp[flat.on].view(np.int32))       # g' itself, bit for bit
    assert np.array_equal(g_out[~flat.on].view(np.int32), flat.g[~flat.on].view(np.int32))
    # ... and the norm exactly at the threshold still is: s = c / max(norm, c)
    rule = {k: float(norm[-1] if mode == 'global' else norm[:-1].max()) for k in rule}
    assert np.all(flat.run(ops, 1.0, **rule)[2] == np.float32(1.0))


def test_one_infinite_gradient_element(ops, flat):
    g = flat.g.copy()
    o, n = flat.ranges[flat.names.index('v1028')]
    g[o + 7] = np.inf
    cn = _thresholds(flat, 1.0)[1]
    ref_split = flat.split(flat.gp(1.0, g))
    # global: every scale NaN
    g_out, _, scale, norm = flat.run(ops, 1.0, g=g, global_clipnorm=1.0)
    assert np.all(np.isnan(scale)) and np.isinf(norm[-1])
    assert np.all(np.isnan(g_out[flat.on])) and np.array_equal(g_out[~flat.on].view(np.int32), g[~flat.on].view(np.int32))
    # per variable: scale 0 for that variable, its infinite element NaN, the others as without the infinity
    g_out, _, scale, norm = flat.run(ops, 1.0, g=g, clipnorm=cn)
    v = flat.names.index('v1028')
    assert scale[v] == 0.0 and np.isinf(norm[v]) and np.isinf(norm[-1])
    assert np.isnan(g_out[o + 7]) and np.all(np.delete(g_out[o:o + n], 7) == 0.0)
    clean = flat.run(ops, 1.0, clipnorm=cn)
    keep = np.ones(flat.total, bool)
    keep[o:o + n] = False
    assert np.array_equal(g_out[keep].view(np.int32), clean[0][keep].view(np.int32))
    assert np.array_equal(np.delete(scale, v).view(np.int32), np.delete(clean[2], v).view(np.int32))
    ref = R.clip(ref_split, flat.split(flat.on), clipnorm=cn)
    assert ref['scale'][v] == 0.0 and np.isnan(ref['product'][v][7])                         # the oracle agrees


# ------------------------------------------------------------------------------------------------------------ model level
N, H, W, C = 2, 65, 65, 21
LR = 2.0 ** -6


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
    for op in m.graph.ops:                                   # dropout off
        if op.kind == 'materialize' and op.rate > 0:
            op.rate = 0.0
    m.compile(optimizer=optimizer, loss=pkg.SparseCategoricalCrossEntropy(ignore_index=255))
    return m


def _launches(m):
    return [l[0] for l in m._executor(N, True).opt.labels]


class _Twin:
    """one unclipped SGD (momentum 0) step: the weights before it, the raw gradient it left in store.G, the regulariser table
    and the freeze mask, per variable, on the host -- what the clipped steps are predicted from"""

    def __init__(self, freeze_level=0):
        pkg = load_pkg()
        m = _model(pkg.SGD(LR, momentum=0.0), freeze_level)
        st = m._ensure_store()
        self.w0 = st.P.cpu().numpy().copy()
        m.train_on_batch(*_data())
        torch.cuda.synchronize()
        self.launches = _launches(m)
        self.g = st.G.cpu().numpy().copy()
        self.w1 = st.P.cpu().numpy().copy()
        self.l2 = st.l2.cpu().numpy().copy()
        self.on = st.lr_scale.cpu().numpy() != 0
        self.ranges = [(st.offset[p], (p.dev_size + 3) // 4 * 4) for p in st.params]
        self.trainable = [bool(self.on[o:o + n].any()) for o, n in self.ranges]
        self.gp = R.loss_gradient(self.g, self.w0, self.l2, 1.0)

    def split(self, a):
        return [a[o:o + n] for o, n in self.ranges]

    def clip(self, **rule):
        return R.clip(self.split(self.gp), self.split(self.on), **rule)

    def check_step(self, m, ref):
        """the clipped model's weights after ITS first step against w0 - lr * clip(g')"""
        st = m._store
        w = st.P.cpu().numpy()
        worst = 0.0
        for (o, n), on, prod, gpv in zip(self.ranges, self.split(self.on), ref['product'], self.split(self.gp)):
            if not on.any():          # (BatchNorm moving statistics move with the forward pass: as in the unclipped step)
                assert np.array_equal(w[o:o + n], self.w1[o:o + n])
                continue
            want = self.w0[o:o + n].astype(np.float64) - LR * prod
            bound = 4 * 2.0 ** -24 * LR * float(np.abs(gpv[on]).max()) + _ulp(np.maximum(np.abs(self.w0[o:o + n]), np.abs(w[o:o + n])))
            err = np.abs(w[o:o + n] - want)
            worst = max(worst, float(np.max((err / bound)[on])))
            assert np.all(err[on] <= bound[on]), (o, n, float(np.max((err / bound)[on])))
            assert np.array_equal(w[o:o + n][~on], self.w1[o:o + n][~on])
        print('worst step error / bound', worst)


@pytest.fixture(scope='module')
def twin():
    return _Twin()


def test_huge_global_clipnorm_changes_no_bit_over_eager_capture_and_replay(twin):
    """the regulariser fold and the grad_scale = 1 hand-over: with a threshold nothing reaches, three steps leave the weights of
    the unclipped run; the plan has exactly the three launches more"""
    pkg = load_pkg()
    plain, clipped = _model(pkg.SGD(LR)), _model(pkg.SGD(LR, global_clipnorm=1e30))
    x, y = _data()
    for t in range(3):
        plain.train_on_batch(x, y)
        clipped.train_on_batch(x, y)
        assert torch.equal(plain._store.P, clipped._store.P), t
        assert torch.equal(plain._store.V, clipped._store.V), t
    assert clipped._executor(N, True).graphed and plain._executor(N, True).graphed
    assert np.isfinite(clipped.last_grad_norm) and clipped.last_grad_norm > 0 and plain.last_grad_norm is None
    lp, lc = _launches(plain), _launches(clipped)
    assert lp == twin.launches
    assert lc == ['dl3p_grad_clip_sumsq', 'dl3p_grad_clip_finalize', 'dl3p_grad_clip_apply'] + lp


def test_clipnorm_below_every_variable_norm_scales_every_variable(twin):
    pkg = load_pkg()
    base = twin.clip()
    norms = np.array([n for n, tr in zip(base['norm'][:-1], twin.trainable) if tr])
    assert norms.min() > 0
    c = float(norms.min() * 0.5)
    ref = twin.clip(clipnorm=c)
    assert all(s < 1 for s, tr in zip(ref['scale'], twin.trainable) if tr)
    m = _model(pkg.SGD(LR, momentum=0.0, clipnorm=c))
    m.train_on_batch(*_data())
    twin.check_step(m, ref)
    assert abs(m.last_grad_norm - base['norm'][-1]) <= 1e-6 * base['norm'][-1]
    assert not np.array_equal(m._store.P.cpu().numpy(), twin.w1)


@pytest.mark.parametrize('rule', ['global_clipnorm', 'clipvalue'])
def test_global_clipnorm_and_clipvalue_steps_and_the_reported_norm(twin, rule):
    pkg = load_pkg()
    if rule == 'global_clipnorm':
        kw = dict(global_clipnorm=float(twin.clip()['norm'][-1] * 0.5))
    else:
        kw = dict(clipvalue=float(np.float32(np.median(np.abs(twin.gp[twin.on])))))
    ref = twin.clip(**kw)
    m = _model(pkg.SGD(LR, momentum=0.0, **kw))
    m.train_on_batch(*_data())
    twin.check_step(m, ref)
    # the norm the rules saw: of the whole-loss gradient, after the clamp, before any norm scaling
    assert abs(m.last_grad_norm - ref['norm'][-1]) <= 1e-6 * ref['norm'][-1], (m.last_grad_norm, ref['norm'][-1])
    assert not np.array_equal(m._store.P.cpu().numpy(), twin.w1)
    extra = ['dl3p_grad_clip_sumsq', 'dl3p_grad_clip_finalize', 'dl3p_grad_clip_apply'] if rule == 'global_clipnorm' else ['dl3p_grad_clip_apply']
    assert _launches(m) == extra + twin.launches


def test_lookahead_over_adam_with_global_clipnorm_under_mixed_bfloat16():
    """six steps (the sync of Lookahead is the sixth): finite, every bf16 mirror made from the synced weights, and the run with
    capture and replays equal to the all-eager run bit for bit"""
    pkg = load_pkg()
    x, y = _data()
    c = 0.1
    runs = []
    for graphs in (False, True):
        m = _model(pkg.get_optimizer('adam', 1e-3, average_type='lookahead', global_clipnorm=c), bf16=True)
        m.use_graphs = graphs
        norms = []
        for t in range(6):
            assert np.isfinite(m.train_on_batch(x, y))
            norms.append(m.last_grad_norm)
        assert m._executor(N, True).graphed == graphs
        runs.append((m, norms))
    (eager, n_e), (replayed, n_r) = runs
    assert np.all(np.isfinite(n_e)) and min(n_e) > c, 'the threshold should clip every step of this test'
    assert n_e == n_r
    st = replayed._store
    assert torch.equal(eager._store.P, st.P) and torch.equal(eager._store.A, st.A) and torch.equal(eager._store.V, st.V)
    assert bool(torch.isfinite(st.P).all())
    on = st.lr_scale != 0
    assert torch.equal(st.P[on], st.A[on]), 'step 6 is a Lookahead sync: the weights are the slow weights'
    left = {'Pb': st.Pb.clone(), 'Pbt': st.Pbt.clone()}
    st.transpose()
    torch.cuda.synchronize()
    assert torch.equal(left['Pb'], st.Pb) and torch.equal(left['Pbt'], st.Pbt), 'a mirror was not made from the synced weights'


def test_freeze_level_1_the_backbone_gradient_is_untouched_and_enters_no_norm():
    pkg = load_pkg()
    tw = _Twin(freeze_level=1)
    assert 0 < sum(tw.trainable) < len(tw.trainable)
    base = tw.clip()
    host = float(np.sqrt(np.sum(tw.gp[tw.on].astype(np.float64) ** 2)))
    assert abs(base['norm'][-1] - host) <= 1e-12 * host
    c = host * 0.25
    m = _model(pkg.SGD(LR, momentum=0.0, global_clipnorm=c), freeze_level=1)
    m.train_on_batch(*_data())
    g = m._store.G.cpu().numpy()
    assert np.array_equal(g[~tw.on].view(np.int32), tw.g[~tw.on].view(np.int32)), 'a frozen gradient entry was written'
    assert abs(m.last_grad_norm - host) <= 1e-6 * host
    ref = tw.clip(global_clipnorm=c)
    prod = np.concatenate(ref['product'])
    flat_on = np.concatenate(tw.split(tw.on))
    got = np.concatenate(tw.split(g))
    assert np.all(np.abs(got - prod)[flat_on] <= 2 * _ulp(prod[flat_on]))
    tw.check_step(m, ref)
