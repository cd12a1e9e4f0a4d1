"""The dense-CRF kernels of csrc/crf.hip per element at their launch and parameter edges, against the float64 pieces and the bounds of
tests/crf_rules.py (tests/test_crf_rules_cpu.py holds those bounds to honest float32 arithmetic and to the planted mistakes first).

Entry points are called through the C ABI where ops.py does not expose an argument (strides, scale, tmp, norm_out, ldq).  Every output
lies in a buffer filled with a sentinel, with a guard band behind it; strided outputs keep the sentinel in the columns beside the 32.
Each test prints the largest error-to-bound ratio of its family."""
import numpy as np
import pytest
import torch

import crf_rules
from conftest import load_pkg

pytestmark = pytest.mark.gpu
LP = crf_rules.LP
SENTINEL = -7.25
GUARD = 256
LDV, LDO, LDQ = 40, 48, 40
COLS = list(crf_rules.PRESENT_COLUMNS)
ZERO_COLS = [c for c in range(LP) if c not in COLS]
WORST = {}


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the shared inputs are read-only)


def _guarded(elements, dtype=torch.float32, fill=SENTINEL):
    """a flat buffer of `elements` and a guard band, all holding the sentinel"""
    return torch.full((elements + GUARD,), fill, dtype=dtype, device='cuda')


def _guard_is_intact(buf, elements, fill=SENTINEL):
    return bool((buf[elements:] == fill).all())


def _wide(v, ld):
    """v (N, n, 32) float32 -> the first 32 columns of an (N, n, ld) buffer whose other columns hold the sentinel"""
    w = torch.full(v.shape[:2] + (ld,), SENTINEL, dtype=torch.float32, device='cuda')
    w[..., :LP] = _dev(v)
    return w


def _ratio(family, got, want, bound):
    """the largest |got - want| / bound over the elements with a bound; elements with a zero bound are met exactly"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    assert (err[bound == 0] == 0).all()
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def _report(family, what, r):
    print('%s %s: largest error / bound %.3f (family so far %.3f)' % (family, what, r, WORST[family]))


# ------------------------------------------------------------------------------------------------ Gaussian message and normaliser
GAUSS = range(len(crf_rules.GAUSS_SHAPES))
GAUSS_IDS = ['%dx%d' % s[:2] for s in crf_rules.GAUSS_SHAPES]


@pytest.mark.parametrize('k', GAUSS, ids=GAUSS_IDS)
def test_the_gaussian_message_per_element(ops, k):
    """two images, sx != sy, V rows of stride 40 and output rows of stride 48, with and without a scale on pixel j"""
    H, W, sx, sy = crf_rules.GAUSS_SHAPES[k]
    N, n = 2, H * W
    a = crf_rules.gauss_exponents(H, W, (sx, sy))
    v = crf_rules.message_v(300 + k, N, n)
    scale = crf_rules.message_scale(400 + k, n)
    vw = _wide(v, LDV)
    tmp, out = _guarded(N * n * LP), _guarded(N * n * LDO)
    for s in (None, scale):
        tmp.fill_(SENTINEL)
        out.fill_(SENTINEL)
        sd = None if s is None else _dev(s)
        ops.lib().crf_gauss_message(_p(vw), LDV, _p(sd), _p(tmp), _p(out), LDO, N, H, W, sx, sy, _st())
        torch.cuda.synchronize()
        got = out[:N * n * LDO].view(N, n, LDO).cpu().numpy()
        assert (got[..., LP:] == SENTINEL).all() and _guard_is_intact(out, N * n * LDO)       # beside the 32 and behind the buffer
        assert _guard_is_intact(tmp, N * n * LP) and bool((tmp[:N * n * LP] != SENTINEL).all())
        assert bool((vw[..., LP:] == SENTINEL).all())
        for b in range(N):
            want = np.exp(a) @ crf_rules._scaled(v[b], s)
            r = _ratio('gaussian message', got[b][:, COLS], want[:, COLS], crf_rules.message_bound(a, v[b], s)[:, COLS])
            assert not got[b][:, ZERO_COLS].any()                                            # columns of zeros stay exactly 0
            _report('gaussian message', '%s image %d %s' % (GAUSS_IDS[k], b, 'scaled' if s is not None else 'plain'), r)
            assert r <= 1


@pytest.mark.parametrize('k', GAUSS, ids=GAUSS_IDS)
def test_the_gaussian_normaliser_per_element(ops, k):
    H, W, sx, sy = crf_rules.GAUSS_SHAPES[k]
    n = H * W
    buf = _guarded(n)
    ops.lib().crf_gauss_norm(_p(buf), H, W, sx, sy, _st())
    torch.cuda.synchronize()
    assert _guard_is_intact(buf, n)
    r = _ratio('gaussian normaliser', buf[:n].cpu().numpy(), crf_rules.gauss_norm(H, W, (sx, sy)),
               crf_rules.norm_bound(crf_rules.gauss_exponents(H, W, (sx, sy))))
    _report('gaussian normaliser', GAUSS_IDS[k], r)
    assert r <= 1


# ------------------------------------------------------------------------------------------------ bilateral message and normaliser
BIL = range(len(crf_rules.BILATERAL_SHAPES))
BIL_IDS = ['%dx%d' % s for s in crf_rules.BILATERAL_SHAPES]
KINDS = sorted(crf_rules.BILATERAL_KINDS)


def _bilateral(ops, img, v, ldv, scale, out, ldo, norm_out, N, H, W, sxy, srgb):
    ops.lib().crf_bilateral_message(_p(img), _p(v), ldv, _p(scale), _p(out), ldo, _p(norm_out), N, H, W, float(sxy), float(srgb), _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('k', BIL, ids=BIL_IDS)
def test_the_bilateral_message_per_element(ops, k, kind):
    """n around the 128-row tile and the 256-row chunk; two images with a scale of their own each; strides 40 and 48; non-default
    sigmas; an image of two regions 255 apart (k underflows to 0 across them) and one of random bytes: no NaN, every element bound"""
    H, W = crf_rules.BILATERAL_SHAPES[k]
    N, n = 2, H * W
    sxy, srgb = crf_rules.BILATERAL_KINDS[kind]
    img = crf_rules.bilateral_image(kind, 500 + k, N, H, W)
    v = crf_rules.message_v(600 + k, N, n)
    scale = crf_rules.message_scale(700 + k, N, n)
    vw = _wide(v, LDV)
    out = _guarded(N * n * LDO)
    _bilateral(ops, _dev(img), vw, LDV, _dev(scale), out, LDO, None, N, H, W, sxy, srgb)
    got = out[:N * n * LDO].view(N, n, LDO).cpu().numpy()
    assert (got[..., LP:] == SENTINEL).all() and _guard_is_intact(out, N * n * LDO) and bool((vw[..., LP:] == SENTINEL).all())
    for b in range(N):
        a = crf_rules.bilateral_exponents(img[b], sxy, srgb)
        want = np.exp(a) @ crf_rules._scaled(v[b], scale[b])
        r = _ratio('bilateral message', got[b][:, COLS], want[:, COLS], crf_rules.message_bound(a, v[b], scale[b])[:, COLS])
        assert not got[b][:, ZERO_COLS].any()
        _report('bilateral message', '%s %s image %d' % (BIL_IDS[k], kind, b), r)
        assert r <= 1


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('k', BIL, ids=BIL_IDS)
def test_the_bilateral_normaliser_and_the_launches_that_produce_it(ops, k, kind):
    """norm_out alone (the launch of ops.dense_crf), per element; v = NULL with out: column 0 is the row sum and columns 1 .. 31 are
    exactly 0; norm_out together with out on a V whose column 0 is all ones: norm_out is 1 / sqrtf(out[..., 0] + 1e-20f) bit for bit"""
    H, W = crf_rules.BILATERAL_SHAPES[k]
    N, n = 2, H * W
    sxy, srgb = crf_rules.BILATERAL_KINDS[kind]
    img = crf_rules.bilateral_image(kind, 500 + k, N, H, W)
    imgd = _dev(img)
    exps = [crf_rules.bilateral_exponents(img[b], sxy, srgb) for b in range(N)]
    want = np.stack([crf_rules.bilateral_norm(img[b], sxy, srgb) for b in range(N)])
    bound = np.stack([crf_rules.norm_bound(a) for a in exps])
    # norm_out alone
    alone = _guarded(N * n)
    _bilateral(ops, imgd, None, 0, None, None, 0, alone, N, H, W, sxy, srgb)
    assert _guard_is_intact(alone, N * n)
    r = _ratio('bilateral normaliser', alone[:N * n].view(N, n).cpu().numpy(), want, bound)
    _report('bilateral normaliser', '%s %s' % (BIL_IDS[k], kind), r)
    assert r <= 1
    # v = NULL with out
    out = _guarded(N * n * LDO)
    _bilateral(ops, imgd, None, 0, None, out, LDO, None, N, H, W, sxy, srgb)
    got = out[:N * n * LDO].view(N, n, LDO).cpu().numpy()
    assert (got[..., LP:] == SENTINEL).all() and _guard_is_intact(out, N * n * LDO) and not got[..., 1:LP].any()
    for b in range(N):
        r = _ratio('bilateral row sum', got[b][:, 0], np.exp(exps[b]).sum(axis=1), crf_rules.message_bound(exps[b], np.ones((n, 1)))[:, 0])
        _report('bilateral row sum', '%s %s image %d' % (BIL_IDS[k], kind, b), r)
        assert r <= 1
    # norm_out together with out
    v = crf_rules.message_v(600 + k, N, n)
    v[..., 0] = 1
    vw = _wide(v, LDV)
    out.fill_(SENTINEL)
    both = _guarded(N * n)
    _bilateral(ops, imgd, vw, LDV, None, out, LDO, both, N, H, W, sxy, srgb)
    got = out[:N * n * LDO].view(N, n, LDO).cpu().numpy()
    assert (got[..., LP:] == SENTINEL).all() and _guard_is_intact(out, N * n * LDO) and _guard_is_intact(both, N * n)
    nrm = both[:N * n].view(N, n).cpu().numpy()
    assert np.array_equal(nrm.view(np.int32), (np.float32(1) / np.sqrt(got[..., 0] + np.float32(1e-20))).view(np.int32))
    assert np.array_equal(nrm.view(np.int32), alone[:N * n].view(N, n).cpu().numpy().view(np.int32))       # the same sum either way
    assert _ratio('bilateral normaliser', nrm, want, bound) <= 1
    for b in range(N):
        cols = COLS[1:]
        assert _ratio('bilateral message', got[b][:, cols], (np.exp(exps[b]) @ v[b].astype(np.float64))[:, cols],
                      crf_rules.message_bound(exps[b], v[b])[:, cols]) <= 1


# ------------------------------------------------------------------------------------------------ unary term and update
UPDATES = sorted(crf_rules.UPDATE_CASES)
NO_MASK = -77


def _census(ops, mask, gt, N, n, C):
    """dl3p_crf_unary -> (census (N, 2) on the device, Q0 (N, n, 32) as numpy) with Q rows of stride 40"""
    census = torch.zeros((N, 2), dtype=torch.int32, device='cuda')
    q = _guarded(N * n * LDQ)
    ops.lib().crf_unary(_p(mask), _p(census), _p(q), LDQ, gt, N, n, C, _st())
    torch.cuda.synchronize()
    got = q[:N * n * LDQ].view(N, n, LDQ).cpu().numpy()
    assert (got[..., LP:] == SENTINEL).all() and _guard_is_intact(q, N * n * LDQ)
    return census, got[..., :LP]


@pytest.mark.parametrize('name', UPDATES)
def test_the_unary_term_and_the_update_per_element(ops, name):
    """random non-negative messages and normalisers in every column; Q only, the mask only, and both; Q rows of stride 40.  The
    argmax equals the rule's wherever the rule's top-two gap exceeds twice the pixel's largest bound"""
    N, n, C, ids, gt, wg, wb = crf_rules.UPDATE_CASES[name]
    mask, fg, ng, fb, nb = crf_rules.update_inputs(name)
    md, fgd, ngd, fbd, nbd = (_dev(t) for t in (mask, fg, ng, fb, nb))
    census, q0 = _census(ops, md, gt, N, n, C)
    present = [sorted(c for c in ids[b] if 0 <= c < C) for b in range(N)]
    assert census.cpu().numpy().tolist() == [[sum(1 << c for c in p), len(p)] for p in present]      # in-range classes only
    rule = [(crf_rules.update(mask[b], C, None, None, None, None, 0, 0, gt), crf_rules.update_bound(mask[b], C, None, None, None, None, 0, 0, gt),
             crf_rules.update(mask[b], C, fg[b], ng, fb[b], nb[b], wg, wb, gt), crf_rules.update_bound(mask[b], C, fg[b], ng, fb[b], nb[b], wg, wb, gt))
            for b in range(N)]
    for b in range(N):
        r = _ratio('unary', q0[b][:, :C], rule[b][0][0], rule[b][1])
        _report('unary', '%s image %d' % (name, b), r)
        assert r <= 1 and not q0[b][:, C:].any()
    seen = {}
    for want_q, want_mask in ((True, False), (False, True), (True, True)):
        q = _guarded(N * n * LDQ)
        mo = _guarded(N * n, torch.int32, NO_MASK)
        ops.lib().crf_update(_p(md), _p(census), _p(fgd), _p(ngd), _p(fbd), _p(nbd), wg, wb, gt, _p(q) if want_q else None, LDQ,
                             _p(mo) if want_mask else None, N, n, C, _st())
        torch.cuda.synchronize()
        assert _guard_is_intact(q, N * n * LDQ) and _guard_is_intact(mo, N * n, NO_MASK)
        got = q[:N * n * LDQ].view(N, n, LDQ).cpu().numpy()
        arg = mo[:N * n].view(N, n).cpu().numpy()
        if not want_q:
            assert (got == SENTINEL).all()
        if not want_mask:
            assert (arg == NO_MASK).all()
        if want_q:
            assert (got[..., LP:] == SENTINEL).all() and not got[..., C:LP].any()
            assert seen.setdefault('q', got.tobytes()) == got.tobytes()                               # the same bits either way
            for b in range(N):
                r = _ratio('update', got[b][:, :C], rule[b][2][0], rule[b][3])
                _report('update', '%s image %d' % (name, b), r)
                assert r <= 1
        if want_mask:
            assert seen.setdefault('mask', arg.tobytes()) == arg.tobytes()
            for b in range(N):
                _, want_arg, gap = rule[b][2]
                clear = gap > 2 * rule[b][3].max(axis=1)
                assert 1 - clear.mean() <= crf_rules.NEAR_TIE_CAP and np.array_equal(arg[b][clear], want_arg[clear])


def test_a_gt_prob_of_0_3_moves_the_unary_argmax_to_the_other_class(ops):
    """two present classes and gt_prob < 0.5: Q0 is (0.3 own, 0.7 other), so the update without messages and iterations=0 of
    ops.dense_crf return the other class at every pixel; with the default gt_prob iterations=0 returns the mask"""
    N, n, C, ids, gt, _, _ = crf_rules.UPDATE_CASES['gt-0.3']
    mask = crf_rules.update_inputs('gt-0.3')[0]
    lo, hi = ids[0]
    other = np.where(mask == lo, hi, lo).astype(np.int32)
    md = _dev(mask)
    census, q0 = _census(ops, md, gt, N, n, C)
    mo = _guarded(N * n, torch.int32, NO_MASK)
    ops.lib().crf_update(_p(md), _p(census), None, None, None, None, 0.0, 0.0, gt, None, LDQ, _p(mo), N, n, C, _st())
    torch.cuda.synchronize()
    assert _guard_is_intact(mo, N * n, NO_MASK) and np.array_equal(mo[:N * n].view(N, n).cpu().numpy(), other)
    img = torch.zeros((1, 1, n, 3), dtype=torch.uint8, device='cuda')
    got, q = ops.dense_crf(img, md.view(1, 1, n), C, iterations=0, gt_prob=gt, want_q=True)
    assert np.array_equal(got.cpu().numpy().reshape(N, n), other)
    want_q, _, _ = crf_rules.update(mask[0], C, None, None, None, None, 0, 0, gt)
    assert _ratio('unary', q.cpu().numpy().reshape(n, C), want_q, crf_rules.update_bound(mask[0], C, None, None, None, None, 0, 0, gt)) <= 1
    same = ops.dense_crf(img, md.view(1, 1, n), C, iterations=0)
    assert torch.equal(same.view(N, n), md) and same.data_ptr() != md.data_ptr()


def test_ids_outside_the_classes_without_messages(ops):
    """iterations=0 on masks with -1, C and 255: such a pixel ties every present class exactly (Q = 1 / n_labels bit for bit) and
    takes the lowest present id; every other pixel keeps its class; an image with one present class comes back as it came"""
    N, n, C, ids, gt, _, _ = crf_rules.UPDATE_CASES['outside']
    mask = crf_rules.update_inputs('outside')[0]
    H, W = 7, 43
    assert H * W == n
    img = torch.zeros((N, H, W, 3), dtype=torch.uint8, device='cuda')
    got, q = ops.dense_crf(img, _dev(mask).view(N, H, W), C, iterations=0, want_q=True)
    got, q = got.cpu().numpy().reshape(N, n), q.cpu().numpy().reshape(N, n, C)
    outside = (mask < 0) | (mask >= C)
    assert outside[0].sum() >= 3 and outside[1].sum() >= 1
    assert np.array_equal(got[0], np.where(outside[0], 0, mask[0])) and np.array_equal(got[1], mask[1])
    third = np.float32(1) / np.float32(3)
    assert (q[0][outside[0]][:, [0, 2, 5]] == third).all() and not q[0][:, [1, 3, 4]].any()
    assert (q[1][:, 3] == 1).all() and q[1].sum() == n
    for b in range(N):
        want = crf_rules.update(mask[b], C, None, None, None, None, 0, 0, gt)[0]
        assert _ratio('unary', q[b], want, crf_rules.update_bound(mask[b], C, None, None, None, None, 0, 0, gt)) <= 1


# ------------------------------------------------------------------------------------------------ end to end
def _end_to_end(ops, name, imgs, masks, C, kw, rule):
    want_mask, want_q, gap = rule
    got_mask, got_q = ops.dense_crf(_dev(imgs), _dev(masks), C, want_q=True, **kw)
    err = np.abs(got_q.cpu().numpy() - want_q)
    clear = gap >= crf_rules.NEAR_TIE
    got_mask = got_mask.cpu().numpy()
    print('end to end %s: max |Q - rule| %.3e; near-tie share %.2e, mask mismatch share %.2e' % (
        name, err.max(), 1 - clear.mean(), (got_mask != want_mask).mean()))
    assert err.max() <= crf_rules.Q_ATOL
    assert 1 - clear.mean() <= crf_rules.NEAR_TIE_CAP
    assert np.array_equal(got_mask[clear], want_mask[clear])
    return got_mask


@pytest.mark.parametrize('i', range(len(crf_rules.EDGE_CASES)), ids=crf_rules.EDGE_IDS)
def test_q_and_mask_follow_the_rule_at_the_edge_cases(ops, i):
    """ops.dense_crf with each row's keyword arguments under the bound of tests/test_crf_gpu.py (swapped weights or one iteration
    fewer move Q by ten times that bound: test_crf_rules_cpu)"""
    N, H, W, C, _, kw = crf_rules.EDGE_CASES[i]
    imgs, masks = crf_rules.edge_inputs(i)
    _end_to_end(ops, crf_rules.EDGE_IDS[i], imgs, masks, C, kw, crf_rules.edge_rule(i))


def test_q_and_mask_follow_the_rule_with_ids_outside_the_classes(ops):
    i = crf_rules.OUTSIDE_BASE
    N, H, W, C, _, kw = crf_rules.EDGE_CASES[i]
    imgs, masks = crf_rules.outside_inputs()
    got = _end_to_end(ops, 'ids outside [0, %d)' % C, imgs, masks, C, kw, crf_rules.outside_rule())
    assert ((got >= 0) & (got < C)).all()
    # fewer than two present classes: unchanged, such ids included
    one = np.where((masks < 0) | (masks >= C), masks, 1).astype(np.int32)
    back = ops.dense_crf(_dev(imgs), _dev(one), C, **kw)
    assert np.array_equal(back.cpu().numpy(), one)


def test_the_dictionary_of_deeplab_reaches_the_kernels(ops, tmp_path):
    """DeepLab(dense_crf={...}) refines with the row's parameters: the result follows the rule at those parameters and differs from
    the rule at the defaults on pixels both decide clearly"""
    i = 1
    N, H, W, C, _, kw = crf_rules.EDGE_CASES[i]
    imgs, masks = crf_rules.edge_inputs(i)
    want, _, gap = crf_rules.edge_rule(i)
    default_mask, default_q = crf_rules.dense_crf(imgs[0], masks[0], C)
    clear = gap[0] >= crf_rules.NEAR_TIE
    both_clear = clear & (crf_rules.top_two_gap(default_q) >= crf_rules.NEAR_TIE)
    assert (default_mask != want[0])[both_clear].any()
    classes = tmp_path / 'classes.txt'
    classes.write_text('\n'.join('class%d' % c for c in range(C)) + '\n')
    d = load_pkg('inference').DeepLab(dense_crf=dict(kw), model_type='mobilenetv2_lite', model_input_shape=(65, 65), output_stride=16,
                                      classes_path=str(classes), weights_path=None)
    got = d._refine(_dev(masks), _dev(imgs)).cpu().numpy()
    assert np.array_equal(got[0][clear], want[0][clear])
    assert (got[0] != default_mask)[both_clear].any()


# ------------------------------------------------------------------------------------------------ front-end helpers
@pytest.mark.parametrize('C', [1, 21, 64])
@pytest.mark.parametrize('total', [1, 255, 257, 600000])
def test_mask_confusion_counts_like_numpy(ops, total, C):
    """labels are float32 and become class ids by the C++ conversion (int), which truncates towards zero: 2.75 counts as class 2,
    -0.5 as class 0, -1 stays -1; labels outside [0, C) after that (-1, C, 255) and predictions outside [0, C) (-1, C) are skipped.
    600000 pixels are past the grid cap (2048 workgroups of 256).  The counters start non-zero and are added to"""
    rng = np.random.default_rng(1000 * C + total % 997)
    special = np.array([-0.5, 2.75, -1, C, 255, 0], np.float32)
    labels = rng.integers(0, C, total).astype(np.float32)
    pred = rng.integers(-1, C + 1, total).astype(np.int32)
    at = rng.permutation(total)[:max(1, total // 8)]
    labels[at] = special[np.arange(at.size) % special.size]
    pred[at[:special.size]] = 0                                    # (the first of each special label meets a valid prediction)
    start = rng.integers(1, 1000, (C, C)).astype(np.int64)
    lab = np.trunc(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < C) & (pred >= 0) & (pred < C)
    want = start.copy()
    np.add.at(want, (lab[ok], pred[ok].astype(np.int64)), 1)
    cm = _guarded(C * C, torch.int64, -5)
    cm[:C * C] = _dev(start).view(-1)
    pd, ld = _dev(pred), _dev(labels)
    ops.lib().mask_confusion(_p(pd), _p(ld), _p(cm), total, C, _st())
    torch.cuda.synchronize()
    assert _guard_is_intact(cm, C * C, -5)
    assert np.array_equal(cm[:C * C].view(C, C).cpu().numpy(), want) and want.sum() - start.sum() == ok.sum()
    if total == 1:
        assert labels[0] == np.float32(-0.5) and ok[0] and want[0, 0] == start[0, 0] + 1
    # the Python wrapper on the same inputs, its own counters
    got = ops.mask_confusion(pd, ld, C, confusion=_dev(start))
    assert np.array_equal(got.cpu().numpy(), want)


def test_denormalize_u8_clamps_then_truncates(ops):
    """all 256 values b / 127.5 - 1 with their float32 neighbours on both sides, the ends, -0.0, +-2, +-inf and NaN against
    "x * 127.5 + 127.5 in float32 (two roundings), clamp to [0, 255], truncate".  NaN gives 0: fmaxf(NaN, 0) returns its other
    argument (IEEE 754 maxNum), 0, which fminf leaves alone"""
    f = np.float32
    base = np.arange(256, dtype=f) / f(127.5) - f(1)
    x = np.concatenate([base, np.nextafter(base, f(np.inf)), np.nextafter(base, f(-np.inf)),
                        np.array([-1, 1, -0.0, 2, -2, np.inf, -np.inf, np.nan], f)]).astype(f)
    t = x * f(127.5) + f(127.5)
    want = np.fmin(np.fmax(t, f(0)), f(255)).astype(np.uint8)          # np.fmax / np.fmin: the non-NaN argument, as fmaxf / fminf
    assert want[-1] == 0 and want[-2] == 0 and want[-3] == 255 and want[-6] == 127
    out = _guarded(x.size, torch.uint8, 99)
    xd = _dev(x)
    ops.lib().denormalize_u8(_p(xd), _p(out), x.size, _st())
    torch.cuda.synchronize()
    assert _guard_is_intact(out, x.size, 99)
    got = out[:x.size].cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert np.array_equal(ops.denormalize_u8(xd).cpu().numpy(), want)
    # every byte survives the round trip through the normalised float
    assert np.array_equal(got[:256], np.arange(256, dtype=np.uint8))
