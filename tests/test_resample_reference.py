"""The float64 restatement of the resampling, pooling and label kernels (tests/resample_reference.py) is checked first, without a GPU: against
the oracle's layers, against the committed fixtures, against autograd of the training reference, by adjointness, and on a few cells worked by
hand.  test_gpu_resample_stages.py then compares the HIP kernels with it."""
import os

import numpy as np
import pytest
import torch

import casapose_oracle as O
import resample_cases as Cs
import resample_reference as R
import torch_train_ref as T

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = Cs.UP_SHAPES + (Cs.CRAFTED_SHAPE, Cs.PYRAMID_SHAPE)
EPS = 2.0 ** -52


def shape_id(shape):
    return "x".join(map(str, shape))


def rel(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(np.abs(b).max(), 1e-9)


def close(a, b, terms=16):
    """equal up to `terms` float64 roundings of the largest magnitude involved"""
    scale = max(float(np.abs(a).max()), float(np.abs(b).max()), 1e-300)
    return float(np.abs(a - b).max()) <= terms * EPS * scale


def halved_pair(shape, seed):
    """hi and lo = hi[:, ::2, ::2], the pair that the oracle's one-hot interface expresses, with its one-hot maps"""
    b, h, w, _ = shape
    rng = np.random.default_rng(seed)
    hi = Cs.blobs(rng, b, 2 * h, 2 * w)
    seg_u = O.onehot_from_labels(hi.astype(np.int64), 3)
    return hi, hi[:, ::2, ::2], O.half_size(seg_u), seg_u, rng


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_forwards_agree_with_the_oracle(shape):
    hi, lo, seg_d, seg_u, rng = halved_pair(shape, 5)
    x = rng.standard_normal(shape)
    sel = R.sel_map(hi, lo)
    assert np.array_equal(sel, O.guided_upsampling_select(seg_d, seg_u))
    assert np.array_equal(R.guided_nearest(x, sel), O.guided_upsampling(x, seg_d, seg_u))
    assert close(R.guided_bilinear(x, R.match_mask(hi, lo)).out, O.guided_bilinear_upsampling(x, seg_d, seg_u))
    assert close(R.bilinear_x2(x).out, O.upsample_bilinear_x2(x))


@pytest.mark.parametrize("kind", Cs.POOL_KINDS)
@pytest.mark.parametrize("shape", Cs.POOL_SHAPES, ids=shape_id)
def test_maxpool_agrees_with_the_oracle(shape, kind):
    x = Cs.pool(shape, kind).x.astype(np.float64)
    r = R.maxpool(x)
    assert np.array_equal(r.val, O.maxpool_3x3_s2_pad1(x))
    assert r.idx.shape == r.val.shape and r.idx.max() <= 8
    # the index is the FIRST tap that holds the value
    taps = np.arange(9)[None, None, None, :, None]
    assert np.array_equal(r.idx, np.where(r.win == r.val[:, :, :, None], taps, 9).min(3))


def test_forwards_reproduce_the_fixtures():
    g = np.load(os.path.join(G, "layers_k4_12x16.npz"))
    hi = g["labels"]
    lo = hi[:, ::2, ::2]
    low = g["low"].astype(np.float64)
    assert rel(R.guided_nearest(low, R.sel_map(hi, lo)), g["guided_up"]) < 1e-7
    assert rel(R.guided_bilinear(low, R.match_mask(hi, lo)).out, g["guided_bilinear_up"]) < 1e-6
    assert rel(R.bilinear_x2(low).out, g["bilinear_up"]) < 1e-6


def autograd(fn, x, dy):
    xt = torch.from_numpy(np.array(x, np.float64)).requires_grad_(True)
    fn(xt).backward(torch.from_numpy(np.array(dy, np.float64)))
    return xt.grad.numpy()


@pytest.mark.parametrize("name", Cs.GUIDED_NAMES)
def test_upsampling_adjoints_agree_with_autograd(name):
    case = Cs.guided(name)
    lo, hi = torch.from_numpy(np.array(case.lo)), torch.from_numpy(np.array(case.hi))
    for dy in (case.dy, case.dy_int):
        assert close(R.guided_bilinear_bwd(dy, case.mask).out, autograd(lambda t: T.guided_bilinear_upsample(t, lo, hi), case.x, dy), 64)
        assert close(R.guided_nearest_bwd(dy, case.sel), autograd(lambda t: T.guided_upsample(t, lo, hi), case.x, dy), 64)
        assert close(R.bilinear_x2_bwd(dy).out, autograd(T.bilinear_x2, case.x, dy), 64)
    assert np.array_equal(T.guided_select(lo.to(torch.int64), hi.to(torch.int64)).numpy(), case.sel)


@pytest.mark.parametrize("kind", Cs.POOL_KINDS)
@pytest.mark.parametrize("shape", Cs.POOL_SHAPES, ids=shape_id)
def test_maxpool_adjoint_agrees_with_autograd_where_the_maximum_is_unique(shape, kind):
    case = Cs.pool(shape, kind)
    r = R.maxpool(case.x)
    unique = (r.win == r.val[:, :, :, None]).sum(3) == 1          # the padded taps count: a zero that ties with the padding is a tie
    dy = np.where(unique, case.dy, 0.0)
    assert np.array_equal(R.maxpool_bwd(case.x, dy), autograd(T.maxpool_zero_pad, case.x, dy))
    if shape in ((2, 7, 9, 64), (2, 9, 13, 12), (2, 10, 14, 32)):
        # a strict subset: the tied remainder is what the GPU test pins
        assert 0 < int(unique.sum()) < unique.size and (~unique & (case.dy != 0)).any(), (shape, kind)
    # accumulate: the previous dx is added to, exactly (small integers)
    assert np.array_equal(R.maxpool_bwd(case.x, case.dy, case.dx_prev), R.maxpool_bwd(case.x, case.dy) + case.dx_prev)


@pytest.mark.parametrize("name", Cs.GUIDED_NAMES)
def test_adjointness(name):
    case = Cs.guided(name)
    x, dy = case.x.astype(np.float64), case.dy.astype(np.float64)
    pairs = ((R.guided_bilinear(x, case.mask).out, R.guided_bilinear_bwd(dy, case.mask).out),
             (R.guided_nearest(x, case.sel), R.guided_nearest_bwd(dy, case.sel)),
             (R.bilinear_x2(x).out, R.bilinear_x2_bwd(dy).out))
    for up, down in pairs:
        lhs, rhs = float((up * dy).sum()), float((x * down).sum())
        assert abs(lhs - rhs) <= 64 * EPS * float(np.abs(up * dy).sum() + np.abs(x * down).sum() + 1e-300), (name, lhs, rhs)


def test_sums_of_absolute_products_and_term_counts():
    case = Cs.guided("independent_2x7x9x64")
    f = R.guided_bilinear(case.x, case.mask)
    assert (f.S >= np.abs(f.out) - 1e-12).all() and f.n.max() <= 4 and ((f.n == 0) == (np.broadcast_to((case.mask == 0)[..., None], f.n.shape))).all()
    assert (f.out[case.mask == 0] == 0).all() and (f.S[case.mask == 0] == 0).all()
    b = R.guided_bilinear_bwd(case.dy, case.mask)
    assert (b.S >= np.abs(b.out) - 1e-12).all() and 4 < b.n.max() <= 16
    bl = R.bilinear_x2_bwd(case.dy)
    assert bl.n.max() == 16 and bl.n.sum() == 4 * case.dy.size           # every hi-res pixel scatters four terms; a corner collects 16 of them
    # coefficients of a pixel add up to 1 wherever a tap matches (the replaced taps hand their weight on), else to 0
    coef = R.guided_bilinear_coefficients(case.mask)
    assert np.allclose(coef.sum(-1), case.mask != 0, rtol=0, atol=4 * EPS)


def test_gather_and_scatter_are_adjoint_and_skip_negative_indices():
    f = Cs.flat(700)
    got = R.gather(f.table, f.idx)
    assert (got[f.idx < 0] == 0).all() and np.array_equal(got[f.idx >= 0], f.table[f.idx[f.idx >= 0]])
    zeros = np.zeros_like(f.table)
    scattered = R.scatter(f.src, f.idx, zeros, accumulate=False)
    assert float((got.astype(np.float64) * f.src).sum()) == float((f.table.astype(np.float64) * scattered).sum())
    assert np.array_equal(R.scatter(f.src, f.idx, f.table, accumulate=True), f.table + scattered)
    untouched = np.setdiff1d(np.arange(len(f.table)), f.idx[f.idx >= 0])
    assert np.array_equal(R.scatter(f.src, f.idx, f.table, accumulate=False)[untouched], f.table[untouched])
    assert np.array_equal(R.pad3to4(f.rgb)[:, :3], f.rgb) and not R.pad3to4(f.rgb)[:, 3].any()
    ax = R.axpby(f.a, 0.75, f.b, -1.5)
    assert np.array_equal(ax.out, 0.75 * f.a.astype(np.float64) - 1.5 * f.b.astype(np.float64))
    assert np.array_equal(R.axpby(f.a, 2.0, None, 9.0).out, 2.0 * f.a.astype(np.float64))


# ---- cells worked by hand, in a 2x2 low-resolution map ----------------------------------------------------------------------------------------------
def one_pixel(lo, hi_label, sub):
    """coefficients and selection of hi-res pixel `sub` of cell (0, 0): the whole hi-res map carries `hi_label`"""
    lo = np.array(lo, np.uint8)[None]
    hi = np.full((1, 4, 4), hi_label, np.uint8)
    mask = R.match_mask(hi, lo)
    return mask[0, sub // 2, sub % 2], R.guided_bilinear_coefficients(mask)[0, sub // 2, sub % 2], R.sel_map(hi, lo)[0, sub // 2, sub % 2]


def test_hand_worked_cells():
    x = np.array([[[[1.0], [10.0]], [[100.0], [1000.0]]]])
    # no tap matches: every coefficient, and the result, is 0; the nearest layer falls back to tap 0
    for sub in range(4):
        m, coef, sel = one_pixel([[1, 1], [1, 1]], 2, sub)
        assert m == 0 and not coef.any() and sel == 0
    hi = np.full((1, 4, 4), 2, np.uint8)
    assert not R.guided_bilinear(x, R.match_mask(hi, np.ones((1, 2, 2), np.uint8))).out.any()
    # only tap 3 matches, at sub-pixel 3: it stands in for the three others, coefficient 1
    m, coef, sel = one_pixel([[1, 1], [1, 2]], 2, 3)
    assert m == 8 and np.array_equal(coef, [0, 0, 0, 1]) and sel == 3
    lo = np.array([[[1, 1], [1, 2]]], np.uint8)
    assert R.guided_bilinear(x, R.match_mask(hi, lo)).out[0, 1, 1, 0] == 1000.0
    # three taps match at sub-pixel 1 (weights 1/2, 1/2, 0, 0) and tap 1 is the foreign one: its 1/2 goes to the mean of the three, so
    # tap 0 has 1/2 + 1/6 and taps 2 and 3 have 1/6 each (the coefficients of a pixel add up to 1)
    m, coef, sel = one_pixel([[2, 1], [2, 2]], 2, 1)
    assert m == 0b1101 and np.allclose(coef, [0.5 + 1 / 6, 0, 1 / 6, 1 / 6], rtol=0, atol=2 * EPS) and sel == 0
    lo = np.array([[[2, 1], [2, 2]]], np.uint8)
    assert abs(R.guided_bilinear(x, R.match_mask(hi, lo)).out[0, 0, 1, 0] - ((0.5 + 1 / 6) * 1 + 100 / 6 + 1000 / 6)) < 1e-12
    # the same three with the foreign tap carrying no weight (tap 3 at sub-pixel 1): nothing to hand on
    m, coef, sel = one_pixel([[2, 2], [2, 1]], 2, 1)
    assert m == 0b0111 and np.array_equal(coef, [0.5, 0.5, 0, 0])
    # the last column of the 2x2 map: taps 1 and 3 are padding and match nothing, whatever the label
    same = R.match_mask(np.zeros((1, 4, 4), np.uint8), np.zeros((1, 2, 2), np.uint8))
    assert same[0, 0, 0] == 0b1111 and same[0, 0, 2] == 0b0101 and same[0, 2, 0] == 0b0011 and same[0, 3, 3] == 0b0001
    # max-pool of a single zero: the padding (tap 0) comes first and wins; of a single positive value: tap 4
    assert R.maxpool(np.zeros((1, 1, 1, 1))).idx.item() == 0 and R.maxpool(np.ones((1, 1, 1, 1))).idx.item() == 4
    assert R.maxpool_bwd(np.zeros((1, 1, 1, 1)), np.ones((1, 1, 1, 1))).item() == 0 and R.maxpool_bwd(np.ones((1, 1, 1, 1)), np.ones((1, 1, 1, 1))).item() == 1
    # bilinear x2 of two pixels in a row: clamped ends, 3/4 - 1/4 in between
    assert np.array_equal(R.bilinear_x2(np.array([[[[0.0], [4.0]]]])).out[0, :, :, 0], [[0, 1, 3, 4], [0, 1, 3, 4]])


def test_the_cases_hold_their_conditions():
    Cs.check_guided_coverage()
    Cs.check_pool_conditions()
    Cs.check_argmax_routes()
    assert len(Cs.argmax_configs()) >= 60
    for name, shape in (("big_fwd", Cs.UP_FWD_BIG), ("big_bwd", Cs.UP_BWD_BIG)):
        assert dict(Cs.GUIDED_SHAPES)[name] == shape
