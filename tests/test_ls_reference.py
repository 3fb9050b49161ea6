"""tests/ls_reference.py (the fp64 restatement the GPU stage tests of the LS voter compare with) pinned on the CPU: its fp32-order sums against
O.ls_voting_sums, its solve against O.ls_voting, its backward closed form against fp64 autograd of R.ls_voting, its reprojection loss against
autograd of R.keypoint_reprojection_loss, the rank-one object against its analytic answer -- and the conditions the GPU tests need of the shared
scenes, on the builders they import."""
import itertools

import numpy as np
import pytest
import torch

import casapose_oracle as O
import ls_reference as L
import torch_train_ref as R


def _split(s):
    """(seg, direct, conf) of a scene for the oracle, which multiplies by the mask instead of selecting: NaN -> 0."""
    f = np.nan_to_num(s.field)
    return (f[..., s.seg_off:s.seg_off + s.objects + 1], f[..., s.dir_off:s.dir_off + 18], f[..., s.conf_off:s.conf_off + 9])


@pytest.mark.parametrize("layout,w", [("rec36", 139), ("rec40", 136)])
def test_fp32_order_sums_equal_the_oracle(layout, w):
    s = L.scene(w, argmax=True, **L.LAYOUTS[layout])
    lab = L.argmax_labels(s.field, s.seg_off, s.objects)
    assert np.array_equal(lab, s.labels)                       # first maximum: the ties did not move a label
    seg = s.field[..., s.seg_off:s.seg_off + s.objects + 1]
    assert ((seg == seg.max(-1, keepdims=True)).sum(-1) > 1).mean() > 0.01
    t32, t64 = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)
    got, mag = L.sums(t32, lab, s.objects)
    want = O.ls_voting_sums(*_split(s))
    ratio = np.abs(got - want) / np.where(mag > 0, mag, 1.0)
    print("fp64 summation order only: %.2e of sum |term|" % ratio.max())
    assert (np.abs(got - want) <= 1e-13 * mag).all()
    assert not got[:, 5:].any() and got[:, :5].any(-1).all()   # three absent objects
    s64, _ = L.sums(t64, lab, s.objects)                       # the fp32 terms are the fp64 ones after a handful of fp32 roundings (4.3e-7 here)
    assert (np.abs(got - s64) <= 1e-6 * mag).all() and (got != s64).any()


def test_solve_equals_the_oracle_to_fp32_rounding():
    s = L.scene(139, argmax=True, **L.LAYOUTS["rec36"])
    seg, direct, conf = _split(s)
    hot = np.eye(s.objects + 1, dtype=np.float32)[s.labels][..., 1:]
    want = O.ls_voting(seg, direct, conf, hot_override=hot).astype(np.float64)
    t32, _ = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)
    sm, _ = L.sums(t32, s.labels, s.objects)
    got = L.solve(sm, s.h)
    cond = np.where(np.isfinite(L.condition(sm)), L.condition(sm), 0.0)[..., None]
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(got) + 1e-12 * cond * s.h).all()
    assert not got[:, 5:].any() and np.abs(got[:, :5]).min() > 0


def _autograd(s, dkp):
    ft = torch.tensor(np.nan_to_num(s.field).astype(np.float64), requires_grad=True)
    kp = R.ls_voting(torch.from_numpy(s.labels.astype(np.int64)), ft[..., s.dir_off:s.dir_off + 18], ft[..., s.conf_off:s.conf_off + 9], s.objects)
    (kp * torch.from_numpy(dkp)).sum().backward()
    g = ft.grad.numpy().reshape(-1, s.ld)
    return kp.detach().numpy(), g[:, s.dir_off:s.dir_off + 18].reshape(-1, 9, 2), g[:, s.conf_off:s.conf_off + 9]


def slice_ratio(s, idx, got, want):
    """Largest |got - want| per (image, object, keypoint) over the object's listed pixels, relative to that slice's largest |want|."""
    lab = s.labels.reshape(-1)[idx]
    img = idx // (s.h * s.w)
    worst = 0.0
    for bi, o in itertools.product(range(s.b), range(s.objects)):
        m = (img == bi) & (lab == o + 1)
        if m.any():
            for j in range(s.kp):
                ref = np.abs(want[m, j]).max()
                assert ref > 0
                worst = max(worst, float(np.abs(got[m, j] - want[m, j]).max() / ref))
    return worst


AUTOGRAD_GATE = 3e-11    # ten times the measured 2.95e-12 (directions; confidences 9.1e-14): two fp64 evaluation orders at condition numbers up to 170


def test_pixel_grads_equal_fp64_autograd():
    s = L.scene(139, **L.LAYOUTS["rec36"])
    s.field, s.labels, s.b = s.field[:2], s.labels[:2], 2
    dkp = np.random.default_rng(3).normal(0, 1, (s.b, s.objects, 9, 2))
    _, t64 = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)
    sm, _ = L.sums(t64, s.labels, s.objects)
    pu, cond = L.prepare(sm, dkp, s.h)
    assert np.isfinite(cond[:, :5]).all() and cond[:, :5].max() > 30 and not pu[:, 5:].any()
    idx, gd, gcf = L.pixel_grads(s.field, s.dir_off, s.conf_off, s.labels, None, None, pu, s.h)
    kp, ad, ac = _autograd(s, dkp)
    assert np.abs(kp - L.solve(sm, s.h)).max() <= 1e-9
    assert np.array_equal(idx, np.flatnonzero(s.labels.reshape(-1) > 0))
    rest = np.ones(ad.shape[0], bool)
    rest[idx] = False
    assert not ad[rest].any() and not ac[rest].any()
    zero = ~np.nan_to_num(s.field).reshape(-1, s.ld)[idx, s.dir_off:s.dir_off + 18].reshape(-1, 9, 2).any(-1)
    assert 0.01 < zero.mean() < 0.03 and not gd[zero].any() and not ad[idx][zero].any()      # exactly 0 on both sides
    rd = max(slice_ratio(s, idx, gd[..., c], ad[idx][..., c]) for c in (0, 1))
    rc = slice_ratio(s, idx, gcf, ac[idx])
    print("closed form with its own fp64 table against autograd: directions %.2e, confidences %.2e" % (rd, rc))
    assert rd <= AUTOGRAD_GATE and rc <= AUTOGRAD_GATE
    # the fp32-rounded table, as ls_bwd_prepare_kernel stores it, is what costs accuracy
    _, gd32, gcf32 = L.pixel_grads(s.field, s.dir_off, s.conf_off, s.labels, None, None, pu.astype(np.float32), s.h)
    r32 = max(slice_ratio(s, idx, gd32[..., 0], ad[idx][..., 0]), slice_ratio(s, idx, gd32[..., 1], ad[idx][..., 1]), slice_ratio(s, idx, gcf32, ac[idx]))
    print("the same with the table rounded to fp32: %.2e" % r32)
    assert 1e-8 < r32 < 1e-4


def test_regulariser_term_is_the_gradient_of_the_softplus_sum():
    s = L.scene(136, reg=True, **L.LAYOUTS["rec40"])
    coef = np.random.default_rng(4).normal(0, 1, (s.b, 9))
    pu = np.zeros((s.b, s.objects, 9, 4))
    idx, gd, gcf = L.pixel_grads(s.field, s.dir_off, s.conf_off, s.labels, s.reg_labels, coef, pu, s.h)
    ct = torch.tensor(np.nan_to_num(s.field[..., s.conf_off:s.conf_off + 9]).astype(np.float64), requires_grad=True)
    m = torch.from_numpy((s.reg_labels > 0).astype(np.float64))[..., None]
    ((torch.nn.functional.softplus(ct) * m).sum((1, 2)) * torch.from_numpy(coef)).sum().backward()
    want = ct.grad.numpy().reshape(-1, 9)
    assert np.array_equal(idx, np.flatnonzero((s.labels.reshape(-1) > 0) | (s.reg_labels.reshape(-1) > 0)))
    assert not gd.any() and np.abs(gcf - want[idx]).max() <= 1e-15 and np.abs(want[idx]).max() > 0.5


def test_reprojection_loss_equals_autograd():
    coords, gt, A, avail, cap = L.reproj_case()
    value, g = L.kp_reproj_loss(coords, gt, A, avail, cap, 0.007)
    ct = torch.tensor(coords.astype(np.float64), requires_grad=True)
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    loss = R.keypoint_reprojection_loss(ct, t(gt), t(A), t(avail), None, None, cap, False)
    (0.007 * loss).backward()
    want = ct.grad.numpy()
    assert abs(value - loss.item()) <= 1e-14 * loss.item() and np.abs(g - want).max() <= 1e-15
    # the case holds what the GPU test says it holds
    X = A[:, None, None, 0, 0] * coords[..., 1] + A[:, None, None, 0, 1] * coords[..., 0] + A[:, None, None, 0, 2]
    Y = A[:, None, None, 1, 0] * coords[..., 1] + A[:, None, None, 1, 1] * coords[..., 0] + A[:, None, None, 1, 2]
    e = np.sqrt((gt[..., 0] - X) ** 2 + (gt[..., 1] - Y) ** 2)
    assert e[2, 3, 4] == 0 and not g[2, 3, 4].any() and (e[0, 1] - 0.5 > cap).all() and (e < 1).sum() > 50 and ((e > 1) & (e - 0.5 < cap)).sum() > 50
    assert not g[1, 2].any() and not g[3, 7].any() and np.abs(g).max() > 0
    assert L.kp_reproj_loss(coords, gt, A, avail * 0, cap, 0.007)[0] == 0.0 and not L.kp_reproj_loss(coords, gt, A, avail * 0, cap, 0.007)[1].any()


def test_rank_one_object_has_its_analytic_answer():
    s = L.scene(139, rank_one=True, **L.LAYOUTS["rec36"])
    t32, t64 = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)
    for t in (t32, t64):
        sm, _ = L.sums(t, s.labels, s.objects)
        r1 = sm[:, L.RANK_ONE - 1]
        assert not r1[..., [0, 1, 3]].any() and (r1[..., 2] > 0).all()                 # r00 = r01 = 0: det = 0
        kp = L.solve(sm, s.h)[:, L.RANK_ONE - 1]
        for bi in range(s.b):
            m = s.labels[bi] == L.RANK_ONE
            wgt = np.logaddexp(0.0, s.field[bi][m][:, s.conf_off:s.conf_off + 9].astype(np.float64))
            x = (wgt * (np.nonzero(m)[1] + 0.5)[:, None]).sum(0) / wgt.sum(0)
            assert not kp[bi, :, 0].any() and np.abs(kp[bi, :, 1] - x).max() <= 1e-5
        pu, cond = L.prepare(sm, np.ones((s.b, s.objects, 9, 2)), s.h)
        assert not pu[:, L.RANK_ONE - 1].any() and np.isinf(cond[:, L.RANK_ONE - 1]).all() and pu[:, :4].all()


def test_kp_stats_counts_out_of_range_labels_as_background():
    rng = np.random.default_rng(6)
    lab, est = rng.integers(0, 9, (2, 7, 11)).astype(np.uint8), rng.integers(0, 14, (2, 7, 11)).astype(np.uint8)
    field = rng.normal(0, 3, (2, 7, 11, 12)).astype(np.float32)
    counts, cs = L.kp_stats(field, 2, lab, est, 9)
    for bi in range(2):
        assert counts[0, bi].tolist() == [int((lab[bi] == c).sum()) for c in range(9)]
        assert counts[1, bi].tolist() == [int(((est[bi] == 0) | (est[bi] >= 9)).sum())] + [int((est[bi] == c).sum()) for c in range(1, 9)]
        want = sum(np.log1p(np.exp(field[bi, y, x, 2:11].astype(np.float64))) for y in range(7) for x in range(11) if lab[bi, y, x] > 0)
        assert np.abs(cs[bi] - want).max() <= 1e-12 * want.max()


@pytest.mark.parametrize("layout", sorted(L.LAYOUTS))
@pytest.mark.parametrize("w", L.WIDTHS)
def test_scenes_are_what_the_stage_tests_assume(layout, w):
    lay = L.LAYOUTS[layout]
    for kind in ({"argmax": True}, {}, {"reg": True}, {"rank_one": True}):
        if kind.get("argmax") and layout == "rec32":
            continue
        s = L.scene(w, **lay, **kind)
        objects = s.objects
        counts = np.stack([(s.labels == o + 1).sum((1, 2)) for o in range(objects)], 1)
        assert s.labels.max() <= objects and (counts[:, :5] >= 50).all() and not counts[:, 5:].any() and objects - 5 == (3 if objects == 8 else 0)
        _, t64 = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)
        sm, _ = L.sums(t64, s.labels, objects)
        cond = L.condition(sm)[:, :5]
        if s.rank_one:
            assert np.isinf(cond[:, L.RANK_ONE - 1]).all()
            cond = np.delete(cond, L.RANK_ONE - 1, 1)
        print("%s w=%d %s: condition numbers up to %.0f" % (layout, w, kind, cond.max()))
        assert cond.max() <= 200 and cond.max() >= 30
        fg, f = s.labels > 0, s.field
        chan = np.zeros(s.ld, bool)
        chan[s.dir_off:s.dir_off + 18] = chan[s.conf_off:s.conf_off + 9] = True
        used = fg if s.reg_labels is None else fg | (s.reg_labels > 0)
        assert np.isfinite(f[fg][:, chan]).all() and np.isnan(f[~used][:, chan]).all() and np.isnan(f[~fg][:, s.dir_off:s.dir_off + 18]).all()
        seg = np.zeros(s.ld, bool)
        seg[s.seg_off:s.seg_off + objects + 1] = kind.get("argmax", False)
        assert np.isnan(f[..., ~(chan | seg)]).all() and np.isfinite(f[..., seg]).all()
        conf, d = f[fg][:, s.conf_off:s.conf_off + 9], f[fg][:, s.dir_off:s.dir_off + 18].reshape(-1, 9, 2)
        tiny = f[s.labels == L.TINY][:, s.conf_off:s.conf_off + 9]
        assert tiny.min() >= -16 and tiny.max() <= -14 and conf.max() > 15 and conf.min() < -17
        assert 0.01 < (~d.any(-1)).mean() < 0.03
        # the strips: object 1 only in the last, partial strip column and down to the last row; the rows between object 2's rows are empty over whole
        # strips; object 3 lies in four strips; every image differs from the others
        assert not (s.labels[:, :, :128] == 1).any() and (s.labels[:, 37, w - 1] == 1).all() and (s.labels[:, 37, :64] == 5).any()
        assert not s.labels[:, 1:9:2, 64:128].any() and not s.labels[:, 25:32:2, 64:128].any() and (s.labels[:, 0:31:2, 64:128] == 2).any(-1).all()
        assert all((s.labels[:, ys, xs] == 3).any() for ys in (slice(0, 16), slice(16, 32)) for xs in (slice(0, 64), slice(64, 128)))
        assert not np.array_equal(s.labels[0], s.labels[1]) and not np.array_equal(s.labels[1], s.labels[2])
        if s.reg_labels is not None:
            for bi, xs in itertools.product(range(s.b), (slice(0, 64), slice(64, 128), slice(128, w))):
                a, r = s.labels[bi, :, xs] > 0, s.reg_labels[bi, :, xs] > 0
                assert (a & r).any() and (a & ~r).any() and (~a & r).any() and (~a & ~r).any()
            assert s.reg_labels.max() <= objects
