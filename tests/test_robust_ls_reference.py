"""tests/robust_ls_reference.py on the CPU: that it restates ls_reference where no weight is given, that two reweighted passes take back the
error the stray pixels of a split cause on the touching discs of tests/test_gpu_vote_split_e2e.py (exact field and directions turned by
N(0, 0.05 rad)), and the three cases of the solve rule: no pass, a rank-one slot, a slot that loses more than 7/8 of its weight.  No GPU.

Measured here, fp64 reference, slot map of vote_split_reference.split_labels, cut-off 4 px, worst keypoint against the planted ones in px:
    scene                     plain LS   pass 1   pass 2   pass 4
    touch2, exact field       1.16       0.0335   0.0334   0.0334
    touch3, exact field       1.84       0.0469   0.0465   0.0465
    touch2, noise (seed 7)    1.21       0.169    0.103    0.0986
    touch3, noise (seed 7)    1.89       0.283    0.154    0.146
The fp32-order restatement gives the same figures to three digits."""
import functools

import numpy as np
import pytest

import ls_reference as L
import robust_ls_reference as RL
from test_gpu_ls_slots import slot_map_of
from test_gpu_vote_split_e2e import KP, NAMES, OBJECTS, R, reference_chain, scene

CUTOFF = 4.0
NOISE, NOISE_SEED = 0.05, 7


@functools.lru_cache(maxsize=None)
def touching(name, noisy):
    """(record [1,h,w,36], slot map, planted keypoints per disc, rank of every disc); noisy: every direction turned by N(0, 0.05 rad)"""
    rec, _, _, _, _, planted = scene(name)
    slots, _, _, _, _, ranks = reference_chain(name)       # the split is made on the exact field in both cases: the same stray pixels
    if noisy:
        rng = np.random.default_rng(NOISE_SEED)
        h, w = rec.shape[1:3]
        d = rec[0, :, :, 9:27].reshape(h, w, KP, 2).astype(np.float64)
        ang = np.arctan2(d[..., 0], d[..., 1]) + rng.normal(0.0, NOISE, d.shape[:3])
        length = np.sqrt((d * d).sum(-1))
        rec = rec.copy()
        rec[0, :, :, 9:27] = (np.stack([np.sin(ang), np.cos(ang)], -1) * length[..., None]).reshape(h, w, 2 * KP).astype(np.float32)
    return rec, slots, [yx for _, yx in planted], ranks


def worst(kps, planted, ranks):
    k = kps.reshape(1, OBJECTS, R, KP, 2)
    return max(float(np.abs(k[0, 0, ranks[i]] - yx).max()) for i, yx in enumerate(planted))


@functools.lru_cache(maxsize=None)
def chain(name, noisy, order, passes=4):
    rec, slots, _, _ = touching(name, noisy)
    return RL.run(rec, 36, 9, 27, 0, slots, OBJECTS * R, CUTOFF, passes, order)


def test_without_a_weight_the_terms_are_ls_reference_bit_for_bit():
    s = L.scene(139, **L.LAYOUTS["rec40"])
    for sigmoid in (0, 1):
        want = L.terms(s.field, s.ld, s.dir_off, s.conf_off, sigmoid, s.h)
        got = RL.weighted_terms(s.field, s.ld, s.dir_off, s.conf_off, sigmoid, s.h)
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True)
    one = np.ones(s.field.shape[:3] + (KP,))
    got = RL.weighted_terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h, one.astype(np.float32), one)
    for a, b in zip(got, L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)):
        assert np.array_equal(a, b, equal_nan=True)          # rho = 1 changes nothing


def test_the_weight_by_hand():
    """one pixel at (y, x) = (10, 20) of a 40-row image pointing along +x, estimates 0, 2, 4 and 6 px beside its line and one behind it"""
    field = np.zeros((1, 40, 64, 4), np.float32)
    field[0, 10, 20, 0:2] = (0.0, 3.0)
    field[0, 10, 21, 0:2] = (0.0, 0.0)                  # a zero direction
    sm = np.zeros((1, 40, 64), np.uint8)
    sm[0, 10, 20:22] = 1
    for dt in (np.float32, np.float64):
        for off, want in ((0.0, 1.0), (2.0, 0.5625), (-2.0, 0.5625), (4.0, 0.0), (6.0, 0.0)):
            for ahead in (30.5, 2.5):                   # before and behind the pixel: lines, not rays
                est = np.array([[[[10.5 + off, ahead]]]], np.float32)
                r = RL.rho(field, 0, sm, est, 40, 4.0, dt, kp=1)
                assert r.dtype == dt and abs(float(r[0, 10, 20, 0]) - want) < 1e-5, (dt, off, ahead, r[0, 10, 20, 0])
                assert r[0, 10, 21, 0] == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_two_passes_take_the_stray_pixels_out_on_the_exact_field(name):
    _, _, planted, ranks = touching(name, False)
    for order in ("fp64", "fp32"):
        c = chain(name, False, order)
        errs = [worst(k, planted, ranks) for k in c.kps]
        print("%s exact, %s: plain %.3g px, pass 1 %.3g, pass 2 %.3g, pass 4 %.3g" % (name, order, errs[0], errs[1], errs[2], errs[4]))
        assert errs[0] > 1.0                              # what the split costs the plain voter (1.16 / 1.84 px)
        assert errs[2] <= 0.05 and errs[1] <= 0.05 and errs[4] <= errs[2] * 1.001
        assert all(t[0, np.asarray(ranks)].all() for t in c.took)      # the found instances took every pass
    # what is left is the strays whose lines pass within the cut-off, not rounding: both orders agree
    assert np.abs(chain(name, False, "fp64").kps[2] - chain(name, False, "fp32").kps[2]).max() < 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_two_passes_halve_the_error_under_direction_noise(name):
    _, _, planted, ranks = touching(name, True)
    c = chain(name, True, "fp64")
    errs = [worst(k, planted, ranks) for k in c.kps]
    print("%s noise: plain %.3g px, pass 1 %.3g, pass 2 %.3g, pass 4 %.3g" % (name, errs[0], errs[1], errs[2], errs[4]))
    assert errs[2] < 0.5 * errs[0]


def test_no_pass_is_the_plain_solve():
    s = L.scene(136, **L.LAYOUTS["rec36"])
    sm = slot_map_of(s.labels, 32)
    c = RL.run(s.field, s.ld, s.dir_off, s.conf_off, 0, sm, 32, CUTOFF, 0)
    t64 = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)[1]
    assert len(c.kps) == 1 and not c.sums and np.array_equal(c.kps[0], L.solve(L.sums(t64, sm, 32)[0], s.h))


def test_a_rank_one_slot_keeps_its_plain_value():
    s = L.scene(136, rank_one=True, **L.LAYOUTS["rec36"])
    sm = slot_map_of(s.labels, 8)
    c = RL.run(s.field, s.ld, s.dir_off, s.conf_off, 0, sm, 8, CUTOFF, 2)
    (o,) = np.unique(sm[s.labels == L.RANK_ONE]) - 1          # at 8 slots object 5 sits in the table's last row
    assert np.isinf(L.condition(c.plain[0][:, o])).all() or (L.condition(c.plain[0][:, o]) > 1e12).all()
    assert c.plain[1][:, o].any() and c.sums[0][1][:, o].any()              # the slot has pixels and they keep weight: it is the rank that refuses
    assert not c.took[0][:, o].any() and not c.took[1][:, o].any()
    assert np.array_equal(c.kps[2][:, o], c.kps[0][:, o]) and np.abs(c.kps[0][:, o]).max() > 0
    assert c.took[0][:, :4].any()                                       # elsewhere passes are taken
    empty = ~c.plain[1].any((0, 2, 3))
    assert empty.sum() == 3 and not c.kps[2][:, empty].any() and not c.sums[1][0][:, empty].any()


def test_a_slot_that_loses_seven_eighths_of_its_weight_keeps_the_previous_value():
    """at a cut-off of 0.3 px most of the noisy scene's lines miss the estimate: many systems keep less than 1/8 of their weight and fall back;
    the rule has no state, so the next pass decides the same"""
    s = L.scene(139, **L.LAYOUTS["rec36"])
    sm = slot_map_of(s.labels, 32)
    c = RL.run(s.field, s.ld, s.dir_off, s.conf_off, 0, sm, 32, 0.3, 2)
    share = RL.kept(c.sums[0][0], c.plain[0])
    present = c.plain[1].any(-1)
    lost = present & (share < RL.MIN_KEPT)
    held = present & (share >= RL.MIN_KEPT) & (L.condition(c.sums[0][0]) < 1e5)
    assert lost.sum() >= 10 and held.sum() >= 10
    assert not c.took[0][lost].any() and np.array_equal(c.kps[1][lost], c.kps[0][lost])
    assert c.took[0][held].all() and (c.kps[1][held] != c.kps[0][held]).any(-1).all()
    assert not c.took[1][lost].any() and np.array_equal(c.kps[2][lost], c.kps[0][lost])
    assert np.array_equal(c.sums[1][0][lost], c.sums[0][0][lost])            # the same estimate, the same terms, the same sums
