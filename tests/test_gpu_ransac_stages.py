"""The RANSAC voter (csrc/ransac_vote.hip) checked stage by stage: the C ABI is called directly, the intermediate products are read out of the
caller's workspace through cp_ransac_workspace_layout and compared with the fp64 restatement of tests/ransac_reference.py -- compaction,
hypotheses, inlier counts (both vote_kernel instantiations), crafted edge cases, the round update and stopping rule, the refinement and its
fallback, and the seeded entry's thinning.  Every condition a check needs of its INPUT is asserted on the reference before the kernel's result is
looked at."""
import ctypes as C
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import casapose_oracle as O
import ransac_reference as R

pytestmark = pytest.mark.gpu

THRESH, MIN_NUM = 0.99, 5
STATE = np.dtype([("tn", "<i4"), ("done", "<i4"), ("rounds", "<i4"), ("hyp_num", "<f4"), ("win_ratio", "<f4", (9,)), ("win_pts", "<f4", (9, 2))])


def vote(lib, device, labels, field, dir_off, objects, hyp, thresh=THRESH, confidence=0.99, max_iter=1, min_num=MIN_NUM, max_num=30000,
         draws=None, seed=None):
    """One call of cp_ransac_vote_f32 (draws given) or cp_ransac_vote_seeded_f32 (seed given); everything it left behind, as NumPy arrays."""
    from casapose_amd import _lib

    b, h, w = labels.shape
    ld = field.shape[-1]
    offs, state_bytes = (C.c_size_t * 7)(), C.c_size_t()
    _lib.check(lib.cp_ransac_workspace_layout(b, h, w, objects, 9, hyp, offs, C.byref(state_bytes)), "cp_ransac_workspace_layout")
    assert state_bytes.value == STATE.itemsize == C.sizeof(_lib.RansacState)
    nbytes = lib.cp_ransac_workspace_bytes(b, h, w, objects, 9, hyp)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    assert ws.data_ptr() % 256 == 0
    lab_d, fld_d = torch.from_numpy(labels).to(device), torch.from_numpy(field).to(device)
    out = torch.full((b, objects, 9, 2), 7.0, dtype=torch.float32, device=device)
    rounds = torch.full((b, objects), -1, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    head = (lab_d.data_ptr(), fld_d.data_ptr(), ld, dir_off, b, h, w, objects, 9)
    tail = (hyp, float(thresh), float(confidence), int(max_iter), int(min_num), int(max_num), ws.data_ptr(), out.data_ptr(), rounds.data_ptr(), stream)
    if draws is not None:
        assert draws.dtype == np.int32 and draws.shape[1:] == (b, objects, hyp, 9, 2) and draws.shape[0] >= max_iter
        dr_d = torch.from_numpy(np.ascontiguousarray(draws)).to(device)
        _lib.check(lib.cp_ransac_vote_f32(*head, dr_d.data_ptr(), *tail), "cp_ransac_vote_f32")
    else:
        _lib.check(lib.cp_ransac_vote_seeded_f32(*head, int(seed), *tail), "cp_ransac_vote_seeded_f32")
    torch.cuda.synchronize(device)
    raw = ws.cpu().numpy()

    def part(i, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert offs[i] % 256 == 0 and offs[i] + n <= nbytes and all(offs[i] + n <= offs[j] for j in range(7) if offs[j] > offs[i])
        return raw[offs[i]:offs[i] + n].view(dtype).reshape(shape).copy()

    return SimpleNamespace(out=out.cpu().numpy(), rounds=rounds.cpu().numpy(), pixlist=part(1, "<i4", (b, objects, h * w)),
                           st=part(2, STATE, (b, objects)), hyp_pts=part(3, "<f4", (b, objects, hyp, 9, 2)), counts=part(4, "<i4", (b, objects, hyp, 9)),
                           sums=part(5, "<f8", (b, objects, 9, 5)), thr=part(6, "<u4", (b, objects)))


@functools.lru_cache(maxsize=None)
def common():
    labels, field, _ = R.common_input(0)
    objs = {}
    for bi, o in itertools.product(range(R.B), range(R.OBJECTS)):
        pix = R.pixel_list(labels[bi], o)
        if pix.size >= MIN_NUM:
            objs[bi, o] = (pix,) + R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
    assert sorted(objs) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    return labels, field, objs


@functools.lru_cache(maxsize=None)
def stage_draws(hyp):
    """Round-1 draws of the hypothesis / count tests: the first 48 hypotheses are the same for hyp = 48 and 64; hypotheses 0 and 1 of every object
    draw one pixel twice (det = 0)."""
    d = R.common_draws(100 + hyp, 1, hyp)
    if hyp == 64:
        d[:, :, :, :48] = stage_draws(48)
    d[:, :, :, :2, :, 1] = d[:, :, :, :2, :, 0]
    return d


@pytest.fixture(scope="module")
def stage_runs(hip_lib, device):
    labels, field, _ = common()
    return {hyp: vote(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, hyp, draws=stage_draws(hyp)) for hyp in (16, 48, 64)}


# ---- b. compaction ----------------------------------------------------------------------------------------------------------------------------------
def test_compaction_lists_every_object_in_raster_order(stage_runs):
    labels, _, objs = common()
    r = stage_runs[16]
    for bi, o in itertools.product(range(R.B), range(R.OBJECTS)):
        st = r.st[bi, o]
        if (bi, o) in objs:
            pix = objs[bi, o][0]
            assert st["tn"] == pix.size and np.array_equal(r.pixlist[bi, o, :pix.size], pix), (bi, o)
            assert st["rounds"] == 1 == r.rounds[bi, o] and st["done"] == 1 and st["hyp_num"] == 16.0
        else:   # absent, or below min_num
            assert int((labels[bi] == o + 1).sum()) in (0, 4)
            assert st["tn"] == 0 and st["done"] == 1 and st["rounds"] == 0 == r.rounds[bi, o] and not r.out[bi, o].any(), (bi, o)
    assert np.isfinite(r.out).all()       # no NaN of the other channels or of the background reached the result


@pytest.mark.parametrize("objects", [1, 4, 70])
def test_mask_to_labels_matches_numpy(hip_lib, device, objects):
    from casapose_amd import _lib

    b, h, w = 2, 19, 23                    # 437 pixels: one full block of 256 and a ragged one
    rng = np.random.default_rng(objects)
    mask = rng.choice(np.array([0.0, 0.25, 0.5 - 2.0 ** -25, 0.5, 0.5 + 2.0 ** -24, 0.75, 1.0], np.float32), (b, h, w, objects),
                      p=[0.5, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05]).astype(np.float32)       # overlapping channels; 0.5 itself is outside
    mask[:, ::3, ::4] = np.minimum(mask[:, ::3, ::4], np.float32(0.5))                  # some pixels inside no object at all
    assert np.float32(0.5 - 2.0 ** -25) < 0.5 < np.float32(0.5 + 2.0 ** -24) and (mask == 0.5).any()
    inside = mask > np.float32(0.5)
    want_labels = np.where(inside.any(-1), objects - np.argmax(inside[..., ::-1], -1), 0).astype(np.uint8)     # the highest channel inside, + 1
    want_counts = inside.sum((1, 2)).astype(np.int32)
    if objects > 1:
        assert (inside.sum(-1) > 1).any() and (inside.sum(-1) == 0).any()
    m = torch.from_numpy(mask).to(device)
    lab = torch.full((b, h, w), 255, dtype=torch.uint8, device=device)
    cnt = torch.full((b, objects), -1, dtype=torch.int32, device=device)
    _lib.check(hip_lib.cp_mask_to_labels_f32(m.data_ptr(), b, h, w, objects, lab.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    assert np.array_equal(lab.cpu().numpy(), want_labels) and np.array_equal(cnt.cpu().numpy(), want_counts)


# ---- c. hypotheses ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyp", [16, 48, 64])
def test_hypotheses_match_fp64_to_their_conditioning(stage_runs, hyp):
    _, _, objs = common()
    zeros = 0
    for (bi, o), (pix, direct, coords) in objs.items():
        idx = stage_draws(hyp)[0, bi, o].astype(np.int64) % pix.size
        pts, det = R.hypotheses(direct, coords, idx)
        fires, clear = det < 5e-7, det > 1.5e-6          # the fp32 determinant carries up to 5e-7 of rounding: nothing may lie between
        assert (fires | clear).all() and fires[:2].all() and clear.sum() > 0.8 * clear.size
        got = stage_runs[hyp].hyp_pts[bi, o].astype(np.float64)
        assert not got[fires].any(), (bi, o)             # exactly (0, 0)
        tol = 1e-5 * (1 + np.sqrt((pts ** 2).sum(-1))) / np.maximum(det, 1e-6)
        err = np.abs(got - pts).max(-1)
        assert (err[clear] <= tol[clear]).all(), (bi, o, float((err[clear] / tol[clear]).max()))
        zeros += int(fires.sum())
    assert zeros >= 6 * 2 * 9


# ---- d. counts ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyp", [16, 48, 64])
def test_counts_lie_in_the_fp64_intervals(stage_runs, hyp):
    _, _, objs = common()
    band = tests = exact = pairs = 0
    for (bi, o), (pix, direct, coords) in objs.items():          # the input's conditions, on the reference's own hypotheses
        hp, _, _ = R.hypotheses_f32(direct, coords, stage_draws(hyp)[0, bi, o].astype(np.int64) % pix.size)
        lo, hi, bm = R.count_bounds(direct, coords, hp, THRESH)
        band, tests, exact, pairs = band + int(bm.sum()), tests + bm.size, exact + int((lo == hi).sum()), pairs + lo.size
    print("hyp %d: band share %.2e of %d pixel tests, %.1f %% of %d (hypothesis, keypoint) pairs checked exactly" % (hyp, band / tests, tests, 100.0 * exact / pairs, pairs))
    assert band / tests <= 1e-3 and exact / pairs >= 0.85
    r = stage_runs[hyp]
    for (bi, o), (pix, direct, coords) in objs.items():
        lo, hi, _ = R.count_bounds(direct, coords, r.hyp_pts[bi, o], THRESH)     # the kernel's own hypotheses (checked in c)
        got = r.counts[bi, o]
        bad = (got < lo) | (got > hi)
        assert not bad.any(), (bi, o, np.argwhere(bad)[:5], got[bad][:5], lo[bad][:5], hi[bad][:5])


def test_both_vote_kernels_count_the_same(stage_runs):
    """hyp = 48 runs vote_kernel<16>, hyp = 64 vote_kernel<64>; the first 48 hypotheses have the same draws: same pixels, same hypotheses,
    integer counts -- bit for bit."""
    _, _, objs = common()
    for bi, o in objs:
        assert np.array_equal(stage_runs[64].hyp_pts[bi, o, :48], stage_runs[48].hyp_pts[bi, o])
        assert np.array_equal(stage_runs[64].counts[bi, o, :48], stage_runs[48].counts[bi, o]), (bi, o)
        assert stage_runs[48].counts[bi, o].max() > 0.2 * objs[bi, o][0].size


# ---- e. crafted edges -----------------------------------------------------------------------------------------------------------------------------------
EH, EW = 12, 16     # one object that fills a 12 x 16 image: position t in its pixel list is pixel t


def _toward(target, noise=0.0, rng=None, length=None):
    """(dy, dx) [EH*EW, 2] pointing from every pixel centre at `target` (x, y)."""
    ys, xs = np.divmod(np.arange(EH * EW), EW)
    ang = np.arctan2(target[1] - (ys + 0.5), target[0] - (xs + 0.5))
    if rng is not None:
        ang = ang + rng.normal(0, noise, ang.shape)
    length = np.ones_like(ang) if length is None else length
    return np.stack([length * np.sin(ang), length * np.cos(ang)], -1)


@functools.lru_cache(maxsize=None)
def edge_input():
    rng = np.random.default_rng(5)
    rec = np.zeros((EH * EW, 9, 2))
    targets = [(6.3, 4.1), (-3.0, 3.0), (9.2, 7.7), (4.4, 8.3), (11.1, 2.2), (2.7, 5.6), (7.9, 9.4), (13.3, 6.1), (5.2, 1.8)]
    for v, t in enumerate(targets):
        rec[:, v] = _toward(t, 0.1 if v != 1 else 0.0, rng, rng.uniform(0.5, 2.0, EH * EW))
    draws = rng.integers(0, 2 ** 31, (1, 1, 1, 16, 9, 2), dtype=np.int64)
    pix = lambda x, y: y * EW + x   # noqa: E731
    # keypoint 0, hypothesis 0: rays from pixel (2,7) along (1,0) and from pixel (10,8) along (-2^-20, 1) meet at (10.5 + 2^-20, 7.5), exactly in
    # fp32; pixel (10,7) under it points along (1,0) at it: cosine 1, but |e| = 9.5e-7 <= 1e-6
    rec[pix(2, 7), 0], rec[pix(10, 8), 0], rec[pix(10, 7), 0] = (0.0, 1.0), (1.0, -2.0 ** -20), (0.0, 1.0)
    draws[0, 0, 0, 0, 0] = (pix(2, 7) + 3 * EH * EW, pix(10, 8))
    # keypoint 1: the field points exactly at (-3, 3); hypothesis 1 is exactly (-3, 3) (rays (-5.5,-0.5) from (2.5,3.5) and (-3.5,-3.5) from (0.5,6.5)):
    # hx + hy = 0, no inliers although every pixel points at it
    rec[pix(2, 3), 1], rec[pix(0, 6), 1] = (-0.5, -5.5), (-3.5, -3.5)
    draws[0, 0, 0, 1, 1] = (pix(2, 3), pix(0, 6))
    # keypoint 2: only the first two rows have directions; every other pixel points exactly at the target with length 5e-7 or is (0,0)
    tiny = _toward(targets[2]) * 5e-7
    tiny[::2] = 0.0
    rec[2 * EW:, 2] = tiny[2 * EW:]
    draws[0, 0, 0, :, 2] = rng.integers(0, 2 * EW, (16, 2))
    field = rec.reshape(1, EH, EW, 18).astype(np.float32)
    return np.ones((1, EH, EW), np.uint8), field, draws.astype(np.int32)


def _edge_records():
    labels, field, draws = edge_input()
    pix = R.pixel_list(labels[0], 0)
    return (pix,) + R.pixel_records(field[0], pix, EW, 0) + (draws[0, 0, 0].astype(np.int64) % pix.size,)


def test_crafted_edges_follow_the_reference(hip_lib, device):
    labels, field, draws = edge_input()
    pix, direct, coords, idx = _edge_records()
    # the reference's answers, from the fp32 oracle on the CPU
    ohyp = O.ransac_generate_hypothesis(direct, coords, idx)
    ocnt = O.ransac_vote(direct, coords, ohyp, np.float32(THRESH)).sum(1)
    under = 7 * EW + 10
    assert tuple(ohyp[0, 0]) == (np.float32(10.5 + 2.0 ** -20), np.float32(7.5))                                        # case 1
    assert O.ransac_vote(direct, coords, ohyp, np.float32(THRESH))[0, under, 0] == 0
    e = ohyp[0, 0] - coords[under]
    assert (direct[under, 0] * e).sum() ** 2 > THRESH ** 2 * (direct[under, 0] ** 2).sum() * (e ** 2).sum() > 0           # the squared form says inlier
    assert tuple(ohyp[1, 1]) == (-3.0, 3.0) and ocnt[1, 1] == 0 and ocnt[:, 1].max() > 150                              # case 2
    assert (ocnt[:, 2] <= 2 * EW).all() and ocnt[:, 2].max() > 10                                                         # case 3
    plo, phi, _ = R.count_bounds(direct, coords, ohyp, THRESH)
    assert ((plo <= ocnt) & (ocnt <= phi)).all() and plo[0, 0] == phi[0, 0] and plo[1, 1] == phi[1, 1] == 0
    r = vote(hip_lib, device, labels, field, 0, 1, 16, draws=draws)
    assert r.st[0, 0]["tn"] == EH * EW
    got_h, got_c = r.hyp_pts[0, 0], r.counts[0, 0]
    assert np.array_equal(got_h[0, 0], ohyp[0, 0]) and np.array_equal(got_h[1, 1], ohyp[1, 1])
    lo, hi, _ = R.count_bounds(direct, coords, got_h, THRESH)
    assert ((lo <= got_c) & (got_c <= hi)).all(), np.argwhere((got_c < lo) | (got_c > hi))
    assert got_c[0, 0] == ocnt[0, 0] and got_c[1, 1] == 0
    assert (got_c[:, 2] <= 2 * EW).all() and got_c[:, 2].max() > 10
    print("crafted edges confirmed with the fp32 oracle: 3 (hypothesis on a pixel centre, hx + hy = 0, directions below 1e-6)")


def test_negative_threshold_takes_the_reference_expression(hip_lib, device):
    """inlier_thresh = -0.5: the squared inequality does not apply, every test is the reference's own expression."""
    labels, field, draws = edge_input()
    pix, direct, coords, idx = _edge_records()
    ohyp = O.ransac_generate_hypothesis(direct, coords, idx)
    ocnt = O.ransac_vote(direct, coords, ohyp, np.float32(-0.5)).sum(1)
    plo, phi, _ = R.count_bounds(direct, coords, ohyp, -0.5)
    assert ((plo <= ocnt) & (ocnt <= phi)).all() and (plo == phi).mean() >= 0.85
    assert ocnt[1, 1] == 0 and (ocnt[:, 2] <= 2 * EW).all()
    assert (ocnt[:, 3:] > O.ransac_vote(direct, coords, ohyp, np.float32(THRESH)).sum(1)[:, 3:]).any()      # the threshold matters
    r = vote(hip_lib, device, labels, field, 0, 1, 16, thresh=-0.5, draws=draws)
    lo, hi, _ = R.count_bounds(direct, coords, r.hyp_pts[0, 0], -0.5)
    got = r.counts[0, 0]
    assert ((lo <= got) & (got <= hi)).all(), np.argwhere((got < lo) | (got > hi))
    assert got[1, 1] == 0 and (got[:, 2] <= 2 * EW).all()


# per keypoint: the hypothesis indices that reach the maximum (every other hypothesis draws one pixel twice: invalid, no inliers)
TIES = {0: (70, 6), 1: (37, 38), 2: (100, 9), 3: (66, 3), 4: (127, 63, 64), 5: (0, 1), 6: (65, 1, 64), 7: (20,), 8: (64, 127)}
TIE_PIXELS = [((0, 0), (15, 0)), ((0, 11), (15, 11)), ((0, 5), (8, 11))]


def test_argmax_ties_go_to_the_lowest_index(hip_lib, device):
    """hyp = 128: equal maxima in one lane's stride (h, h + 64), in neighbouring lanes, and with the lower index in the higher lane."""
    hyp = 128
    rec = np.zeros((EH * EW, 9, 2))
    draws = np.repeat(np.random.default_rng(6).integers(0, 2 ** 31, (1, 1, 1, hyp, 9, 1), dtype=np.int64), 2, -1)     # one pixel twice
    want_pts = {}
    for v, tied in TIES.items():
        target = np.array([4.0 + v, 3.0 + (v % 4)])           # a pixel corner: every centre is >= 0.7 px away
        rec[:, v] = _toward(target)
        for k, hidx in enumerate(tied):                       # tied hypothesis k: two pixels that point at target + delta_k
            for (x, y) in TIE_PIXELS[k]:
                p = target + (0.004 * (k + 1), -0.003 * (k + 1))
                a = np.arctan2(p[1] - (y + 0.5), p[0] - (x + 0.5))
                rec[y * EW + x, v] = (1.5 * np.sin(a), 1.5 * np.cos(a))
            draws[0, 0, 0, hidx, v] = [y * EW + x for (x, y) in TIE_PIXELS[k]]
            want_pts[v, hidx] = p
    labels, field, draws = np.ones((1, EH, EW), np.uint8), rec.reshape(1, EH, EW, 18).astype(np.float32), draws.astype(np.int32)
    pix = R.pixel_list(labels[0], 0)
    direct, coords = R.pixel_records(field[0], pix, EW, 0)
    idx = draws[0, 0, 0].astype(np.int64) % pix.size
    ohyp = O.ransac_generate_hypothesis(direct, coords, idx)                 # the reference's answer on the CPU
    ocnt = O.ransac_vote(direct, coords, ohyp, np.float32(THRESH)).sum(1)
    for v, tied in TIES.items():
        assert (ocnt[list(tied), v] == EH * EW).all() and (np.delete(ocnt[:, v], tied) == 0).all()
        assert ocnt[:, v].argmax() == min(tied)
        assert len({tuple(ohyp[hi, v]) for hi in tied}) == len(tied)          # different hypotheses
        for hi in tied:
            assert np.abs(ohyp[hi, v] - want_pts[v, hi]).max() < 1e-4
    r = vote(hip_lib, device, labels, field, 0, 1, hyp, draws=draws)
    lo, hi_, _ = R.count_bounds(direct, coords, r.hyp_pts[0, 0], THRESH)
    assert np.array_equal(lo, hi_) and np.array_equal(r.counts[0, 0], lo) and np.array_equal(lo, ocnt)
    for v, tied in TIES.items():
        assert len({tuple(r.hyp_pts[0, 0, hi, v]) for hi in tied}) == len(tied)
        assert np.array_equal(r.st[0, 0]["win_pts"][v], r.hyp_pts[0, 0, min(tied), v]), (v, r.st[0, 0]["win_pts"][v])
        assert r.st[0, 0]["win_ratio"][v] == 1.0


# ---- f. rounds ------------------------------------------------------------------------------------------------------------------------------------------
F_THRESH, F_CONF, F_ITER, F_HYP, F_SEED = 0.995, 0.99, 6, 16, 20


@functools.lru_cache(maxsize=None)
def rounds_reference():
    _, _, objs = common()
    draws = R.common_draws(F_SEED, F_ITER, F_HYP)
    ref = {}
    for (bi, o), (pix, direct, coords) in objs.items():
        ref[bi, o] = R.reference_rounds(direct, coords, [draws[k, bi, o].astype(np.int64) % pix.size for k in range(F_ITER)], F_THRESH, F_CONF, F_ITER)
    return draws, ref


def test_rounds_winners_and_stopping_rule(hip_lib, device):
    labels, field, objs = common()
    draws, ref = rounds_reference()
    # conditions on the input, by the reference alone
    want_rounds = {k: v["rounds"] for k, v in ref.items()}
    print("reference rounds per (image, object):", want_rounds, "confidences:", {k: np.round(v["confs"], 4).tolist() for k, v in ref.items()})
    assert all(not v["problems"] for v in ref.values()), [v["problems"] for v in ref.values()]
    assert {1, F_ITER} <= set(want_rounds.values()) and set(want_rounds.values()) & {2, 3, 4, 5}
    runs = {m: vote(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, F_HYP, thresh=F_THRESH, confidence=F_CONF, max_iter=m, draws=draws)
            for m in range(1, F_ITER + 1)}
    final = runs[F_ITER]
    for (bi, o), (pix, direct, coords) in objs.items():
        want, st = ref[bi, o], final.st[bi, o]
        assert final.rounds[bi, o] == st["rounds"] == want["rounds"], (bi, o)
        assert st["hyp_num"] == F_HYP * want["rounds"] and st["done"] == 1
        assert (st["win_ratio"] >= want["ratio_lo"] - 1e-6).all() and (st["win_ratio"] <= want["ratio_hi"] + 1e-6).all(), (bi, o)
        for v, (rnd, hidx) in enumerate(want["win_at"]):
            # round rnd's hypotheses are what a call with max_iter = rnd + 1 leaves behind (the object was still voting in that round)
            hyp_then = runs[rnd + 1].hyp_pts[bi, o]
            pts, det = R.hypotheses(direct, coords, draws[rnd, bi, o].astype(np.int64) % pix.size)
            tol = 1e-5 * (1 + np.sqrt((pts[hidx, v] ** 2).sum())) / max(det[hidx, v], 1e-6)
            assert np.abs(hyp_then[hidx, v] - pts[hidx, v]).max() <= tol
            assert np.array_equal(st["win_pts"][v], hyp_then[hidx, v]), (bi, o, v)
        # a finished object's state does not change in later rounds
        then = runs[want["rounds"]]
        assert then.st[bi, o] == st and np.array_equal(then.out[bi, o], final.out[bi, o]), (bi, o)
        for m in range(1, F_ITER + 1):
            assert runs[m].rounds[bi, o] == min(m, want["rounds"])


# ---- g. refinement ----------------------------------------------------------------------------------------------------------------------------------------
def _check_sums(direct, coords, win_pts, sums, thresh):
    """sums [kp,5] = the terms over the definite inliers plus SOME subset of the undecided ones (at most 3 per keypoint, by condition)."""
    definite, possible = R.inlier_sets(direct, coords, win_pts[None], thresh)
    terms = R.normal_terms(direct, coords)
    for v in range(9):
        band = np.flatnonzero(possible[0, :, v] & ~definite[0, :, v])
        assert band.size <= 3, "undecided inliers of a winner: %d" % band.size
        base = terms[definite[0, :, v], v].sum(0)
        tol = 1e-6 * np.abs(terms[possible[0, :, v], v]).sum(0)      # the kernel forms each term in fp32 (<= 3 roundings, 2e-7 relative) and accumulates in fp64
        assert any((np.abs(base + terms[list(sub), v].sum(0) - sums[v]) <= tol).all()
                   for n in range(band.size + 1) for sub in itertools.combinations(band, n)), (v, base, sums[v], tol)


def test_refinement_sums_and_solution(stage_runs):
    _, _, objs = common()
    r = stage_runs[48]
    for (bi, o), (pix, direct, coords) in objs.items():
        st = r.st[bi, o]
        _check_sums(direct, coords, st["win_pts"], r.sums[bi, o], THRESH)
        want, refined, cond = R.solve(r.sums[bi, o], st["win_pts"])
        assert refined and not ((cond > 0.9e6) & (cond < 1.1e6)).any(), cond
        assert (np.abs(r.out[bi, o] - want) <= 2e-6 * (1 + np.abs(want))).all(), (bi, o)
        assert not np.array_equal(r.out[bi, o], st["win_pts"])


def test_refinement_falls_back_to_the_winners(hip_lib, device):
    """Keypoint 8 of one object has a constant direction field: every pair of rays is parallel, no hypothesis is valid, ATA is singular -- all nine
    outputs of THAT object are its winners, bit for bit; the other objects are still refined."""
    labels, field, objs = common()
    field = field.copy()
    fb = (1, 0)
    m = labels[fb[0]] == fb[1] + 1
    field[fb[0]][m, R.DIR_OFF + 16:R.DIR_OFF + 18] = (0.6, -0.8)
    r = vote(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, 16, draws=stage_draws(16))
    for (bi, o), (pix, _, coords) in objs.items():
        direct, _ = R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
        st = r.st[bi, o]
        want, refined, cond = R.solve(r.sums[bi, o], st["win_pts"])
        assert refined == ((bi, o) != fb)
        if (bi, o) == fb:
            assert not r.counts[bi, o][:, 8].any() and not r.hyp_pts[bi, o][:, 8].any() and st["win_ratio"][8] == 0 and not st["win_pts"][8].any()
            assert not r.sums[bi, o][8].any() and (st["win_ratio"][:8] > 0.3).all()
            assert np.array_equal(r.out[bi, o], st["win_pts"])
        else:
            assert (np.abs(r.out[bi, o] - want) <= 2e-6 * (1 + np.abs(want))).all() and not np.array_equal(r.out[bi, o], st["win_pts"])


# ---- h. seeded entry ----------------------------------------------------------------------------------------------------------------------------------------
def test_seeded_entry_thins_per_object_and_image(hip_lib, device):
    labels, field, objs = common()
    max_num = 400
    run = lambda seed, **kw: vote(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, 16, seed=seed, **{"max_num": max_num, **kw})   # noqa: E731
    a, a2, c = run(11), run(11), run(12)
    ranks = {}
    for bi, o in itertools.product(range(R.B), range(R.OBJECTS)):
        count = int((labels[bi] == o + 1).sum())
        st = a.st[bi, o]
        if count < MIN_NUM:
            assert a.thr[bi, o] == 0 and st["tn"] == 0 and not a.out[bi, o].any()
            continue
        pix = objs[bi, o][0]
        kept = a.pixlist[bi, o, :st["tn"]]
        if count <= max_num:
            assert a.thr[bi, o] == 0xFFFFFFFF and np.array_equal(kept, pix)
            continue
        assert a.thr[bi, o] == int(max_num / count * 4294967296.0)
        assert abs(int(st["tn"]) - max_num) <= 5 * np.sqrt(max_num * (1 - max_num / count)), (bi, o, st["tn"])       # binomial(count, max_num / count)
        assert (np.diff(kept) > 0).all() and np.isin(kept, pix).all()
        assert np.array_equal(kept, a2.pixlist[bi, o, :a2.st[bi, o]["tn"]]) and np.array_equal(a.out[bi, o], a2.out[bi, o])
        assert not np.array_equal(kept, c.pixlist[bi, o, :c.st[bi, o]["tn"]])
        ranks[bi, o] = np.searchsorted(pix, kept)
    assert sorted(ranks) == [(0, 0), (0, 2), (1, 0), (1, 2)]
    for o in (0, 2):     # the images thin independently: not the same positions of the (equally large) pixel lists
        assert not np.array_equal(ranks[0, o], ranks[1, o])
    # the min_num gate belongs to the un-thinned count: 64 >= 40 pixels are thinned to about 20 < 40 and still voted
    g = run(11, min_num=40, max_num=20)
    st = g.st[0, 1]
    assert 0 < st["tn"] < 40 and g.thr[0, 1] == int(20 / 64 * 4294967296.0) and st["rounds"] >= 1 and g.out[0, 1].any()
    assert g.thr[1, 3] == 0 and g.st[1, 3]["tn"] == 0
