"""tests/ransac_reference.py (the fp64 restatement the GPU stage tests compare with) pinned against the fp32 oracle, on the CPU: its count
intervals contain the oracle's counts, its hypotheses agree with the oracle's to the conditioning of the 2x2 solve, and its round update and
refinement reproduce ransac_voting_single."""
import numpy as np

import casapose_oracle as O
import ransac_reference as R

THRESH = 0.99


def _objects():
    labels, field, _ = R.common_input(0)
    draws = R.common_draws(1, 1, 48)[0]
    for bi in range(R.B):
        for o in range(R.OBJECTS):
            pix = R.pixel_list(labels[bi], o)
            if pix.size >= 5:
                direct, coords = R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
                yield bi, o, pix, direct, coords, (draws[bi, o].astype(np.int64) % pix.size)


def test_common_input_is_what_the_stage_tests_assume():
    labels, field, _ = R.common_input(0)
    counts = [[int((labels[bi] == o + 1).sum()) for o in range(R.OBJECTS)] for bi in range(R.B)]
    assert counts == [[6164 - 529, 64, 529, 0], [6164 - 529, 64, 529, 4]]
    assert not np.array_equal(labels[0], labels[1])
    fg = labels > 0
    chan = np.zeros(R.LD, bool)
    chan[R.DIR_OFF:R.DIR_OFF + 18] = True
    assert np.isnan(field[~fg]).all() and np.isnan(field[fg][:, ~chan]).all() and np.isfinite(field[fg][:, chan]).all()
    rec = field[fg][:, chan].reshape(-1, 9, 2)
    length = np.sqrt((rec.astype(np.float64) ** 2).sum(-1))
    assert length.min() < 0.6 and length.max() > 1.9 and length.min() >= 0.49
    d = R.common_draws(1, 1, 16)
    assert d.dtype == np.int32 and d.min() >= 0 and d.max() > 2 ** 30


def test_count_intervals_contain_the_fp32_oracle_counts():
    pairs = exact = band = tests = 0
    for bi, o, pix, direct, coords, idx in _objects():
        hyp = O.ransac_generate_hypothesis(direct, coords, idx)
        got = O.ransac_vote(direct, coords, hyp, np.float32(THRESH)).sum(1)
        lo, hi, bm = R.count_bounds(direct, coords, hyp, THRESH)
        assert ((lo <= got) & (got <= hi)).all(), (bi, o)
        assert (hi - lo == bm.sum(1)).all()
        pairs += lo.size
        exact += int((lo == hi).sum())
        band += int(bm.sum())
        tests += bm.size
        print("image %d object %d: %d px, best inlier ratios %.2f-%.2f" % (bi, o, pix.size, (got.max(0) / pix.size).min(), (got.max(0) / pix.size).max()))
    print("band share %.2e, exact pairs %.1f %% of %d" % (band / tests, 100.0 * exact / pairs, pairs))
    assert pairs == 6 * 48 * 9 and band / tests <= 1e-3 and exact / pairs >= 0.85


def test_hypotheses_agree_with_the_oracle_to_the_conditioning():
    for bi, o, pix, direct, coords, idx in _objects():
        idx = idx.copy()
        idx[:4, :, 1] = idx[:4, :, 0]                      # the same pixel twice: det == 0
        got = O.ransac_generate_hypothesis(direct, coords, idx).astype(np.float64)
        pts, det = R.hypotheses(direct, coords, idx)
        assert (det[:4] == 0).all() and not got[:4].any() and not pts[:4].any()
        ok, zero = det > 1.5e-6, det < 5e-7                # the fp32 determinant of two vectors of length <= 2 carries up to 5e-7 of rounding
        assert (ok | zero).all() and ok.sum() > 0.9 * ok.size and not got[zero].any()
        tol = 1e-5 * (1 + np.sqrt((pts ** 2).sum(-1))) / np.maximum(det, 1e-300)
        assert (np.abs(got - pts).max(-1)[ok] <= tol[ok]).all(), (bi, o)


def test_rounds_and_refinement_reproduce_the_oracle():
    labels, field, _ = R.common_input(0)
    rounds, hyp, conf = 4, 16, 0.99
    draws = R.common_draws(2, rounds, hyp)
    seen = set()
    for bi in range(R.B):
        for o in range(3):
            pix = R.pixel_list(labels[bi], o)
            direct, coords = R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
            idxs = [draws[r, bi, o].astype(np.int64) % pix.size for r in range(rounds)]
            vert = np.nan_to_num(field[bi][:, :, R.DIR_OFF:R.DIR_OFF + 18]).reshape(R.H, R.W, 9, 2)
            want, want_rounds = O.ransac_voting_single(labels[bi] == o + 1, vert, idxs, THRESH, conf, rounds)
            s, hyps = R.new_state(pix.size), []
            while not s["done"]:
                hyps.append(O.ransac_generate_hypothesis(direct, coords, idxs[s["rounds"]]))
                s = R.round_update(s, O.ransac_vote(direct, coords, hyps[-1], np.float32(THRESH)).sum(1), conf, rounds)
            assert s["rounds"] == want_rounds
            seen.add(want_rounds)
            win = np.stack([hyps[r][i, v] for v, (r, i) in enumerate(s["win_at"])])
            inl = O.ransac_vote(direct, coords, win[None], np.float32(THRESH))[0].astype(bool)
            got, refined, cond = R.solve(R.normal_sums(direct, coords, inl), win)
            assert refined and np.abs(got - want).max() <= 1e-4 * (1 + np.abs(want).max()), (bi, o, cond)
    assert len(seen) > 1
