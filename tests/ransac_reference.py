"""The RANSAC voter (csrc/ransac_vote.hip) restated stage by stage in plain fp64 NumPy, from the semantics of ransac_voting.py as
oracle/casapose_oracle.py states them (ransac_generate_hypothesis, ransac_vote, ransac_voting_single).  The inputs are the voter's fp32
values; every product, sum, root and quotient here is fp64, except where the reference itself rounds to fp32 on purpose (the inlier ratio
and the stopping rule, ATA / ATb before the solve).  tests/test_ransac_reference.py pins these functions against the fp32 oracle on the CPU,
tests/test_gpu_ransac_stages.py compares the kernels' intermediate products with them.

Conventions: object o is label o + 1; a pixel is y * w + x; coordinates are (x + 0.5, y + 0.5); the field stores (dy, dx) per keypoint and
the voter works in (dx, dy)."""
import numpy as np

KP = 9
EPS = 2e-6   # the kernel promises the decision of the reference's fp32 expression  ang = (d . e) / (|d| |e|) > t.  That expression -- two products
             # and a sum, two square roots, a product, a division, on values <= 1 -- differs from its fp64 value by well under 8 fp32 ulps of 1.0
             # (~1e-6); EPS doubles that.  Derived from the arithmetic, not measured on any implementation.


def pixel_list(labels_hw, o):
    """Pixels of object o in raster order (the order of tf.where)."""
    return np.flatnonzero(np.asarray(labels_hw).reshape(-1) == o + 1).astype(np.int64)


def pixel_records(field_hwc, pix, w, dir_off=0, kp=KP):
    """(direct [tn,kp,2] (dx,dy), coords [tn,2] (x,y)) of the listed pixels, in the field's own fp32."""
    pix = np.asarray(pix, np.int64)
    rec = field_hwc.reshape(-1, field_hwc.shape[-1])[pix, dir_off:dir_off + 2 * kp].reshape(-1, kp, 2)
    coords = np.stack([pix % w, pix // w], 1).astype(np.float32) + np.float32(0.5)
    return np.ascontiguousarray(rec[:, :, ::-1]), coords


def hypotheses(direct, coords, idx):
    """Two-ray intersections.  idx [hn,kp,2]: positions in the pixel list (already reduced mod tn).  Returns (pts [hn,kp,2], |det| [hn,kp]) in
    fp64; pts is the intersection wherever det != 0 (the caller applies the |det| <= 1e-6 -> (0,0) rule) and 0 where det == 0."""
    d, c = direct.astype(np.float64), coords.astype(np.float64)
    v = np.arange(idx.shape[1])[None, :]
    d0, d1 = d[idx[..., 0], v], d[idx[..., 1], v]       # [hn,kp,2]
    c0, c1 = c[idx[..., 0]], c[idx[..., 1]]
    det = d1[..., 0] * d0[..., 1] - d1[..., 1] * d0[..., 0]
    num = (c1[..., 1] - c0[..., 1]) * d1[..., 0] - (c1[..., 0] - c0[..., 0]) * d1[..., 1]
    ok = det != 0
    u = np.where(ok, num / np.where(ok, det, 1.0), 0.0)
    return np.where(ok[..., None], c0 + d0 * u[..., None], 0.0), np.abs(det)


def inlier_sets(direct, coords, hyp_pts, thresh, eps=EPS):
    """(definite, possible) inliers [hn,tn,kp] of hyp_pts [hn,kp,2] (fp32 values): ang > t + eps resp. ang > t - eps with ang in fp64 and the
    reference's validity rules |d| > 1e-6, |e| > 1e-6, |hx + hy| > 1e-6 (the last is one fp32 addition of the two stored coordinates: exact
    here; a length within 1e-5 relative of its 1e-6 limit counts as undecided)."""
    d, c = direct.astype(np.float64), coords.astype(np.float64)
    hp32 = np.asarray(hyp_pts, np.float32)
    hp = hp32.astype(np.float64)
    e = hp[:, None, :, :] - c[None, :, None, :]                    # [hn,tn,kp,2]
    ne = np.sqrt((e * e).sum(-1))
    nd = np.sqrt((d * d).sum(-1))[None]                            # [1,tn,kp]
    hsum_ok = (np.abs(hp32[..., 0] + hp32[..., 1]) > np.float32(1e-6))[:, None, :]
    lim, rel = 1e-6, 1e-5
    sure = (nd > lim * (1 + rel)) & (ne > lim * (1 + rel)) & hsum_ok
    maybe = (nd > lim * (1 - rel)) & (ne > lim * (1 - rel)) & hsum_ok
    with np.errstate(divide="ignore", invalid="ignore"):
        ang = np.where(maybe, (d[None] * e).sum(-1) / (nd * ne), -np.inf)
    return sure & (ang > thresh + eps), maybe & (ang > thresh - eps)


def count_bounds(direct, coords, hyp_pts, thresh, eps=EPS):
    """Bounds on the inlier counts: (lo [hn,kp], hi [hn,kp], band [hn,tn,kp]) = the numbers of definite and of possible inliers of inlier_sets,
    and the undecided tests between them."""
    inl_lo, inl_hi = inlier_sets(direct, coords, hyp_pts, thresh, eps)
    return inl_lo.sum(1), inl_hi.sum(1), inl_hi & ~inl_lo


def new_state(tn):
    return {"tn": int(tn), "done": tn == 0, "rounds": 0, "hyp_num": np.float32(0), "win_ratio": np.zeros(KP, np.float32),
            "win_at": np.full((KP, 2), -1), "conf": np.float32(0)}


def round_update(state, counts, confidence, max_iter):
    """One round of the best-so-far update on counts [hn,kp] (ransac_voting.py:325-347), in fp32 like the reference: per keypoint the lowest
    index among the maxima, replace the winner where win_ratio < ratio, then stop when 1 - (1 - min ratio^2)^hyps > confidence or after max_iter
    rounds.  state["win_at"][v] = (round, hypothesis index) of the current winner, (-1, -1) while there is none; state["conf"] the confidence."""
    s = dict(state)
    if s["done"]:
        return s
    counts = np.asarray(counts)
    widx = counts.argmax(axis=0)                                    # first maximum
    ratio = counts.max(axis=0).astype(np.float32) / np.float32(s["tn"])
    larger = s["win_ratio"] < ratio
    s["win_at"] = np.where(larger[:, None], np.stack([np.full(KP, s["rounds"]), widx], 1), s["win_at"])
    s["win_ratio"] = np.where(larger, ratio, s["win_ratio"]).astype(np.float32)
    s["hyp_num"] = np.float32(s["hyp_num"] + np.float32(counts.shape[0]))
    s["rounds"] += 1
    s["conf"] = _confidence(s["win_ratio"], s["hyp_num"])
    s["done"] = bool(s["conf"] > np.float32(confidence) or s["rounds"] >= max_iter)
    return s


def hypotheses_f32(direct, coords, idx):
    """The hypotheses as an fp32 implementation must store them: (pts fp32 [hn,kp,2] with (0,0) where |det| <= 1e-6, pos_tol [hn,kp], valid).
    pos_tol = 1e-5 (1 + |pt|) / max(|det|, 1e-6) is the distance an fp32 evaluation of the 2x2 solve may lie from the fp64 point.  The fp32
    determinant of two vectors of length <= 2 carries up to 5e-7 of rounding, so an input with 5e-7 <= |det| <= 1.5e-6 does not determine the
    rule's outcome: such an input is refused."""
    pts, det = hypotheses(direct, coords, idx)
    if not ((det > 1.5e-6) | (det < 5e-7)).all():
        raise ValueError("a determinant lies within rounding of the 1e-6 rule: choose other draws")
    valid = det > 1e-6
    tol = np.where(valid, 1e-5 * (1 + np.sqrt((pts ** 2).sum(-1))) / np.maximum(det, 1e-6), 0.0)
    return np.where(valid[..., None], pts, 0.0).astype(np.float32), tol, valid


def _confidence(ratio, hyp_num):
    mn = np.float32(ratio.min())
    return np.float32(1) - np.power(np.float32(1) - mn * mn, np.float32(hyp_num), dtype=np.float32)


def reference_rounds(direct, coords, idx_rounds, thresh, confidence, max_iter, eps=EPS):
    """The rounds of one object from the inputs alone: hypotheses_f32, count_bounds, and round_update's rules applied to the
    count INTERVALS.  Returns {"rounds", "win_at" [kp,2] (round, index), "ratio_lo", "ratio_hi" [kp] (fp32 bounds of win_ratio), "confs" (per
    round, from ratio_lo), "problems"}: problems lists every decision the intervals leave open (an arg-max another hypothesis' interval reaches, a
    best-so-far comparison of overlapping intervals, a stopping confidence within 1e-3 of `confidence`) -- an input is usable only if it is empty."""
    tn, kp = coords.shape[0], direct.shape[1]
    wlo, whi = np.zeros(kp, np.float32), np.zeros(kp, np.float32)
    win_at, hyp_num, rounds, confs, problems = np.full((kp, 2), -1), 0, 0, [], []
    while True:
        hp, tol, _ = hypotheses_f32(direct, coords, idx_rounds[rounds])
        lo, hi, _ = count_bounds(direct, coords, hp, thresh, eps)
        for v in range(kp):
            i = int(lo[:, v].argmax())
            if (hi[:i, v] >= lo[i, v]).any() or (hi[i + 1:, v] > lo[i, v]).any():
                problems.append("round %d keypoint %d: arg-max open" % (rounds, v))
            rlo, rhi = np.float32(lo[i, v]) / np.float32(tn), np.float32(hi[i, v]) / np.float32(tn)
            if whi[v] < rlo:
                wlo[v], whi[v], win_at[v] = rlo, rhi, (rounds, i)
            elif not wlo[v] >= rhi:
                problems.append("round %d keypoint %d: best-so-far comparison open" % (rounds, v))
        hyp_num += lo.shape[0]
        rounds += 1
        c_lo, c_hi = _confidence(wlo, hyp_num), _confidence(whi, hyp_num)
        confs.append(float(c_lo))
        if min(abs(c_lo - confidence), abs(c_hi - confidence)) < 1e-3 or (c_lo > confidence) != (c_hi > confidence):
            problems.append("round %d: confidence %.5f..%.5f too close to %g" % (rounds, c_lo, c_hi, confidence))
        if c_lo > np.float32(confidence) or rounds >= max_iter:
            return {"rounds": rounds, "win_at": win_at, "ratio_lo": wlo, "ratio_hi": whi, "confs": confs, "problems": problems}


def normal_terms(direct, coords):
    """Per pixel and keypoint the five terms of the normal equations [tn,kp,5] = (nx nx, nx ny, ny ny, nx b, ny b) with n = (-dy, dx) and
    b = n . c (:349-361), exact products of the fp32 inputs (an fp32 evaluation rounds each term up to three times)."""
    d, c = direct.astype(np.float64), coords.astype(np.float64)
    nx, ny = -d[..., 1], d[..., 0]
    b = nx * c[:, None, 0] + ny * c[:, None, 1]
    return np.stack([nx * nx, nx * ny, ny * ny, nx * b, ny * b], -1)


def normal_sums(direct, coords, inliers):
    """fp64 sums of the terms over inliers [tn,kp] (bool) -> [kp,5]."""
    return (normal_terms(direct, coords) * inliers[..., None]).sum(0)


def solve(sums, win_pts):
    """sums [kp,5] -> (keypoints [kp,2] fp32, refined?, cond [kp]): ATA and ATb rounded to fp32, the condition number from an fp64 SVD; if it is
    finite and < 1e6 for every keypoint the 2x2 solutions, else the winners unchanged (:267-272, :364)."""
    q = np.asarray(sums, np.float64).astype(np.float32).astype(np.float64)
    ata = np.stack([np.stack([q[:, 0], q[:, 1]], -1), np.stack([q[:, 1], q[:, 2]], -1)], -2)
    sv = np.linalg.svd(ata, compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = sv[:, 0] / sv[:, -1]
    if not np.all(np.isfinite(cond) & (cond < 1e6)):
        return np.asarray(win_pts, np.float32).copy(), False, cond
    return np.linalg.solve(ata, q[:, 3:, None])[..., 0].astype(np.float32), True, cond


# ---- the common input of the stage tests ---------------------------------------------------------------------------------------------------------
B, H, W, OBJECTS, LD, DIR_OFF = 2, 72, 100, 4, 40, 7
# per image: object -> (y0, x0, rows, cols, angular noise in rad, share of uniform outliers).  Two 64-row scan steps, two ballot steps per row with
# a ragged tail; the 23x23 block (529 = 8*64 + 17 px) is cut out of the 67x92 block, whose rows are therefore interrupted (6164 - 529 px); the 8x8
# block has exactly 64 px; object 3 is absent in image 0 and has 4 px (< min_num) in image 1.  Masks and fields differ between the images.
LAYOUT = (
    {0: (0, 0, 67, 92, 0.12, 0.3), 1: (3, 92, 8, 8, 0.05, 0.0), 2: (20, 40, 23, 23, 0.2, 0.5)},
    {0: (5, 8, 67, 92, 0.12, 0.3), 1: (60, 0, 8, 8, 0.05, 0.0), 2: (44, 69, 23, 23, 0.2, 0.5), 3: (1, 2, 2, 2, 0.05, 0.0)},
)


def common_input(seed=0):
    """labels uint8 [B,H,W]; field fp32 [B,H,W,LD] with (dy,dx) x 9 at DIR_OFF and NaN in every other channel and in every background pixel;
    kps [B,OBJECTS,9,2] (x,y).  Directions point at the keypoint, turned by N(0, noise) (outliers: a uniform angle), lengths uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    labels = np.zeros((B, H, W), np.uint8)
    field = np.full((B, H, W, LD), np.nan, np.float32)
    kps = np.zeros((B, OBJECTS, KP, 2))
    for bi in range(B):
        for o in sorted(LAYOUT[bi]):        # a later (smaller) block is cut out of an earlier one
            y0, x0, rows, cols = LAYOUT[bi][o][:4]
            labels[bi, y0:y0 + rows, x0:x0 + cols] = o + 1
        for o, (y0, x0, rows, cols, noise, outliers) in LAYOUT[bi].items():
            ys, xs = np.nonzero(labels[bi] == o + 1)
            n = ys.size
            kps[bi, o] = np.stack([rng.uniform(x0 - 5, x0 + cols + 5, KP), rng.uniform(y0 - 5, y0 + rows + 5, KP)], 1)
            ex, ey = kps[bi, o, None, :, 0] - (xs[:, None] + 0.5), kps[bi, o, None, :, 1] - (ys[:, None] + 0.5)
            ang = np.arctan2(ey, ex) + rng.normal(0.0, noise, (n, KP))
            ang = np.where(rng.uniform(size=(n, KP)) < outliers, rng.uniform(-np.pi, np.pi, (n, KP)), ang)
            length = rng.uniform(0.5, 2.0, (n, KP))
            rec = np.stack([length * np.sin(ang), length * np.cos(ang)], -1).reshape(n, 2 * KP)       # (dy, dx)
            field[bi, ys, xs, DIR_OFF:DIR_OFF + 2 * KP] = rec.astype(np.float32)
    return labels, field, kps


def common_draws(seed, rounds, hyp):
    """int32 [rounds,B,OBJECTS,hyp,9,2] over the full [0, 2^31) range (not reduced mod tn)."""
    return np.random.default_rng(seed).integers(0, 2 ** 31, (rounds, B, OBJECTS, hyp, KP, 2), dtype=np.int64).astype(np.int32)
