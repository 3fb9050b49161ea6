"""The keypoint covariance of csrc/ransac_vote.hip (cp_kp_cov_f32) restated in plain fp64 NumPy: the inlier-count-weighted second moments of
the hypotheses about a given mean (PVNet's voting distribution).  The hypotheses and the count intervals are those of tests/ransac_reference.py,
which this module builds on; tests/test_kpcov_reference.py pins it on closed-form cases, tests/test_gpu_kpcov.py compares the kernel with it."""
import numpy as np

import ransac_reference as R


def covariance(hyp_pts, counts, mean):
    """hyp_pts [hn,kp,2] (fp32 values), counts [hn,kp] (integers), mean [kp,2] -> (cov [kp,3] = (sxx, sxy, syy) in fp64, wsum [kp] int64).
    wsum = sum_j c_j; cov = sum_j c_j (h_j - mean)(h_j - mean)^T / wsum over the hypotheses with c_j > 0 -- a hypothesis without inliers is
    skipped, not multiplied by 0 (it may be non-finite).  wsum == 0 or a non-finite mean give zeros."""
    h = np.asarray(hyp_pts, np.float64)
    c = np.asarray(counts, np.int64)
    m = np.asarray(mean, np.float64)
    kp = c.shape[1]
    cov, wsum = np.zeros((kp, 3)), np.zeros(kp, np.int64)
    for v in range(kp):
        use = c[:, v] > 0
        w = int(c[use, v].sum())
        if w == 0 or not np.isfinite(m[v]).all():
            continue
        d = h[use, v] - m[v]
        cw = c[use, v].astype(np.float64)
        cov[v] = ((cw * d[:, 0] * d[:, 0]).sum() / w, (cw * d[:, 0] * d[:, 1]).sum() / w, (cw * d[:, 1] * d[:, 1]).sum() / w)
        wsum[v] = w
    return cov, wsum


def reference_object(direct, coords, idx, thresh, mean):
    """One object from its pixel records and draws (already reduced mod tn): (cov of the definite inliers, wsum_lo, wsum_hi, hyp_pts fp32).
    hypotheses_f32 refuses draws whose determinant lies within rounding of the 1e-6 rule."""
    hp, _, _ = R.hypotheses_f32(direct, coords, idx)
    lo, hi, _ = R.count_bounds(direct, coords, hp, thresh)
    cov, wlo = covariance(hp, lo, mean)
    return cov, wlo, hi.sum(0), hp
