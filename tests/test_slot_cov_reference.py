"""tests/slot_cov_reference.py (the covariance per slot and keypoint of csrc/ls_cov_math.h, cp_ls_slot_covariance_f32) on the CPU: known answers,
a calibration of the definition against the scatter of the LS estimates it describes, and what weighting the PnP by it buys on an occluded
instance.  No GPU.

CALIBRATION (fp64).  A disc of radius 10 on 48 x 64, every pixel's line offset perpendicularly by N(0, 0.5 px), weights uniform in 0.5..1.5,
CAL_DRAWS = 2000 independent draws per keypoint.  The estimate is linear in the offsets, so its covariance is sigma^2 A^-1 (sum w^2 P) A^-1,
which for weights independent of the directions is Sigma / n_eff with n_eff = (sum w)^2 / sum w^2: the two generalised eigenvalues of (the
covariance of the estimates over the draws, the mean of Sigma / n_eff) should be 1.  Measured at 2000 draws, seed 7 (smaller, larger):
    keypoint at the centre      1.008, 1.069
    15 px away                  0.967, 1.027
    90 px away                  0.962, 1.029
The sampling error of a variance over N draws is sqrt(2 / (N - 1)) = 3.2 % at 2000; the bounds CAL_BOUNDS are the measured extremes over the
three keypoints widened by four of them (12.7 %) either way: 0.840 .. 1.204.  They lie far inside the factor of 2 at which the definition or
its restatement would be wrong.

THE PNP CLAIM.  PNP_POSES = 60 random poses of a 10 cm box (its centre and eight corners) at 120 x 160; the instance's pixels are the left half
of a disc of radius RADIUS = 25 px around the projected centre (about 980 pixels); every pixel's direction to every keypoint is turned by
independent N(0, 0.05 rad); the fp64 LS vote, its covariance, and the host PnP (floor 1/12 px^2), seed 11.  Measured medians of the rotation error:
    unweighted 0.158 deg, weighted by Sigma 0.091 deg, weighted by Sigma / pixels (the standard error) 0.147 deg
The gain is MEASURED_GAIN = unweighted - weighted = 0.067 deg; the test asks for half of it, and that the standard-error scaling gains less
than a quarter of it (0.011 deg, 16 %: it is swamped by the floor, and the weighting then changes next to nothing).  The radius decides the
second claim: the standard error is Sigma over the pixel count, so it sinks below the
floor only for an instance of enough pixels.  At a radius of 12 px (226 pixels) the same 60 poses give 0.702 / 0.259 / 0.502 deg: the weighting
by Sigma pays even more, and the standard error is NOT swamped (45 % of the gain).  25 px is what an object of this size covers at this
distance, and a slot of the instance path at 480 x 640 holds more pixels still, not fewer."""
import functools
import os
import re

import numpy as np
import pytest

import ls_reference as L
import robust_ls_reference as RL
import slot_cov_reference as SC

KP = 9
CAL_DRAWS = 2000
CAL_MEASURED = (0.962, 1.069)                       # the extremes of the docstring's table
CAL_SPREAD = 4 * np.sqrt(2.0 / (CAL_DRAWS - 1))     # 0.127
CAL_BOUNDS = (CAL_MEASURED[0] * (1 - CAL_SPREAD), CAL_MEASURED[1] * (1 + CAL_SPREAD))
PNP_POSES = 60
RADIUS = 25.0
MEASURED = dict(unweighted=0.158, weighted=0.091, standard_error=0.147)      # degrees, the docstring's medians
MEASURED_GAIN = MEASURED["unweighted"] - MEASURED["weighted"]


@pytest.fixture(autouse=True, scope="module")
def the_header_that_is_restated():
    """slot_cov_reference.py restates csrc/ls_cov_math.h: the order of the pixel's arithmetic, the constants and the refusals it shares with
    the robust solve are read from the headers, so that the restatement cannot outlive or drift from what it restates"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "casapose_amd", "csrc")
    cov, robust = open(os.path.join(csrc, "ls_cov_math.h")).read(), open(os.path.join(csrc, "ls_robust_math.h")).read()
    for words in ("const float d = ey * nx - ex * ny;", "const float omega = w * r;", "omega * (d * d)", "cp_lsr::well_posed(a, b, c)",
                  "w >= cp_lsr::CP_LS_ROBUST_MIN_KEPT * wall", "if (ny == 0.f && nx == 0.f) return {0.f, 0.f, 0.f};"):
        assert words in cov, words
    assert float(re.search(r"CP_LS_ROBUST_MIN_KEPT = ([0-9.e-]+);", robust).group(1)) == SC.MIN_KEPT
    assert float(re.search(r"CP_LS_ROBUST_MAX_COND = ([0-9.e-]+);", robust).group(1)) == RL.MAX_COND
    assert "LSR_HD bool well_posed(double a, double b, double c)" in robust


# ---- scenes for the known answers ---------------------------------------------------------------------------------------------------------------
H, W = 48, 64
REC = dict(ld=36, dir_off=9, conf_off=27)


def blank(b=1, h=H, w=W):
    f = np.full((b, h, w, 36), np.nan, np.float32)
    return f, np.zeros((b, h, w), np.uint8)


def centres(h=H, w=W):
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    return yy, xx


def aim(field, mask, kpt, j, offset=None):
    """directions of keypoint j on the pixels of mask: at kpt, or with offset [H,W] (pixels) such that kpt lies that far from the pixel's line"""
    yy, xx = centres(*field.shape[1:3])
    vy, vx = kpt[0] - yy, kpt[1] - xx
    r = np.hypot(vy, vx)
    ang = np.arctan2(vy, vx) + (0.0 if offset is None else np.arcsin(np.clip(offset / np.where(r > 0, r, 1.0), -1.0, 1.0)))
    field[0, ..., 9 + 2 * j][mask] = np.sin(ang)[mask]
    field[0, ..., 9 + 2 * j + 1][mask] = np.cos(ang)[mask]


def ring_scene(delta=0.5):
    """slot 1: the pixels at 6..14 px from (24, 32), a pixel corner, so that the set is invariant under a quarter turn; the sign of the offset
    depends on the radius alone, so the set of lines is invariant too and sum n n^T = (N / 2) I exactly.  Weights all softplus(0.3)."""
    f, sm = blank()
    yy, xx = centres()
    r2 = (yy - 24.0) ** 2 + (xx - 32.0) ** 2
    m = (r2 >= 36.0) & (r2 <= 196.0)
    sm[0][m] = 1
    sign = np.where(np.floor(r2).astype(np.int64) % 2 == 0, 1.0, -1.0)
    for j in range(KP):
        aim(f, m, (24.0, 32.0), j, sign * delta)
    f[0, ..., 27:36][m] = 0.3
    est = np.zeros((1, 4, KP, 2), np.float32)
    est[0, 0] = (24.0, 32.0)
    return f, sm, est


def band_scene(noise=0.0, seed=3):
    """slot 2: a block of pixels left of the keypoint (30.3, 55.6), which lies 25..45 px outside along x: the rays are nearly parallel to x"""
    f, sm = blank()
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), bool)
    m[22:38, 10:30] = True
    sm[0][m] = 2
    for j in range(KP):
        aim(f, m, (30.3, 55.6), j, rng.normal(0, noise, (H, W)) if noise else None)
    f[0, ..., 27:36][m] = rng.normal(0, 1, (int(m.sum()), KP))
    est = np.zeros((1, 4, KP, 2), np.float32)
    est[0, 1] = (30.3, 55.6)
    return f, sm, est


def run(f, sm, est, cutoff=None, slots=4):
    (s32, _), (s64, _) = SC.moments(f, 9, 27, 0, sm, slots, est, cutoff)
    return s32, s64, SC.finish(s32, est, f.shape[1]), SC.finish(s64, est, f.shape[1])


def test_a_full_ring_of_lines_offset_by_delta_gives_two_delta_squared():
    for delta in (0.5, 1.25):
        f, sm, est = ring_scene(delta)
        s32, s64, (c32, st32, ok32), (c64, st64, ok64) = run(f, sm, est)
        assert ok64[0, 0].all() and ok32[0, 0].all() and not ok64[0, 1:].any()
        n = int((sm == 1).sum())
        assert s64[0, 0, :, 4] == pytest.approx(n * np.logaddexp(0, np.float32(0.3)), rel=1e-6)                  # Wall: every pixel's weight
        for cov, stat, tol in ((c64, st64, 1e-4), (c32, st32, 2e-3)):
            assert cov[0, 0, :, 0] == pytest.approx(2 * delta ** 2, rel=tol) and cov[0, 0, :, 2] == pytest.approx(2 * delta ** 2, rel=tol)
            assert np.abs(cov[0, 0, :, 1]).max() <= tol * 2 * delta ** 2
            assert stat[0, 0, :, 0] == pytest.approx(delta ** 2, rel=tol) and stat[0, 0, :, 1] == pytest.approx(1.0, abs=1e-6)
        assert np.isnan(c64[0, 1:]).all() and not st64[0, 1:].any()                                             # the empty slots


def test_the_order_is_x_then_y_and_an_exact_field_has_no_residual():
    f, sm, est = band_scene()
    _, s64, (c32, st32, ok32), (c64, st64, ok64) = run(f, sm, est)
    assert ok64[0, 1].all() and ok32[0, 1].all()
    # directions stored in fp32: the lines miss the keypoint by ~ 45 px * 6e-8; Q is that squared
    assert st64[0, 1, :, 0].max() < 1e-9 and st32[0, 1, :, 0].max() < 1e-7
    f, sm, est = band_scene(noise=0.4)
    _, s64, _, (c64, st64, ok64) = run(f, sm, est)
    assert ok64[0, 1].all()
    assert (c64[0, 1, :, 0] > 20 * c64[0, 1, :, 2]).all()            # sxx first: long along the rays, which run along x
    assert (st64[0, 1, :, 0] > 0.1).all() and (st64[0, 1, :, 0] < 0.25).all()        # about 0.4^2
    # the matrix of the (y, x) sums, inverted by hand
    a, b, c, q = (s64[0, 1, 0, i] for i in range(4))
    sig = H * H * q * np.linalg.inv(np.array([[a, b], [b, c]]))
    assert c64[0, 1, 0] == pytest.approx([sig[1, 1], sig[0, 1], sig[0, 0]], rel=1e-9)


def test_every_refusal_gives_three_nans():
    f, sm, est = band_scene(noise=0.4)
    # parallel directions in slot 3, nothing in slot 4
    m = np.zeros((H, W), bool)
    m[2:12, 40:60] = True
    sm[0][m] = 3
    f[0, ..., 9:27][m] = np.tile([1.0, 0.0], KP)
    f[0, ..., 27:36][m] = 0.0
    est[0, 2] = (7.0, 50.0)
    for cutoff in (None, 4.0):
        _, s64, (c32, _, ok32), (c64, st64, ok64) = run(f, sm, est, cutoff)
        assert ok64[0, 1].all() and not ok64[0, 2].any() and not ok64[0, 3].any() and not ok64[0, 0].any()
        assert np.array_equal(ok32, ok64) and np.isnan(c64[~ok64]).all() and np.isfinite(c64[ok64]).all()
        assert (st64[0, 2, :, 1] == 1.0).all() if cutoff is None else (st64[0, 2, :, 1] > SC.MIN_KEPT).all()      # rank one: weight enough, and still no covariance
        assert not st64[0, 3].any()
    # an estimate 2 px off across the rays at a cut-off of 2 px keeps less than 1/8 of the weight
    off = est.copy()
    off[0, 1, :, 0] += 2.0
    _, _, _, (c64, st64, ok64) = run(f, sm, off, 2.0)
    assert not ok64[0, 1].any() and (st64[0, 1, :, 1] < SC.MIN_KEPT).all() and (st64[0, 1, :, 1] > 0).any() and np.isnan(c64[0, 1]).all()
    _, _, _, (c64, _, ok64) = run(f, sm, off, None)                  # without a cut-off the same estimate has a covariance, and a large one
    assert ok64[0, 1].all() and (c64[0, 1, :, 2] > 1.0).all()
    # a NaN estimate
    bad = est.copy()
    bad[0, 1, 4, 1] = np.nan
    bad[0, 1, 5, 0] = np.inf
    for cutoff in (None, 4.0):
        _, _, (c32, st32, ok32), (c64, st64, ok64) = run(f, sm, bad, cutoff)
        assert not ok64[0, 1, 4] and not ok64[0, 1, 5] and ok64[0, 1, :4].all() and ok64[0, 1, 6:].all() and np.array_equal(ok32, ok64)
        assert np.isnan(c64[0, 1, 4:6]).all() and not st64[0, 1, 4:6].any() and not st32[0, 1, 4:6].any()


def test_zero_direction_pixels_change_nothing():
    f, sm, est = band_scene(noise=0.4)
    for cutoff in (None, 4.0):
        before = run(f, sm, est, cutoff)
        g, sm2 = f.copy(), sm.copy()
        sm2[0, 40:44, 10:30] = 2                                  # more pixels of the slot, all without a direction, with any weight
        g[0, 40:44, 10:30, 9:27] = 0.0
        g[0, 40:44, 10:30, 27:36] = 3.0
        g[0, 25, 12, 9:27] = 0.0                                  # and one of its own pixels loses its direction: it leaves all five sums
        after = run(g, sm2, est, cutoff)
        h2 = f.copy()
        sm3 = sm.copy()
        sm3[0, 25, 12] = 0
        without = run(h2, sm3, est, cutoff)
        assert np.array_equal(after[0], without[0]) and np.array_equal(after[1], without[1])
        assert not np.array_equal(before[1], after[1])
        plain = L.sums(L.terms(g, 36, 9, 27, 0, H)[1], sm2, 4)[0]
        assert plain[0, 1, 0, 0] + plain[0, 1, 0, 2] > after[1][0, 1, 0, 4] + 80 * 3.0             # the plain vote does count them, as w I


def test_no_cutoff_is_the_plain_normal_matrix_and_a_cutoff_is_the_reweighted_one():
    """A00, A01, A11 are the plain sums' matrix without a cut-off and the reweighted pass's with one, bit for bit in both orders, on a scene
    without zero directions; Wall is the plain trace"""
    f, sm, est = band_scene(noise=0.4)
    est = est + np.float32(0.3)
    t32, t64 = L.terms(f, 36, 9, 27, 0, H)
    s32, s64, _, _ = run(f, sm, est)
    for mine, t in ((s32, t32), (s64, t64)):
        plain = L.sums(t, sm, 4)[0]
        assert np.array_equal(mine[..., :3], plain[..., :3])
        assert mine[..., 4] == pytest.approx(plain[..., 0] + plain[..., 2], rel=1e-6)
    (r32, _), (r64, _) = RL.one_pass(f, 36, 9, 27, 0, sm, 4, est, 4.0)
    s32, s64, _, _ = run(f, sm, est, 4.0)
    assert np.array_equal(s32[..., :3], r32[..., :3]) and np.array_equal(s64[..., :3], r64[..., :3])
    assert (s64[0, 1, :, 0] + s64[0, 1, :, 2] < s64[0, 1, :, 4]).all()


# ---- calibration ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def calibration(dist, draws=CAL_DRAWS, seed=7):
    """the two generalised eigenvalues of (covariance of the LS estimates over the draws, mean of Sigma / n_eff), ascending"""
    rng = np.random.default_rng([seed, int(dist)])
    yy, xx = centres()
    m = (yy - 24.0) ** 2 + (xx - 32.0) ** 2 <= 100.0
    cy, cx = yy[m], xx[m]
    kpt = np.array([24.0, 32.0]) + dist * np.array([np.sin(0.6), np.cos(0.6)])
    vy, vx = kpt[0] - cy, kpt[1] - cx
    r = np.hypot(vy, vx)
    ny, nx = vy / r, vx / r
    eps = rng.normal(0, 0.5, (draws, cy.size))
    w = rng.uniform(0.5, 1.5, (draws, cy.size))
    ay, ax = (cy + eps * nx) / H, (cx - eps * ny) / H              # the line's anchor moved by eps across the line: the keypoint is eps off it
    est = SC.flat_vote(ay, ax, ny, nx, w, H)
    cov, stat, ok = SC.flat_covariance(ay, ax, ny, nx, w, est, H)
    assert ok.all() and stat[:, 0] == pytest.approx(0.25, rel=0.35)
    n_eff = w.sum(-1) ** 2 / (w * w).sum(-1)
    mean = (cov / n_eff[:, None]).mean(0)
    M = np.array([[mean[0], mean[1]], [mean[1], mean[2]]])
    C = np.cov(est[:, ::-1].T)                                     # (x, y), as cov is
    return tuple(np.sort(np.linalg.eigvals(np.linalg.solve(M, C)).real))


@pytest.mark.parametrize("dist", [0, 15, 90])
def test_calibration_against_the_scatter_of_the_estimates(dist):
    lo, hi = calibration(dist)
    print("keypoint %d px from the disc's centre, %d draws: generalised eigenvalues %.3f, %.3f (bounds %.3f .. %.3f)" % (dist, CAL_DRAWS, lo, hi, *CAL_BOUNDS))
    assert 0.5 < CAL_BOUNDS[0] and CAL_BOUNDS[1] < 2.0
    assert CAL_BOUNDS[0] <= lo and hi <= CAL_BOUNDS[1]


# ---- the PnP claim --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pnp_experiment(poses=PNP_POSES, s=0.05, seed=11):
    """median rotation errors in degrees: (unweighted, weighted by Sigma, weighted by Sigma / pixels)"""
    from casapose_amd.pose_estimation import pnp as P

    rng = np.random.default_rng(seed)
    h, w = 120, 160
    K = np.array([[180.0, 0.0, 80.0], [0.0, 180.0, 60.0], [0.0, 0.0, 1.0]])
    X = 0.05 * np.array([[0, 0, 0]] + [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    yy, xx = centres(h, w)
    floor = np.array([P.COV_FLOOR, 0.0, P.COV_FLOOR])
    errs = []
    for _ in range(poses):
        axis = rng.normal(size=3)
        rvec = axis / np.linalg.norm(axis) * rng.uniform(0.2, 2.8)
        R, t = P.rodrigues(rvec), np.array([rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05), rng.uniform(0.55, 0.75)])
        xy = P.project(X, K, R, t)
        m = ((yy - xy[0, 1]) ** 2 + (xx - xy[0, 0]) ** 2 <= RADIUS ** 2) & (xx < xy[0, 0])
        cy, cx = yy[m], xx[m]
        ang = np.arctan2(xy[:, 1, None] - cy, xy[:, 0, None] - cx) + rng.normal(0, s, (KP, cy.size))
        ny, nx, wgt = np.sin(ang), np.cos(ang), np.ones_like(ang)
        est = SC.flat_vote(cy / h, cx / h, ny, nx, wgt, h)
        cov, _, ok = SC.flat_covariance(cy / h, cx / h, ny, nx, wgt, est, h)
        assert ok.all()
        row = []
        for c in (None, cov + floor, cov / cy.size + floor):
            p6 = P.pnp_rvec_t(X, est[:, ::-1], K, rng=np.random.default_rng(0), cov=c)
            dR = P.rodrigues(p6[:3]) @ R.T
            row.append(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))
        errs.append(row)
    return tuple(np.median(np.array(errs), axis=0))


def test_weighting_the_pnp_by_the_covariance_pays_and_the_standard_error_does_not():
    u, wt, se = pnp_experiment()
    print("%d poses, s = 0.05 rad: median rotation error unweighted %.3f deg, weighted %.3f deg, weighted by the standard error %.3f deg (measured gain %.3f)"
          % (PNP_POSES, u, wt, se, MEASURED_GAIN))
    assert MEASURED_GAIN > 0
    assert wt <= u - 0.5 * MEASURED_GAIN
    assert u - se < 0.25 * MEASURED_GAIN
