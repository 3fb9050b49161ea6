"""The device PnP's arithmetic on the CPU: `cp_pnp_host_f64` (the host twin of `cp_pnp_f64`: the same csrc/pnp_math.h, serially) against the
host path `pnp.pnp`, plus the hypothesis table and the callers' rules.  No kernel is launched here.

Gates come from the host path alone, never from the code under test: for each fixture set the host solver runs with RANSAC
seeds 0..3, and the largest seed-to-seed difference of a pose entry (R and t separately) and of the relative all-point cost is the spread of
that set.  Gate for R: 10 x spread + 8 fp32 ulps of 1; for t: 10 x spread + 8 fp32 ulps of the largest |t|; for the relative cost: 100 x spread.
The factor 10 covers another LM stopping iterate in the same basin.  Single hypotheses are not compared: a 5-point system has a null space of
dimension >= 2 and LAPACK and Jacobi return different bases of it; the final pose is the optimum of one fixed objective.

The case generator of this module is shared with tests/test_gpu_pnp.py."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from casapose_amd import _lib
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation import pose_evaluation as E
from casapose_amd.pose_estimation.device_pnp import DevicePnP, HostTwinPnP, affine_from_offsets, hypothesis_table

K32 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
# float32 [n,3], [n,2] image pixels (fp32 values unless `crop` is given), float64 [3,4]; K float32 [3,3]; crop: float32 [n,2] crop pixels whose
# transform_points_back under `offsets` is points_2d
Case = namedtuple("Case", "points_3d points_2d pose_gt sigma outliers K crop offsets")
Reference = namedtuple("Reference", "poses costs spread_R spread_t spread_cost gate_R gate_t gate_cost")
ULP_ONE = float(np.spacing(np.float32(1.0)))


def make_case(rng, n=9, sigma=0.0, outliers=0, K=K32, offsets=None) -> Case:
    """n 3-D points uniform in +-60 mm with the first at the origin; a rotation of 0.2..2.8 rad about a random axis; t = (+-150, +-100,
    600..1200) mm; pixel noise sigma; `outliers` points displaced by 40..80 px.  Everything the solvers read is an fp32 value."""
    X = rng.uniform(-60.0, 60.0, (n, 3))
    X[0] = 0.0
    X = X.astype(np.float32)
    axis = rng.normal(size=3)
    R = P.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.2, 2.8))
    t = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1200)])
    x = P.project(X.astype(np.float64), K.astype(np.float64), R, t) + sigma * rng.normal(size=(n, 2))
    for i in rng.choice(n, outliers, replace=False):
        a = rng.uniform(0, 2 * np.pi)
        x[i] += rng.uniform(40.0, 80.0) * np.array([np.cos(a), np.sin(a)])
    pose = np.concatenate([R, t[:, None]], axis=1)
    if offsets is None:
        return Case(X, x.astype(np.float32), pose, sigma, outliers, K, None, None)
    A = affine_from_offsets(offsets)[0]
    M, c = np.array([[A[0], A[1]], [A[3], A[4]]]), np.array([A[2], A[5]])
    crop = ((x - c) @ np.linalg.inv(M).T).astype(np.float32)
    return Case(X, E.transform_points_back(crop, offsets), pose, sigma, outliers, K, crop, offsets)


# name -> (generator seed, n, [(sigma, outliers, cases)]).  The sets with another point count than 9 are compared with the host path on
# small-residual cases only: with 10 or more points the four host seeds find the same consensus set, their poses are bit-identical, and a
# spread of exactly 0 says nothing about the LM stopping iterate, which for a cost of ~2000 px^2 (a planted outlier) and the relative stop
# of 1e-10 is uncertain at the 1e-6 level (the "hard" set measures it for n = 9).  Their outlier cases check the consensus instead.
FIXTURE_SETS = {
    "clean": (11, 9, [(0.0, 0, 4)]),
    "hard": (12, 9, [(0.5, 0, 3), (0.0, 1, 3), (0.5, 1, 3), (0.0, 2, 3), (0.5, 2, 3)]),   # 15 cases: b = 3, oc = 5 on the GPU
    "percam": (18, 9, [(0.5, 0, 5), (0.5, 1, 5), (0.0, 2, 5)]),   # image i = case // 5 has its own K and crop offsets
    "n5": (13, 5, [(0.0, 0, 2)]),
    "n10": (14, 10, [(0.0, 0, 2), (0.5, 0, 2)]),
    "n11": (15, 11, [(0.0, 0, 2), (0.5, 0, 2)]),
    "n10_outliers": (16, 10, [(0.5, 1, 2), (0.5, 2, 2)]),
    "n11_outliers": (17, 11, [(0.5, 1, 2), (0.5, 2, 2)]),
}


PERCAM_K = np.stack([K32 * np.float32([[s], [s], [1.0]]) + np.float32([[0, 0, 7.0 * i], [0, 0, -4.0 * i], [0, 0, 0]]) for i, s in enumerate((1.0, 1.05, 0.9))])
PERCAM_OFFSETS = np.array([[12.0, 20.0, 0.0, 0.0, 3.0, -2.0, 4.0, 1.25, 640.0, 480.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 640.0, 480.0],
                           [30.0, 5.0, 0.0, 0.0, -6.0, 9.0, -11.0, 0.8, 640.0, 480.0]])
PERCAM_MASK = np.array([[1, 0, 1, 1, 0], [0, 1, 1, 1, 1], [1, 1, 0, 1, 1]], np.int32)


@functools.lru_cache(maxsize=None)
def fixture_set(name):
    seed, n, settings = FIXTURE_SETS[name]
    rng = np.random.default_rng(seed)
    if name == "percam":
        return tuple(make_case(rng, n, sigma, outliers, PERCAM_K[i], PERCAM_OFFSETS[i]) for i, (sigma, outliers, count) in enumerate(settings)
                     for _ in range(count))
    return tuple(make_case(rng, n, sigma, outliers) for sigma, outliers, count in settings for _ in range(count))


def all_point_cost(case: Case, pose) -> float:
    pose = np.asarray(pose, np.float64)
    d = P.project(case.points_3d.astype(np.float64), case.K.astype(np.float64), pose[:, :3], pose[:, 3]) - case.points_2d.astype(np.float64)
    return float((d * d).sum())


@functools.lru_cache(maxsize=None)
def host_runs(name):
    """pnp.pnp with RANSAC seeds 0..3 on every case of the set -> (poses [cases,4,3,4], all-point costs [cases,4]) in fp64"""
    cases = fixture_set(name)
    poses = np.stack([[P.pnp(c.points_3d, c.points_2d, c.K, rng=np.random.default_rng(s)) for s in range(4)] for c in cases]).astype(np.float64)
    assert np.abs(poses).sum(axis=(2, 3)).min() > 0, "the host path failed on a fixture case"
    return poses, np.array([[all_point_cost(c, poses[i, s]) for s in range(4)] for i, c in enumerate(cases)])


# The noisy nine-point cases are one fixture set in two batches ("hard": shared K, image pixels; "percam": per-image K and crop offsets): the
# spread is taken over both.  On "percam" alone the four seeds happen to find the same consensus sets and agree bit for bit, which would
# make the cost gate 0 -- a statement about the sample, not about the host path.
GATE_SETS = {"hard": ("hard", "percam"), "percam": ("hard", "percam")}


@functools.lru_cache(maxsize=None)
def host_reference(name) -> Reference:
    """The reference poses and costs of a set (seed 0), the seed-to-seed spreads of its fixture set and the gates.  Asserts the condition under
    which a comparison means anything: on every case the four seeds agree within the gates."""
    dR, dt, dc, tmax = [], [], [], 0.0
    for member in GATE_SETS.get(name, (name,)):
        poses, costs = host_runs(member)
        dR.append(np.ptp(poses[:, :, :, :3], axis=1).max())
        dt.append(np.ptp(poses[:, :, :, 3], axis=1).max())
        dc.append((np.ptp(costs, axis=1) / costs.min(axis=1)).max())
        tmax = max(tmax, np.abs(poses[:, :, :, 3]).max())
    dR, dt, dc = float(max(dR)), float(max(dt)), float(max(dc))
    gate_R = 10.0 * dR + 8.0 * ULP_ONE
    gate_t = 10.0 * dt + 8.0 * float(np.spacing(np.float32(tmax)))
    gate_cost = 100.0 * dc
    assert dR <= gate_R and dt <= gate_t, "the host seeds disagree beyond the gates on set %s" % name
    poses, costs = host_runs(name)
    return Reference(poses[:, 0], costs[:, 0], dR, dt, dc, gate_R, gate_t, gate_cost)


def batch_of(cases, b, oc):
    """-> (float32 [b,oc,n,2] keypoints: crop pixels where the cases have them, image pixels otherwise; float32 [b,oc,n,3])"""
    n = cases[0].points_3d.shape[0]
    xy = np.stack([c.points_2d if c.crop is None else c.crop for c in cases]).astype(np.float32).reshape(b, oc, n, 2)
    x3 = np.stack([c.points_3d for c in cases]).reshape(b, oc, n, 3)
    return xy, x3


def assert_within_gates(got, want, ref: Reference, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dR, dt = np.abs(got[..., :3] - want[..., :3]).max(), np.abs(got[..., 3] - want[..., 3]).max()
    print("%s: max |dR| %.3g (gate %.3g), max |dt| %.3g (gate %.3g)" % (what, dR, ref.gate_R, dt, ref.gate_t))
    assert dR <= ref.gate_R and dt <= ref.gate_t, "%s: max |dR| %.3g (gate %.3g), max |dt| %.3g (gate %.3g)" % (what, dR, ref.gate_R, dt, ref.gate_t)


def assert_costs_within_gate(cases, poses, ref: Reference, what):
    rel = max(abs(all_point_cost(c, poses[i]) - ref.costs[i]) / ref.costs[i] for i, c in enumerate(cases))
    print("%s: max relative cost difference %.3g (gate %.3g)" % (what, rel, ref.gate_cost))
    assert rel <= ref.gate_cost, "%s: relative all-point cost differs by %.3g (gate %.3g)" % (what, rel, ref.gate_cost)


@pytest.fixture(scope="module")
def twin9():
    return DevicePnP(None, 9)


def test_noise_free_poses_against_ground_truth(twin9):
    cases, ref = fixture_set("clean"), host_reference("clean")
    xy, x3 = batch_of(cases, 1, len(cases))
    got = twin9.solve_host(xy, x3, K32, np.ones((1, len(cases)), np.int32))[0]
    assert (twin9.last_info[0, :, 0] == 0).all() and (twin9.last_info[0, :, 2] == 9).all()
    assert_within_gates(got, np.stack([c.pose_gt for c in cases]), ref, "twin against ground truth")
    assert_within_gates(got, ref.poses, ref, "twin against pnp.pnp")


def test_noisy_and_outlier_poses_against_the_host_path(twin9):
    cases, ref = fixture_set("hard"), host_reference("hard")
    xy, x3 = batch_of(cases, 3, 5)
    got = twin9.solve_host(xy, x3, K32, np.ones((3, 5), np.int32)).reshape(15, 3, 4)
    info = twin9.last_info.reshape(15, 4)
    assert (info[:, 0] == 0).all()
    for i, c in enumerate(cases):
        assert info[i, 2] >= 9 - c.outliers, "case %d: %d inliers with %d planted outliers" % (i, info[i, 2], c.outliers)
        assert 0 <= info[i, 1] < 126 and 1 <= info[i, 3] <= 20
    assert_within_gates(got, ref.poses, ref, "twin against pnp.pnp")
    assert_costs_within_gate(cases, got, ref, "twin against pnp.pnp")
    cost = twin9.last_cost.reshape(15, 2)
    assert (cost[:, 1] <= cost[:, 0]).all()
    np.testing.assert_allclose(cost[:, 1], [all_point_cost(c, got[i]) for i, c in enumerate(cases)], rtol=1e-4)


def test_per_image_camera_and_crop_affine(twin9):
    cases, ref = fixture_set("percam"), host_reference("percam")
    xy, x3 = batch_of(cases, 3, 5)
    got = twin9.solve_host(xy, x3, PERCAM_K, PERCAM_MASK, affine=affine_from_offsets(PERCAM_OFFSETS)).reshape(15, 3, 4)
    on = PERCAM_MASK.reshape(15) != 0
    assert np.array_equal(twin9.last_info.reshape(15, 4)[:, 0], np.where(on, 0, 1)) and not got[~on].any()
    assert_within_gates(got[on], ref.poses[on], ref, "twin against pnp.pnp, per-image K and affine")
    assert_costs_within_gate([c for c, o in zip(cases, on) if o], got[on], ref._replace(costs=ref.costs[on]), "twin against pnp.pnp, per-image K and affine")


@pytest.mark.parametrize("name", ["n5", "n10", "n11"])
def test_other_point_counts(name):
    cases, ref = fixture_set(name), host_reference(name)
    n = cases[0].points_3d.shape[0]
    solver = DevicePnP(None, n)
    xy, x3 = batch_of(cases, 1, len(cases))
    got = solver.solve_host(xy, x3, K32, np.ones((1, len(cases)), np.int32))[0]
    assert (solver.last_info[0, :, 0] == 0).all() and (solver.last_info[0, :, 2] == n).all()
    assert_within_gates(got, ref.poses, ref, "twin against pnp.pnp, n = %d" % n)


@pytest.mark.parametrize("name", ["n10_outliers", "n11_outliers"])
def test_consensus_with_other_point_counts(name):
    cases = fixture_set(name)
    n = cases[0].points_3d.shape[0]
    solver = DevicePnP(None, n)
    xy, x3 = batch_of(cases, 1, len(cases))
    got = solver.solve_host(xy, x3, K32, np.ones((1, len(cases)), np.int32))[0]
    info, cost = solver.last_info[0], solver.last_cost[0]
    assert (info[:, 0] == 0).all() and (cost[:, 1] <= cost[:, 0]).all()
    for i, c in enumerate(cases):
        assert n - c.outliers <= info[i, 2] <= n and 0 <= info[i, 1] < solver.hypotheses
        assert abs(np.linalg.det(got[i][:, :3].astype(np.float64)) - 1.0) < 1e-5 and got[i][2, 3] > 0


def test_hypothesis_table():
    for n, rows in ((5, 1), (9, 126), (10, 252)):
        t = hypothesis_table(n)
        assert t.dtype == np.uint8 and t.shape == (rows, 5) and t.max() == n - 1
        as_tuples = [tuple(r) for r in t]
        assert as_tuples == sorted(set(as_tuples)), "rows must be distinct and in lexicographic order"
        assert all(r[i] < r[i + 1] for r in as_tuples for i in range(4))
    t = hypothesis_table(11)
    assert t.shape == (256, 5) and len({tuple(r) for r in t}) == 256 and t.max() <= 10
    assert all(r[i] < r[i + 1] for r in t for i in range(4))
    assert np.array_equal(t, hypothesis_table(11)) and np.array_equal(t, DevicePnP(None, 11).table_host)
    with pytest.raises(ValueError, match="host path"):
        hypothesis_table(4)
    with pytest.raises(ValueError, match="host path"):
        DevicePnP(None, 4)


def test_solve_flag_zero_gives_the_zero_pose_and_leaves_neighbours_alone(twin9):
    cases = fixture_set("hard")[:3]
    xy, x3 = batch_of(cases, 1, 3)
    full = twin9.solve_host(xy, x3, K32, np.ones((1, 3), np.int32)).copy()
    got = twin9.solve_host(xy, x3, K32, np.array([[1, 0, 1]], np.int32))
    assert np.array_equal(got[0, 1], np.zeros((3, 4), np.float32)) and twin9.last_info[0, 1].tolist() == [1, -1, 0, 0]
    assert np.array_equal(got[0, 0], full[0, 0]) and np.array_equal(got[0, 2], full[0, 2])
    none = twin9.solve_host(xy, x3, K32, np.zeros((1, 3), np.int32))
    assert not none.any()


def degenerate_batch(kind):
    """Three pairs; the middle one is the failure: "equal" = nine equal 2-D points (a collapsed vote), "collinear" = 3-D points on one line,
    "nan" = one NaN keypoint."""
    cases = fixture_set("hard")[:3]
    xy, x3 = batch_of(cases, 1, 3)
    xy, x3 = xy.copy(), x3.copy()
    if kind == "equal":
        xy[0, 1] = np.float32([311.5, 207.25])
    elif kind == "collinear":
        x3[0, 1] = np.linspace(-60, 60, 9, dtype=np.float32)[:, None] * np.float32([0.6, -0.3, 0.74])
    else:
        xy[0, 1, 4, 0] = np.nan
    return xy, x3


@pytest.mark.parametrize("kind,status", [("equal", 3), ("collinear", 3), ("nan", 2)])
def test_bounded_failure(twin9, kind, status):
    cases = fixture_set("hard")[:3]
    xy0, x30 = batch_of(cases, 1, 3)
    full = twin9.solve_host(xy0, x30, K32, np.ones((1, 3), np.int32)).copy()
    xy, x3 = degenerate_batch(kind)
    got = twin9.solve_host(xy, x3, K32, np.ones((1, 3), np.int32))   # the call returns
    assert not got[0, 1].any() and twin9.last_info[0, 1, 0] == status != 0
    assert np.array_equal(got[0, 0], full[0, 0]) and np.array_equal(got[0, 2], full[0, 2])


def test_argument_errors_raise(twin9):
    xy, x3 = batch_of(fixture_set("hard")[:3], 1, 3)
    with pytest.raises(ValueError):
        twin9.solve_host(xy[:, :, :8], x3[:, :, :8], K32, np.ones((1, 3), np.int32))
    with pytest.raises(_lib.CasaposeHipError, match="reprojection_error"):
        DevicePnP(None, 9, reprojection_error=0.0).solve_host(xy, x3, K32, np.ones((1, 3), np.int32))
    with pytest.raises(_lib.CasaposeHipError, match="solve_host"):
        twin9.solve(xy, x3, K32, np.ones((1, 3), np.int32))


OFFSETS = np.array([[12.0, 20.0, 0.0, 0.0, 3.0, -2.0, 4.0, 1.25, 640.0, 480.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 640.0, 480.0]])


def caller_batch():
    """b = 2, oc = 3 crop-pixel keypoints for estimate_poses: image 0 has a crop offset, a rotation and a scale.  Object 1 of image 0 is
    absent (zero points, valid); object 2 of image 1 is voted although it is not in the ground truth (a false positive)."""
    cases = fixture_set("hard")[:6]
    xy, x3 = batch_of(cases, 2, 3)
    A = affine_from_offsets(OFFSETS)
    crop = np.empty_like(xy, dtype=np.float64)
    for n in range(2):
        M, c = np.array([[A[n, 0], A[n, 1]], [A[n, 3], A[n, 4]]]), np.array([A[n, 2], A[n, 5]])
        crop[n] = (xy[n].astype(np.float64) - c) @ np.linalg.inv(M).T
    crop = crop.astype(np.float32)
    crop[0, 1] = 0.0
    valid = np.array([[1, 1, 1], [1, 1, 0]], np.float32)
    return crop, x3[:, :, None], valid


def test_affine_is_transform_points_back():
    crop, _, _ = caller_batch()
    A = affine_from_offsets(OFFSETS)
    for n in range(2):
        p = crop[n, 0].astype(np.float64)
        want = E.transform_points_back(p, OFFSETS[n])
        got = np.stack([A[n, 0] * p[:, 0] + A[n, 1] * p[:, 1] + A[n, 2], A[n, 3] * p[:, 0] + A[n, 4] * p[:, 1] + A[n, 5]], axis=1)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_estimate_poses_with_a_solver_keeps_the_callers_rules():
    crop, kp3, valid = caller_batch()
    ref = host_reference("hard")
    want, want_fp = E.estimate_poses(crop, kp3, K32, valid, OFFSETS, rng=np.random.default_rng(0))
    got, got_fp = E.estimate_poses(crop, kp3, K32, valid, OFFSETS, solver=HostTwinPnP(9))
    assert got.shape == (2, 3, 3, 4) and got.dtype == np.float32 and isinstance(got, np.ndarray)
    assert not want[0, 1].any() and not got[0, 1].any()
    assert np.array_equal(got_fp, want_fp) and want_fp.tolist() == [0.0, 0.0, 1.0]
    assert np.array_equal(np.abs(got).sum(axis=(2, 3)) == 0, np.abs(want).sum(axis=(2, 3)) == 0)
    assert_within_gates(got, want, ref, "estimate_poses with the twin against the host path")
