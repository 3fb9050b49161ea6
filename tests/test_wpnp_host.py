"""The uncertainty-weighted PnP on the CPU: `cp_pnp_weighted_host_f64` (the host twin of `cp_pnp_weighted_f64`: the same csrc/pnp_math.h,
serially) against the weighted host path `pnp.pnp(..., cov=)`, which is NumPy and shares no code with the kernel.  No kernel is launched here.

Cases come from tests/test_pnp_twin_host.py's generator plus a heteroscedastic one: per point a covariance of random orientation, and noise
drawn from it.  Gates are built the way test_pnp_twin_host.host_reference builds its own, from the WEIGHTED host path alone: it runs with RANSAC
seeds 0..3 on the shared-K set and on the per-camera set, the largest seed-to-seed difference of a pose entry (R and t separately) pooled
over both is the spread; gate for R: 10 x spread + 8 fp32 ulps of 1; for t: 10 x spread + 8 fp32 ulps of the largest |t|.  A pooled spread of
exactly 0 would say nothing about the LM stopping iterate: it is asserted not to be (SETS says which cases make it), and a case whose seeds
end in different local minima is no fixture (host_runs).

The case generators of this module are shared with tests/test_gpu_wpnp.py."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import test_pnp_twin_host as T
from casapose_amd import _lib, twin
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation import pose_evaluation as E
from casapose_amd.pose_estimation.device_pnp import DevicePnP, HostTwinPnP, affine_from_offsets

# case: a test_pnp_twin_host.Case; cov: float32 [n,3] (sxx, sxy, syy) in image pixels; cov_crop: the same in crop pixels where the case has offsets
WCase = namedtuple("WCase", "case cov cov_crop")
Gates = namedtuple("Gates", "gate_R gate_t spread_R spread_t")


def linear_part(offsets):
    A = affine_from_offsets(offsets)[0]
    return np.array([[A[0], A[1]], [A[3], A[4]]])


def as_matrices(cov3):
    c = np.asarray(cov3, np.float64)
    return np.stack([np.stack([c[..., 0], c[..., 1]], -1), np.stack([c[..., 1], c[..., 2]], -1)], -2)


def as_triples(mats):
    m = np.asarray(mats)
    return np.stack([m[..., 0, 0], m[..., 0, 1], m[..., 1, 1]], -1)


def make_wcase(rng, n=9, major=(8.0, 0.5), minor=0.3, n_major=3, K=T.K32, offsets=None) -> WCase:
    """A noise-free case of the shared generator, then per point a covariance: the first n_major points (after a shuffle) an ellipse with the
    axes `major` px at a random angle, the others isotropic `minor` px; the keypoint noise is drawn from it.  With offsets the covariance is
    stated in crop pixels (fp32) and the image-pixel one is transform_cov_back of those very values."""
    base = T.make_case(rng, n, 0.0, 0, K, None)
    ellipse = np.zeros(n, bool)
    ellipse[rng.choice(n, n_major, replace=False)] = True
    th = rng.uniform(0, np.pi, n)
    s0, s1 = np.where(ellipse, major[0], minor), np.where(ellipse, major[1], minor)
    Rm = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    x = base.points_2d.astype(np.float64) + np.einsum("nab,nb->na", Rm, np.stack([s0, s1], -1) * rng.normal(size=(n, 2)))
    S = Rm @ (np.stack([s0 ** 2, s1 ** 2], -1)[:, :, None] * np.eye(2)) @ Rm.transpose(0, 2, 1)
    if offsets is None:
        return WCase(base._replace(points_2d=x.astype(np.float32)), as_triples(S).astype(np.float32), None)
    A = affine_from_offsets(offsets)[0]
    M, c = linear_part(offsets), np.array([A[2], A[5]])
    Mi = np.linalg.inv(M)
    crop = ((x - c) @ Mi.T).astype(np.float32)
    cov_crop = as_triples(Mi @ S @ Mi.T).astype(np.float32)
    cov_img = as_triples(E.transform_cov_back(cov_crop, offsets)).astype(np.float32)
    return WCase(base._replace(points_2d=E.transform_points_back(crop, offsets), K=K, crop=crop, offsets=offsets), cov_img, cov_crop)


# name -> (generator seed, n, cases, per-camera?).  In every set the cases i with i % 5 >= 3 have ellipses of 30 x 0.5 px instead of 8 x 0.5 px:
# such a point often lies beyond the consensus stage's 12 px, the host RANSAC seeds then find different consensus sets and start LM from
# different EPnP poses, and their stopping iterates differ -- the seed-to-seed spread the gates are made of.  With 8 px ellipses alone the four
# seeds agree bit for bit on all thirty nine-point cases, and a spread of exactly 0 says nothing.
SETS = {"shared": (41, 9, 15, False), "percam": (44, 9, 15, True), "n5": (33, 5, 5, False), "n11": (34, 11, 5, False), "n5_percam": (35, 5, 5, True),
        "n11_percam": (36, 11, 5, True)}


@functools.lru_cache(maxsize=None)
def wset(name):
    seed, n, count, percam = SETS[name]
    rng = np.random.default_rng(seed)
    n_major = 3 if n >= 9 else 1
    # (not for n = 5: there EPnP on all five points is the only start, a 10 x 12 system has a null space of dimension >= 2 of which LAPACK and Jacobi
    #  return different bases, and with a 30 px point the two starts can lie in different basins -- test_pnp_twin_host keeps n = 5 noise-free for
    #  the same reason)
    major = lambda i: (8.0, 0.5) if i % 5 < 3 or n == 5 else (30.0, 0.5)   # noqa: E731
    if percam:   # image i = case // 5 has its own K and crop offsets (test_pnp_twin_host.PERCAM_*)
        return tuple(make_wcase(rng, n, major(i), n_major=n_major, K=T.PERCAM_K[i // 5], offsets=T.PERCAM_OFFSETS[i // 5]) for i in range(count))
    return tuple(make_wcase(rng, n, major(i), n_major=n_major) for i in range(count))


def mahalanobis_cost(wc: WCase, pose) -> float:
    c, pose = wc.case, np.asarray(pose, np.float64)
    r = P.project(c.points_3d.astype(np.float64), c.K.astype(np.float64), pose[:, :3], pose[:, 3]) - c.points_2d.astype(np.float64)
    return float(np.einsum("na,nab,nb->", r, np.linalg.inv(as_matrices(wc.cov)), r))


def host_pose(wc: WCase, seed=0, weighted=True):
    c = wc.case
    return P.pnp(c.points_3d, c.points_2d, c.K, rng=np.random.default_rng(seed), cov=wc.cov if weighted else None).astype(np.float64)


@functools.lru_cache(maxsize=None)
def host_runs(name):
    poses = np.stack([[host_pose(wc, s) for s in range(4)] for wc in wset(name)])
    assert np.abs(poses).sum(axis=(2, 3)).min() > 0, "the weighted host path failed on a fixture case"
    # a case is a fixture only if its four seeds end in ONE basin: there the Mahalanobis cost is stationary and the seeds' costs agree far
    # below 1e-3, while another local minimum differs by a factor (a basin classifier, not a precision gate)
    costs = np.array([[mahalanobis_cost(wc, poses[i, s]) for s in range(4)] for i, wc in enumerate(wset(name))])
    assert (np.ptp(costs, axis=1) <= 1e-3 * costs.min(axis=1)).all(), "set %s: the host seeds end in different local minima" % name
    return poses


@functools.lru_cache(maxsize=None)
def gates() -> Gates:
    dR, dt, tmax = 0.0, 0.0, 0.0
    for member in ("shared", "percam"):
        poses = host_runs(member)
        dR = max(dR, float(np.ptp(poses[:, :, :, :3], axis=1).max()))
        dt = max(dt, float(np.ptp(poses[:, :, :, 3], axis=1).max()))
        tmax = max(tmax, float(np.abs(poses[:, :, :, 3]).max()))
    assert dR > 0 and dt > 0, "the pooled seed-to-seed spread is exactly 0: add cases, do not widen the gate"
    g = Gates(10.0 * dR + 8.0 * T.ULP_ONE, 10.0 * dt + 8.0 * float(np.spacing(np.float32(tmax))), dR, dt)
    print("weighted host path: spread R %.3g, t %.3g -> gates %.3g, %.3g" % (dR, dt, g.gate_R, g.gate_t))
    return g


def within_gates(got, want, what, g=None):
    g = g or gates()
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dR, dt = np.abs(got[..., :3] - want[..., :3]).max(), np.abs(got[..., 3] - want[..., 3]).max()
    print("%s: max |dR| %.3g (gate %.3g), max |dt| %.3g (gate %.3g)" % (what, dR, g.gate_R, dt, g.gate_t))
    assert dR <= g.gate_R and dt <= g.gate_t, "%s: max |dR| %.3g (gate %.3g), max |dt| %.3g (gate %.3g)" % (what, dR, g.gate_R, dt, g.gate_t)


def wbatch(wcases, b, oc, crop: bool):
    """-> keypoints [b,oc,n,2] (crop pixels when `crop`), model points [b,oc,n,3], covariances [b,oc,n,3] in the keypoints' pixels"""
    n = wcases[0].case.points_3d.shape[0]
    xy = np.stack([w.case.crop if crop else w.case.points_2d for w in wcases]).astype(np.float32).reshape(b, oc, n, 2)
    x3 = np.stack([w.case.points_3d for w in wcases]).reshape(b, oc, n, 3)
    cov = np.stack([w.cov_crop if crop else w.cov for w in wcases]).astype(np.float32).reshape(b, oc, n, 3)
    return xy, x3, cov


def solve_set(solver, name, host=True):
    """The set through solver.solve_host (host=False: solver.solve) with floor 0: a shared-K set as b = 1 in image pixels, a per-camera set as
    b = cases / 5 in crop pixels with the affine.  -> poses [cases,3,4] as a NumPy array"""
    ws = wset(name)
    fn = solver.solve_host if host else solver.solve
    if SETS[name][3]:
        b = len(ws) // 5
        xy, x3, cov = wbatch(ws, b, 5, True)
        out = fn(xy, x3, T.PERCAM_K[:b], np.ones((b, 5), np.int32), affine=affine_from_offsets(T.PERCAM_OFFSETS[:b]), cov=cov, cov_floor=0.0)
    else:
        xy, x3, cov = wbatch(ws, 1, len(ws), False)
        out = fn(xy, x3, T.K32, np.ones((1, len(ws)), np.int32), cov=cov, cov_floor=0.0)
    return np.asarray(out if host else out.cpu()).reshape(len(ws), 3, 4)


def test_the_twins_are_paired():
    """the header pairs the two entry points; the binding lists the pair as cp_pnp_f64's weighted variant, and twin.call finds it there"""
    assert _lib.parse_header(open(_lib.HEADER_PATH).read())[3]["cp_pnp_weighted_f64"] == "cp_pnp_weighted_host_f64"
    assert _lib.TWIN_VARIANTS == {"cp_pnp_weighted_f64": "cp_pnp_weighted_host_f64"} and "cp_pnp_weighted_f64" not in _lib.TWINS
    assert _lib.host_twin("cp_pnp_weighted_f64") == "cp_pnp_weighted_host_f64" and _lib.host_twin("cp_pnp_f64") == "cp_pnp_host_f64"
    assert _lib.host_twin("cp_pose_eval_f32") is None
    assert _lib.POINTEES["cp_pnp_weighted_f64"] == _lib.POINTEES["cp_pnp_weighted_host_f64"] + ("void",)


@pytest.mark.parametrize("name", list(SETS))
def test_twin_against_the_weighted_host_path(name):
    n = SETS[name][1]
    solver = DevicePnP(None, n)
    got = solve_set(solver, name)
    assert (solver.last_info[..., 0] == 0).all() and (solver.last_weighted == 1).all()
    cost = solver.last_cost.reshape(-1, 2)
    assert (cost[:, 1] <= cost[:, 0]).all()
    within_gates(got, host_runs(name)[:, 0], "weighted twin against pnp.pnp(cov=), set %s" % name)
    # cost[1] is the Mahalanobis cost of the returned pose
    for i, wc in enumerate(wset(name)):
        maha = mahalanobis_cost(wc, got[i])
        assert abs(cost[i, 1] - maha) <= 1e-3 * maha, (name, i, cost[i, 1], maha)


def test_identity_covariance_is_the_unweighted_solve():
    cases, ref = T.fixture_set("hard"), T.host_reference("hard")
    xy, x3 = T.batch_of(cases, 3, 5)
    solver = DevicePnP(None, 9)
    plain = solver.solve_host(xy, x3, T.K32, np.ones((3, 5), np.int32)).copy()
    assert solver.last_weighted is None
    cov = np.tile(np.float32([1, 0, 1]), (3, 5, 9, 1))
    got = solver.solve_host(xy, x3, T.K32, np.ones((3, 5), np.int32), cov=cov, cov_floor=0.0)
    assert (solver.last_weighted == 1).all()
    T.assert_within_gates(got.reshape(15, 3, 4), plain.reshape(15, 3, 4), ref, "cov = I, floor 0 against cp_pnp_host_f64")
    T.assert_within_gates(got.reshape(15, 3, 4), ref.poses, ref, "cov = I, floor 0 against pnp.pnp")


def test_a_scaled_covariance_gives_the_same_poses():
    solver = DevicePnP(None, 9)
    xy, x3, cov = wbatch(wset("shared"), 3, 5, False)
    a = solver.solve_host(xy, x3, T.K32, np.ones((3, 5), np.int32), cov=cov, cov_floor=0.0).copy()
    cost_a = solver.last_cost.copy()
    b = solver.solve_host(xy, x3, T.K32, np.ones((3, 5), np.int32), cov=3.0 * cov, cov_floor=0.0)
    within_gates(b.reshape(15, 3, 4), a.reshape(15, 3, 4), "covariance x 3")
    np.testing.assert_allclose(3.0 * solver.last_cost[..., 1], cost_a[..., 1], rtol=1e-3)


def test_crop_pixels_with_offsets_equal_image_pixels_with_the_covariance_transformed_back():
    ws = wset("percam")
    solver = DevicePnP(None, 9)
    crop = solve_set(solver, "percam")
    xy, x3, _ = wbatch(ws, 3, 5, False)
    cov_img = np.stack([as_triples(E.transform_cov_back(w.cov_crop, w.case.offsets)) for w in ws]).astype(np.float32).reshape(3, 5, 9, 3)
    image = solver.solve_host(xy, x3, T.PERCAM_K, np.ones((3, 5), np.int32), cov=cov_img, cov_floor=0.0).reshape(15, 3, 4)
    assert (solver.last_weighted == 1).all()
    within_gates(crop, image, "crop pixels + affine against image pixels + transform_cov_back")
    # transform_cov_back is M cov M^T for the linear part of transform_points_back, for both layouts
    M = linear_part(T.PERCAM_OFFSETS[0])
    c3 = ws[0].cov_crop.astype(np.float64)
    want = M @ as_matrices(c3) @ M.T
    np.testing.assert_allclose(E.transform_cov_back(c3, T.PERCAM_OFFSETS[0]), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(E.transform_cov_back(as_matrices(c3), T.PERCAM_OFFSETS[0]), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", ["singular", "nan", "negative", "inf"])
def test_an_unusable_covariance_falls_back_alone(kind):
    solver = DevicePnP(None, 9)
    xy, x3, cov = wbatch(wset("shared")[:3], 1, 3, False)
    ones = np.ones((1, 3), np.int32)
    full = solver.solve_host(xy, x3, T.K32, ones, cov=cov, cov_floor=0.0).copy()
    plain = solver.solve_host(xy, x3, T.K32, ones).copy()
    plain_info, plain_cost = solver.last_info.copy(), solver.last_cost.copy()
    bad = cov.copy()
    bad[0, 1, 4] = {"singular": (1.0, 2.0, 4.0), "nan": (1.0, np.nan, 1.0), "negative": (-1.0, 0.0, 1.0), "inf": (np.inf, 0.0, 1.0)}[kind]
    got = solver.solve_host(xy, x3, T.K32, ones, cov=bad, cov_floor=0.0)
    assert solver.last_weighted.tolist() == [[1, 0, 1]]
    assert got[0, 1].tobytes() == plain[0, 1].tobytes() and solver.last_info[0, 1].tobytes() == plain_info[0, 1].tobytes()
    assert solver.last_cost[0, 1].tobytes() == plain_cost[0, 1].tobytes()
    assert np.array_equal(got[0, 0], full[0, 0]) and np.array_equal(got[0, 2], full[0, 2])
    assert not np.array_equal(full[0, 1], plain[0, 1])       # the weights mattered for that pair
    if kind == "singular":   # the host path ignores an unusable set too
        c = wset("shared")[1].case
        a = P.pnp(c.points_3d, c.points_2d, c.K, rng=np.random.default_rng(0), cov=bad[0, 1])
        assert np.array_equal(a, P.pnp(c.points_3d, c.points_2d, c.K, rng=np.random.default_rng(0)))


def test_the_floor_rescues_a_zero_covariance_and_a_skipped_pair_stays_skipped():
    solver = DevicePnP(None, 9)
    xy, x3, _ = wbatch(wset("shared")[:3], 1, 3, False)
    zero = np.zeros((1, 3, 9, 3), np.float32)
    mask = np.array([[1, 0, 1]], np.int32)
    solver.solve_host(xy, x3, T.K32, mask, cov=zero, cov_floor=0.0)
    assert solver.last_weighted.tolist() == [[0, 0, 0]] and solver.last_info[0, :, 0].tolist() == [0, 1, 0]
    plain = solver.solve_host(xy, x3, T.K32, mask).copy()
    got = solver.solve_host(xy, x3, T.K32, mask, cov=zero)       # the default floor, 1/12 px^2
    assert solver.last_weighted.tolist() == [[1, 0, 1]] and solver.last_info[0, 1].tolist() == [1, -1, 0, 0] and not got[0, 1].any()
    within_gates(got[0, [0, 2]], plain[0, [0, 2]], "isotropic floor against the unweighted solve")


def test_argument_refusals_by_name():
    """the pointers named below are never dereferenced: every refusal comes before the first pair"""
    solver = DevicePnP(None, 9)
    xy, x3, cov = wbatch(wset("shared")[:3], 1, 3, False)
    ones = np.ones((1, 3), np.int32)
    out = twin.alloc(dict(poses=((1, 3, 3, 4), np.float32), info=((1, 3, 4), np.int32), cost=((1, 3, 2), np.float32), weighted=((1, 3), np.int32)))
    head = (xy, x3, T.K32, 0, None, ones, solver.table_host, 1, 3, 9, solver.hypotheses, 12.0)
    with pytest.raises(_lib.CasaposeHipError, match="cp_pnp_weighted_host_f64: cov is a null pointer.*cp_pnp_f64"):
        twin.call("cp_pnp_weighted_f64", *head, None, 0.0, out["poses"], out["info"], out["cost"], out["weighted"], host=True)
    with pytest.raises(_lib.CasaposeHipError, match="cp_pnp_weighted_host_f64: weighted is a null pointer"):
        twin.call("cp_pnp_weighted_f64", *head, cov, 0.0, out["poses"], out["info"], out["cost"], None, host=True)
    for floor in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.CasaposeHipError, match="cp_pnp_weighted_host_f64: cov_floor"):
            twin.call("cp_pnp_weighted_f64", *head, cov, floor, out["poses"], out["info"], out["cost"], out["weighted"], host=True)
    with pytest.raises(_lib.CasaposeHipError, match="cp_pnp_weighted_host_f64: null pointer"):
        twin.call("cp_pnp_weighted_f64", *head, cov, 0.0, None, out["info"], out["cost"], out["weighted"], host=True)
    with pytest.raises(_lib.CasaposeHipError, match=r"argument 12 \(float\*\): the array holds float64"):
        twin.call("cp_pnp_weighted_f64", *head, cov.astype(np.float64), 0.0, out["poses"], out["info"], out["cost"], out["weighted"], host=True)
    with pytest.raises(ValueError, match="cov must be"):
        solver.solve_host(xy, x3, T.K32, ones, cov=cov[:, :, :8])
    with pytest.raises(ValueError, match="cov must be"):
        P.refine_lm(x3[0, 0], xy[0, 0], T.K32, np.zeros(3), np.array([0.0, 0.0, 800.0]), cov=np.zeros((9, 4)))


def test_estimate_poses_passes_the_covariance_to_either_pnp():
    ws = wset("percam")[:10]
    xy, x3, cov = wbatch(ws, 2, 5, True)
    valid, offs, cams = np.ones((2, 5), np.float32), T.PERCAM_OFFSETS[:2], T.PERCAM_K[:2]
    solver = HostTwinPnP(9)
    got, _ = E.estimate_poses(xy, x3[:, :, None], cams, valid, offs, solver=solver, cov=cov)
    assert (solver.last_weighted == 1).all()
    want, _ = E.estimate_poses(xy, x3[:, :, None], cams, valid, offs, rng=np.random.default_rng(0), cov=cov)
    within_gates(got, want, "estimate_poses(cov=) with the twin against the host path")
    plain, _ = E.estimate_poses(xy, x3[:, :, None], cams, valid, offs, rng=np.random.default_rng(0))
    assert np.abs(want[..., 3] - plain[..., 3]).max() > 100 * gates().gate_t       # the covariance reached the host path


def test_poses_pnp_passes_the_covariance_to_either_pnp(monkeypatch):
    monkeypatch.delenv("CASAPOSE_UNCERTAINTY_PNP", raising=False)
    xy, x3, cov = wbatch(wset("shared")[:3], 1, 3, False)
    seg = np.zeros((1, 6, 8, 4), np.float32)
    seg[0, :, :, 0] = 1.0
    for o in range(3):       # 6 pixels per object, more than min_num = 2
        seg[0, 2 * o, 1:7] = np.eye(4, dtype=np.float32)[o + 1]
    solver = HostTwinPnP(9)
    yx = xy[..., ::-1]
    got = E.poses_pnp(yx, seg, x3, T.K32, 3, min_num=2, solver=solver, cov=cov)
    assert (solver.last_weighted == 1).all() and got.shape == (1, 3, 1, 3, 4)
    want = E.poses_pnp(yx, seg, x3, T.K32, 3, min_num=2, rng=np.random.default_rng(0), cov=cov)
    within_gates(got[:, :, 0], want[:, :, 0], "poses_pnp(cov=) with the twin against the host path")
    plain = E.poses_pnp(yx, seg, x3, T.K32, 3, min_num=2, rng=np.random.default_rng(0))
    assert np.abs(want[..., 3] - plain[..., 3]).max() > 100 * gates().gate_t
    monkeypatch.setenv("CASAPOSE_UNCERTAINTY_PNP", "1")       # under the switch a call without a covariance is refused by name
    with pytest.raises(ValueError, match="poses_pnp: CASAPOSE_UNCERTAINTY_PNP=1 needs cov="):
        E.poses_pnp(yx, seg, x3, T.K32, 3, min_num=2, rng=np.random.default_rng(0))
    assert np.array_equal(E.poses_pnp(yx, seg, x3, T.K32, 3, min_num=2, rng=np.random.default_rng(0), cov=cov), want)


# ---- the statistical case: what the weights are for -------------------------------------------------------------------------------------------------
def pose_errors(poses, wcases):
    """(rotation error in degrees, translation error in mm) per case"""
    rot, tr = [], []
    for p, w in zip(np.asarray(poses, np.float64), wcases):
        g = w.case.pose_gt
        c = np.clip((np.trace(p[:, :3].T @ g[:, :3]) - 1.0) / 2.0, -1.0, 1.0)
        rot.append(np.degrees(np.arccos(c)))
        tr.append(np.linalg.norm(p[:, 3] - g[:, 3]))
    return np.array(rot), np.array(tr)


@functools.lru_cache(maxsize=None)
def statistical_cases():
    rng = np.random.default_rng(40)
    return tuple(make_wcase(rng, 9) for _ in range(64))       # nine points: three with an 8 x 0.5 px ellipse, six at 0.3 px


def assert_weighting_halves_the_errors(weighted, unweighted, what):
    ws = statistical_cases()
    (rw, tw), (ru, tu) = pose_errors(weighted, ws), pose_errors(unweighted, ws)
    print("%s: median rotation error %.3g deg weighted, %.3g unweighted (ratio %.2f); translation %.3g mm, %.3g mm (ratio %.2f)"
          % (what, np.median(rw), np.median(ru), np.median(rw) / np.median(ru), np.median(tw), np.median(tu), np.median(tw) / np.median(tu)))
    assert np.median(rw) <= 0.5 * np.median(ru) and np.median(tw) <= 0.5 * np.median(tu), what


def test_weighting_halves_the_median_pose_errors():
    ws = statistical_cases()
    assert_weighting_halves_the_errors([host_pose(w) for w in ws], [host_pose(w, weighted=False) for w in ws], "host path")       # first
    solver = DevicePnP(None, 9)
    xy, x3, cov = wbatch(ws, 8, 8, False)
    ones = np.ones((8, 8), np.int32)
    plain = solver.solve_host(xy, x3, T.K32, ones).reshape(64, 3, 4).copy()
    got = solver.solve_host(xy, x3, T.K32, ones, cov=cov, cov_floor=0.0).reshape(64, 3, 4)
    assert (solver.last_weighted == 1).all() and (solver.last_info[..., 0] == 0).all()
    assert_weighting_halves_the_errors(got, plain, "twin")
