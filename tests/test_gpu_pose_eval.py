"""cp_pose_eval_f32 (csrc/pose_eval.hip) and DevicePoseEvaluator on the GPU against the host evaluate_poses in fp64 (records) and a NumPy fp64
brute force (per-point distances), both fed the same fp32-rounded inputs as the device.

Gates (derived from the arithmetic, not from what the kernel gives).  S = the largest |camera-frame coordinate| of a test, every test keeps
z >= S / 2 (asserted):
  3-D, per-point distances and per-pair means: |dev - ref| <= 4e-6 * S.  A transformed coordinate is three fp32 FMAs, <= 3 * 2^-24 * S per point;
      a distance takes two points and three coordinates: about 6e-7 * S, so the gate leaves about 6x.
  2-D: |dev - ref| <= 2e-6 * (f + max(W, H)): the same argument through the projection, about 6x margin.
Flags and counts must match exactly; the ordinary pairs are built (and asserted, on the fp64 values) at least 1 % away from both thresholds.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "config_8.ini")
K32 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
GATE_2D = 2e-6 * (float(K32[1, 1]) + 640.0)


def gate_3d(s):
    return 4e-6 * s


def rodrigues(rv):
    from casapose_amd.pose_estimation import pnp as P

    return P.rodrigues(np.asarray(rv, np.float64))


def pose32(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32)


def per_point_reference(mesh, est, gt, K, symmetric):
    """fp64 brute force on the fp32-rounded inputs -> (e2 [n], e3 [n], S, smallest z)"""
    from casapose_amd.pose_estimation.pose_evaluation import project

    X, est, gt, K = (np.asarray(a, np.float64) for a in (mesh, est, gt, K))
    p2, p3 = project(X, K, est)
    t2, t3 = project(X, K, gt)
    e2 = np.linalg.norm(t2 - p2, axis=1)
    if symmetric:
        d2 = np.full(len(X), np.inf)
        for j0 in range(0, len(X), 512):
            d = t3[:, None, :] - p3[None, j0:j0 + 512, :]
            d2 = np.minimum(d2, (d * d).sum(-1).min(axis=1))
        e3 = np.sqrt(np.abs(d2) + 1e-5)
    else:
        e3 = np.linalg.norm(t3 - p3, axis=1)
    return e2, e3, max(np.abs(p3).max(), np.abs(t3).max()), min(p3[:, 2].min(), t3[:, 2].min())


def host_records(monkeypatch, poses, gt, mesh, counts, cams, diam, valid, flags, allowed=5.0):
    """The host evaluate_poses (fp64) image by image -> records [b, oc, 6] in the device's column order.  ADD-S is routed by vertex count on the
    host, so the counts of the flagged objects stand in for SYMMETRIC_VERTEX_COUNTS."""
    from casapose_amd.pose_estimation import pose_evaluation as E

    counts = np.asarray(counts).reshape(-1)
    flagged = tuple(int(c) for c, f in zip(counts, flags) if f)
    assert not set(flagged) & {int(c) for c, f in zip(counts, flags) if not f}
    b, oc = gt.shape[0], gt.shape[1]
    out = np.zeros((b, oc, 6))
    with monkeypatch.context() as m:
        m.setattr(E, "SYMMETRIC_VERTEX_COUNTS", flagged)
        pts, cnt = E._eval_points(None, mesh, counts.reshape(oc, 1), 1, oc, 1)
        for n in range(b):
            e2, e3, v2, v3, miss, _, fp = E.evaluate_poses(poses[n:n + 1], gt[n:n + 1], None, pts, cnt, cams[n:n + 1], diam[n:n + 1], valid[n:n + 1], allowed)
            out[n] = np.stack([e2, e3, v3, v2, miss, fp], axis=1)
    return out


def assert_records(got, ref, s, where=""):
    assert np.all(np.isfinite(got)), where
    print("%s max |err_2d - ref| = %.3g (gate %.3g), max |err_3d - ref| = %.3g (gate %.3g)" % (
        where, np.abs(got[..., 0] - ref[..., 0]).max(), GATE_2D, np.abs(got[..., 1] - ref[..., 1]).max(), gate_3d(s)))
    assert np.array_equal(got[..., 2:], ref[..., 2:]), where            # valid_3d, valid_2d, missing, false_positive
    assert np.abs(got[..., 0] - ref[..., 0]).max() <= GATE_2D, where
    assert np.abs(got[..., 1] - ref[..., 1]).max() <= gate_3d(s), where


# ---- 1. ring meshes ---------------------------------------------------------------------------------------------------------------------
RING_SIZES = ["1", "63", "64", "65", "255", "256", "257", "T-1", "T", "T+1", "2*T+1"]      # T = cp_pose_eval_est_tile()


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("size", RING_SIZES)
def test_ring_meshes(device, hip_lib, monkeypatch, size, symmetric):
    """Object points 60 (cos 2 pi i / n, sin 2 pi i / n, 0); the estimated pose is the ground truth turned by k ring steps, so every estimated point
    is the nearest neighbour of exactly one target: ADD is the chord (about 102 - 104), ADD-S is sqrt(1e-5) = 3.1623e-3.  A dropped, duplicated or
    mis-tiled estimated point moves one per-point ADD-S to at least the ring spacing (0.18 at the largest n)."""
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    T = hip_lib.cp_pose_eval_est_tile()
    n = eval(size, {"T": T})
    k = max(1, n // 3)
    a = 2.0 * np.pi * np.arange(n) / n
    mesh = np.stack([60.0 * np.cos(a), 60.0 * np.sin(a), np.zeros(n)], axis=1).astype(np.float32)
    Rg, t = rodrigues([0.4, -0.7, 0.3]), [30.0, -20.0, 900.0]
    th = 2.0 * np.pi * k / n
    Rz = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    gt, est = pose32(Rg, t), pose32(Rg @ Rz, t)
    padded = np.full((1, n + 5, 3), np.nan, np.float32)            # rows n .. vmax-1 must never be read
    padded[0, :n] = mesh
    diam, valid = np.full((1, 1, 1), 120.0, np.float32), np.ones((1, 1), np.float32)

    e2, e3, s, zmin = per_point_reference(mesh, est, gt, K32, symmetric)
    assert zmin >= s / 2
    ref = host_records(monkeypatch, est[None, None], gt[None, None, None], padded, [n], K32[None], diam, valid, [symmetric])
    if n >= 63:
        if symmetric:
            assert abs(ref[0, 0, 1] - 3.1623e-3) < 1e-6 and ref[0, 0, 2] == 1.0
        else:
            assert 100.0 < ref[0, 0, 1] < 105.0 and ref[0, 0, 2] == 0.0
    # the two references agree (the host returns its fp64 means rounded to fp32)
    assert abs(ref[0, 0, 0] - e2.mean()) <= 1e-7 * e2.mean() + 1e-12 and abs(ref[0, 0, 1] - e3.mean()) <= 1e-7 * e3.mean() + 1e-12

    ev = DevicePoseEvaluator(padded, [n], device, symmetric=[symmetric])
    ev.evaluate(est[None, None], gt[None, None, None], K32[None], diam, valid, 5.0, point_errors=True)
    d2, d3 = (x[0, 0] for x in ev.last_point_errors)
    assert d2.shape == (n + 5,) and np.all(np.isfinite(d2)) and np.all(np.isfinite(d3))
    assert np.all(d2[n:] == 0) and np.all(d3[n:] == 0)
    print("ring n=%d sym=%d: per-point max |e2 - ref| = %.3g, max |e3 - ref| = %.3g" % (n, symmetric, np.abs(d2[:n] - e2).max(), np.abs(d3[:n] - e3).max()))
    assert np.abs(d2[:n] - e2).max() <= GATE_2D
    assert np.abs(d3[:n] - e3).max() <= gate_3d(s)
    assert_records(ev.last_records, ref, s, "ring n=%d sym=%d:" % (n, symmetric))


# ---- 2. case logic ----------------------------------------------------------------------------------------------------------------------
def case_scene():
    """b = 2, oc = 4, vmax = 705 with NaN padding: counts (300, 257, 64, 700), ADD-S for objects 1 and 3."""
    rng = np.random.default_rng(21)
    b, oc, counts, flags = 2, 4, [300, 257, 64, 700], [0, 1, 0, 1]
    mesh = np.full((oc, 705, 3), np.nan, np.float32)
    for o, c in enumerate(counts):
        mesh[o, :c] = rng.uniform(-50, 50, (c, 3))
    gt = np.zeros((b, oc, 1, 3, 4), np.float32)
    est = np.zeros((b, oc, 3, 4), np.float32)
    near, far = np.array([1.0, -0.5, 2.0]), np.array([80.0, -60.0, 100.0])
    for n in range(b):
        for o in range(oc):
            R, t = rodrigues(rng.normal(0, 0.6, 3)), np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(750, 850)])
            gt[n, o, 0] = pose32(R, t)
            good = (n + o) % 2 == 0
            est[n, o] = pose32(R @ rodrigues([0.0, 0.0, 0.0 if good else 0.4]), t + (near if good else far))
    valid = np.ones((b, oc), np.float32)
    valid[0, 1] = 0                       # not in the ground truth, non-zero pose: a false positive
    valid[0, 2] = 0                       # not in the ground truth, zero pose: nothing
    est[0, 2] = 0
    est[0, 3] = 0                         # in the ground truth, zero pose: missing
    cams = np.stack([K32, K32 + np.array([[3.0, 0, -2.0], [0, 2.0, 1.5], [0, 0, 0]], np.float32)])
    diam = np.array([[110.0, 120.0, 95.0, 130.0]] * b, np.float32)[:, :, None]
    return dict(mesh=mesh, counts=counts, flags=flags, gt=gt, est=est, valid=valid, cams=cams, diam=diam)


def test_case_logic_in_one_launch(device, monkeypatch):
    from casapose_amd.pose_estimation import pose_evaluation as E
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    sc = case_scene()
    ref = host_records(monkeypatch, sc["est"], sc["gt"], sc["mesh"], sc["counts"], sc["cams"], sc["diam"], sc["valid"], sc["flags"])
    assert list(ref[0, 1]) == [0, 0, 0, 0, 0, 1] and list(ref[0, 2]) == [0] * 6 and np.allclose(ref[0, 3], [99.9, 999.9, 0, 0, 1, 0])
    ordinary = [(0, 0)] + [(1, o) for o in range(4)]
    s = 0.0
    for n, o in ordinary:                  # every ordinary pair is at least 1 % away from both thresholds, on the fp64 reference
        e2, e3 = ref[n, o, 0], ref[n, o, 1]
        assert abs(e3 - 0.1 * sc["diam"][n, o, 0]) >= 0.01 * 0.1 * sc["diam"][n, o, 0] and abs(e2 - 5.0) >= 0.05, (n, o, e2, e3)
        _, _, sp, zmin = per_point_reference(sc["mesh"][o, :sc["counts"][o]], sc["est"][n, o], sc["gt"][n, o, 0], sc["cams"][n], 0)
        s = max(s, sp)
        assert zmin >= sp / 2
    assert {tuple(ref[n, o, 2:4]) for n, o in ordinary} == {(1.0, 1.0), (0.0, 0.0)}      # both outcomes occur

    ev = DevicePoseEvaluator(sc["mesh"], sc["counts"], device, symmetric=sc["flags"])
    got = ev.evaluate(sc["est"], sc["gt"], sc["cams"], sc["diam"], sc["valid"], 5.0, point_errors=True)
    assert ev.last_records.shape == (2, 4, 6) and ev.last_records.dtype == np.float32
    assert_records(ev.last_records, ref, s, "case logic:")
    assert all(np.all(np.isfinite(x)) for x in ev.last_point_errors)
    # all seven returned arrays against the host's (one call over the whole batch)
    monkeypatch.setattr(E, "SYMMETRIC_VERTEX_COUNTS", (257, 700))
    pts, cnt = E._eval_points(None, sc["mesh"], np.array(sc["counts"]).reshape(4, 1), 2, 4, 1)
    want = E.evaluate_poses(sc["est"], sc["gt"], None, pts, cnt, sc["cams"], sc["diam"], sc["valid"], 5.0)
    assert len(got) == len(want) == 7
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape == (4,) and g.dtype == w.dtype == np.float32
        if i == 0:      # err_2d, err_3d: sums over two images (the 99.9 / 999.9 sentinels add an fp32 rounding of the sum)
            assert np.abs(g - w).max() <= 2 * GATE_2D + 1e-5
        elif i == 1:
            assert np.abs(g - w).max() <= 2 * gate_3d(s) + 1e-4
        else:
            assert np.array_equal(g, w), i
    assert list(got[5]) == [2, 1, 1, 2] and list(got[4]) == [0, 0, 0, 1] and list(got[6]) == [0, 1, 0, 0]

    # two calls on the same input: bit-identical records and per-point values
    first, first_pts = ev.last_records.copy(), [x.copy() for x in ev.last_point_errors]
    ev.evaluate(sc["est"], sc["gt"], sc["cams"], sc["diam"], sc["valid"], 5.0, point_errors=True)
    assert first.tobytes() == ev.last_records.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first_pts, ev.last_point_errors))


# ---- 3. exact values --------------------------------------------------------------------------------------------------------------------
def test_exact_values(device, monkeypatch):
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    # camera z exactly 0 under the estimated pose: the pixel is (0, 0) (divide_no_nan), so the 2-D distance is |ground-truth pixel|
    mesh = np.array([[[0.0, 0.0, -5.0]]], np.float32)
    est, gt = pose32(np.eye(3), [0.0, 0.0, 5.0]), pose32(np.eye(3), [0.0, 0.0, 905.0])
    diam, valid = np.full((1, 1, 1), 100.0, np.float32), np.ones((1, 1), np.float32)
    ref = host_records(monkeypatch, est[None, None], gt[None, None, None], mesh, [1], K32[None], diam, valid, [0])
    assert abs(ref[0, 0, 0] - np.hypot(float(K32[0, 2]), float(K32[1, 2]))) < 1e-4 and ref[0, 0, 1] == 900.0
    ev = DevicePoseEvaluator(mesh, [1], device, symmetric=[0])
    ev.evaluate(est[None, None], gt[None, None, None], K32[None], diam, valid, 5.0, point_errors=True)
    assert_records(ev.last_records, ref, 900.0, "z = 0:")
    assert abs(ev.last_point_errors[0][0, 0, 0] - ref[0, 0, 0]) <= GATE_2D and ev.last_point_errors[1][0, 0, 0] == 900.0

    # identical poses: ADD = 0 and the 2-D error = 0 exactly; ADD-S = sqrt(1e-5) to fp32 rounding: the constant rounds to fp32 (2^-25 after the
    # root) and the root is within one ulp (2^-23), together below 2^-22
    rng = np.random.default_rng(3)
    T = ev._lib.cp_pose_eval_est_tile()
    n = T + 300
    mesh = rng.uniform(-50, 50, (2, n, 3)).astype(np.float32)
    pose = pose32(rodrigues([0.3, 0.2, -0.5]), [12.0, -7.0, 820.0])
    poses = np.stack([pose, pose])[None]
    diam, valid = np.full((1, 2, 1), 100.0, np.float32), np.ones((1, 2), np.float32)
    ev = DevicePoseEvaluator(mesh, [n, n - 3], device, symmetric=[0, 1])
    ev.evaluate(poses, poses[:, :, None], K32, diam, valid, 5.0, point_errors=True)
    e2, e3 = ev.last_point_errors
    assert np.all(e2 == 0) and np.all(e3[0, 0] == 0) and list(ev.last_records[0, 0]) == [0, 0, 1, 1, 0, 0]
    root = np.sqrt(1e-5)
    assert np.abs(e3[0, 1, :n - 3] - root).max() <= 2.0 ** -22 * root and np.all(e3[0, 1, n - 3:] == 0)
    assert abs(ev.last_records[0, 1, 1] - root) <= 2.0 ** -22 * root and list(ev.last_records[0, 1, [0, 2, 3, 4, 5]]) == [0, 1, 1, 0, 0]


# ---- 4. the evaluator through Python, at the workload's shape ---------------------------------------------------------------------------
def test_evaluator_routes_adds_by_vertex_count(device):
    """b = 1, oc = 8, random meshes whose counts include 7862 and 3417; no explicit flags, and the host path (cKDTree) as it stands."""
    from casapose_amd.pose_estimation import pose_evaluation as E
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    rng = np.random.default_rng(8)
    counts = np.array([5841, 7862, 300, 3417, 9000, 1024, 2000, 4500], np.int32)
    oc, vmax = len(counts), int(counts.max())
    mesh = np.zeros((oc, vmax, 3), np.float32)
    for o, c in enumerate(counts):
        mesh[o, :c] = rng.uniform(-50, 50, (c, 3))
    gt = np.zeros((1, oc, 1, 3, 4), np.float32)
    est = np.zeros((1, oc, 3, 4), np.float32)
    for o in range(oc):
        R, t = rodrigues(rng.normal(0, 0.6, 3)), np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(750, 850)])
        gt[0, o, 0] = pose32(R, t)
        good = o % 2 == 1
        est[0, o] = pose32(R @ rodrigues([0.05, -0.03, 0.1] if good else [0.0, 0.3, 0.4]), t + ([1.0, -0.5, 2.0] if good else [80.0, -60.0, 100.0]))
    valid = np.ones((1, oc), np.float32)
    diam = np.full((1, oc, 1), 120.0, np.float32)
    ev = DevicePoseEvaluator(mesh, counts.reshape(oc, 1), device)
    assert list(ev.symmetric_host) == [0, 1, 0, 1, 0, 0, 0, 0]
    got = ev.evaluate(est, gt, K32[None], diam, valid)
    pts, cnt = E._eval_points(None, mesh, counts.reshape(oc, 1), 1, oc, 1)
    want = E.evaluate_poses(est, gt, None, pts, cnt, K32[None], diam, valid, 5.0)
    ref = np.stack([want[0], want[1], want[3], want[2], want[4], want[6]], axis=1).astype(np.float64)[None]
    s, zmin = 0.0, np.inf
    for o in range(oc):
        X = mesh[o, :counts[o]].astype(np.float64)
        cams = [X @ p[:, :3].astype(np.float64).T + p[:, 3].astype(np.float64) for p in (est[0, o], gt[0, o, 0])]
        s, zmin = max(s, max(np.abs(c).max() for c in cams)), min(zmin, min(c[:, 2].min() for c in cams))
        assert abs(ref[0, o, 1] - 12.0) >= 0.12 and abs(ref[0, o, 0] - 5.0) >= 0.05, (o, ref[0, o])
    # ADD-S is what the two flagged objects got: their ADD would be several millimetres larger
    add1 = np.linalg.norm(mesh[1, :7862].astype(np.float64) @ (est[0, 1, :, :3].astype(np.float64) - gt[0, 1, 0, :, :3].astype(np.float64)).T
                          + (est[0, 1, :, 3] - gt[0, 1, 0, :, 3]).astype(np.float64), axis=1).mean()
    assert add1 > ref[0, 1, 1] + 1.0 and zmin >= s / 2
    assert_records(ev.last_records, ref, s, "evaluator, oc = 8:")
    assert np.array_equal(got[5], want[5]) and all(g.dtype == np.float32 and g.shape == (oc,) for g in got)


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_pose_estimates_with_and_without_an_evaluator(device):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator
    from casapose_amd.pose_estimation.pose_evaluation import evaluate_pose_estimates

    oc = 4
    ds = SyntheticSceneDataset(oc, (120, 160), length=2, seed=5, random_crop=False)
    batch = ds.batch(0, 2)
    mesh, counts = ds.generate_object_vertex_array()
    gt = batch["poses_gt"].numpy()
    poses = gt[:, :, 0].copy()
    poses[..., 3] += np.array([1.0, -0.5, 2.0], np.float32)
    pts = np.zeros((2, oc, 9, 2), np.float32)
    args = (pts, poses, batch["poses_gt"], batch["target_seg"], batch["keypoints3d"], batch["cam_mat"], batch["diameters"])
    host, _, _ = evaluate_pose_estimates(*args, evaluation_points=mesh, object_points_3d_count=counts, min_num=20)
    ev = DevicePoseEvaluator(mesh, counts, device)
    dev, p_out, pts_out = evaluate_pose_estimates(*args, evaluation_points=mesh, object_points_3d_count=counts, min_num=20, evaluator=ev)
    assert p_out is poses and pts_out is pts and len(dev) == 8
    cam = np.einsum("boij,ovj->bovi", gt[:, :, 0, :, :3].astype(np.float64), mesh.astype(np.float64)) + gt[:, :, 0, None, :, 3]
    s = np.abs(cam).max() + 3.0
    assert cam[..., 2].min() >= s / 2
    assert host[2].sum() >= 6 and host[7].sum() >= 1                      # the batch has objects in and out of the ground truth
    for i in (0, 1, 2, 3, 6, 7):
        assert np.array_equal(dev[i], host[i]) and dev[i].dtype == host[i].dtype, i
    assert np.array_equal(host[0], host[2]) and np.array_equal(host[1], host[2])         # 2.3 mm off: every object in the GT is correct
    assert np.abs(dev[4] - host[4]).max() <= 2 * GATE_2D and np.abs(dev[5] - host[5]).max() <= 2 * gate_3d(s)


def test_test_script_with_device_evaluation(device, tmp_path, monkeypatch, capsys):
    """test_casapose.py with CASAPOSE_DEVICE_EVAL=1: it runs, says so, the evaluator is what computes the statistics, and the results are finite.
    (No numbers are compared: an untrained network's poses are ill-conditioned.)"""
    import test_casapose
    from casapose_amd.pose_estimation import device_evaluation as D
    from casapose_amd.pose_estimation import pose_evaluation as E

    calls = []
    inner = D.DevicePoseEvaluator.evaluate

    def counted(self, *a, **k):
        out = inner(self, *a, **k)
        calls.append(self.last_records.copy())
        return out

    def refuse(*a, **k):
        raise AssertionError("the host statistics ran although CASAPOSE_DEVICE_EVAL=1")

    monkeypatch.setattr(D.DevicePoseEvaluator, "evaluate", counted)
    monkeypatch.setattr(E, "evaluate_poses", refuse)
    monkeypatch.setenv("CASAPOSE_DEVICE_EVAL", "1")
    out = str(tmp_path / "run")
    res = test_casapose.main(["-c", CFG, "--outf", out, "--manualseed", "7", "--workers", "0", "--datatest", "synthetic:2", "--net", "", "--pretrained", "0"])
    assert "pose evaluation: device" in capsys.readouterr().out
    assert len(calls) == 2 and all(r.shape == (1, 8, 6) and np.all(np.isfinite(r)) for r in calls)
    assert all(np.all(np.isfinite(res[k])) for k in ("loss", "valid_2d", "valid_3d", "precision")) and res["valid_3d"].shape == (8,)
