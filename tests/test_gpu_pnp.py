"""`cp_pnp_f64` on the GPU (csrc/pnp.hip through `DevicePnP`) against the host path `pnp.pnp`, at the smallest shapes at which the kernel can go
wrong.  Cases, references and gates are those of tests/test_pnp_twin_host.py (gates from the host path's own seed-to-seed spread, never from the
device or its twin).  `info` (winning hypothesis, inlier count) is compared with the host twin's: integers from the same code."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_pnp_twin_host as T
from casapose_amd.pose_estimation.device_pnp import DevicePnP, affine_from_offsets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def solve_both(device, cases, b, oc, K, mask, affine=None):
    """-> (device poses [b*oc,3,4], device info, device cost, twin info): the same call on the GPU and through the host twin"""
    n = cases[0].points_3d.shape[0]
    xy, x3 = T.batch_of(cases, b, oc)
    dev, twin = DevicePnP(device, n), DevicePnP(None, n)
    poses = dev.solve(xy, x3, K, mask, affine=affine)
    assert poses.is_cuda and tuple(poses.shape) == (b, oc, 3, 4) and poses.dtype.is_floating_point
    twin.solve_host(xy, x3, K, mask, affine=affine)
    return poses.cpu().numpy().reshape(b * oc, 3, 4), dev.last_info.reshape(b * oc, 4), dev.last_cost.reshape(b * oc, 2), twin.last_info.reshape(b * oc, 4)


def compare_info(info, twin_info, what):
    """Status always; winner and inlier count unless a fused multiply-add flipped a tie between two hypotheses, which is said, and then the
    poses (compared by every caller anyway) are what counts."""
    assert np.array_equal(info[:, 0], twin_info[:, 0]), what
    if not np.array_equal(info[:, 1:3], twin_info[:, 1:3]):
        rows = np.flatnonzero((info[:, 1:3] != twin_info[:, 1:3]).any(axis=1))
        print("%s: winner / inlier count differ from the twin in pairs %s (device %s, twin %s): a tie flipped by FMA contraction; falling back "
              "to the pose comparison" % (what, rows.tolist(), info[rows, 1:3].tolist(), twin_info[rows, 1:3].tolist()))
        assert (np.abs(info[rows, 2] - twin_info[rows, 2]) <= 1).all(), what


def test_one_block(device):
    """b = 1, oc = 1, n = 9: 126 hypotheses = one full wave and 62 lanes of the next, two idle waves"""
    cases, ref = T.fixture_set("hard")[6:7], T.host_reference("hard")
    poses, info, cost, twin_info = solve_both(device, cases, 1, 1, T.K32, np.ones((1, 1), np.int32))
    compare_info(info, twin_info, "one block")
    assert info[0, 0] == 0 and info[0, 2] >= 8 and 1 <= info[0, 3] <= 20 and cost[0, 1] <= cost[0, 0]
    T.assert_within_gates(poses, ref.poses[6:7], ref, "device against pnp.pnp, one block")
    T.assert_costs_within_gate(cases, poses, ref._replace(costs=ref.costs[6:7]), "device against pnp.pnp, one block")


def test_batch_shared_camera(device):
    """b = 3, oc = 5, mixed solve flags, K [3,3] shared, no affine"""
    cases, ref = T.fixture_set("hard"), T.host_reference("hard")
    mask = T.PERCAM_MASK
    on = mask.reshape(15) != 0
    poses, info, cost, twin_info = solve_both(device, cases, 3, 5, T.K32, mask)
    compare_info(info, twin_info, "shared K")
    assert np.array_equal(info[:, 0], np.where(on, 0, 1)) and not poses[~on].any() and not cost[~on].any()
    for i in np.flatnonzero(on):
        assert info[i, 2] >= 9 - cases[i].outliers
    T.assert_within_gates(poses[on], ref.poses[on], ref, "device against pnp.pnp, shared K")
    T.assert_costs_within_gate([c for c, o in zip(cases, on) if o], poses[on], ref._replace(costs=ref.costs[on]), "device against pnp.pnp, shared K")


def test_batch_per_image_camera_and_affine(device):
    """b = 3, oc = 5, mixed solve flags, K [b,3,3], crop pixels with the crop->image affine of every image"""
    cases, ref = T.fixture_set("percam"), T.host_reference("percam")
    mask = T.PERCAM_MASK
    on = mask.reshape(15) != 0
    poses, info, cost, twin_info = solve_both(device, cases, 3, 5, T.PERCAM_K, mask, affine_from_offsets(T.PERCAM_OFFSETS))
    compare_info(info, twin_info, "per-image K and affine")
    assert np.array_equal(info[:, 0], np.where(on, 0, 1)) and not poses[~on].any()
    T.assert_within_gates(poses[on], ref.poses[on], ref, "device against pnp.pnp, per-image K and affine")
    T.assert_costs_within_gate([c for c, o in zip(cases, on) if o], poses[on], ref._replace(costs=ref.costs[on]),
                               "device against pnp.pnp, per-image K and affine")


@pytest.mark.parametrize("name", ["n5", "n10", "n11"])
def test_other_point_counts(device, name):
    """n = 5: one hypothesis and 255 idle threads; n = 10: 252 hypotheses; n = 11: the sampled table of 256"""
    cases, ref = T.fixture_set(name), T.host_reference(name)
    n = cases[0].points_3d.shape[0]
    poses, info, cost, twin_info = solve_both(device, cases, 1, len(cases), T.K32, np.ones((1, len(cases)), np.int32))
    compare_info(info, twin_info, "n = %d" % n)
    assert (info[:, 0] == 0).all() and (info[:, 2] == n).all()
    T.assert_within_gates(poses, ref.poses, ref, "device against pnp.pnp, n = %d" % n)


def test_one_call_path_for_the_kernel_and_its_twin(device):
    """twin.call refuses a device tensor for the host twin in Python (nothing is launched, the outputs stay as they were); solve and solve_host
    share one argument list and agree at b = 1, oc = 1, n = 5 (one hypothesis)"""
    import torch

    from casapose_amd import _lib, twin

    cases, ref = T.fixture_set("n5")[:1], T.host_reference("n5")
    xy, x3 = T.batch_of(cases, 1, 1)
    solver = DevicePnP(device, 5)
    d = {k: twin.array(a, t, solver.device) for k, (a, t) in dict(xy=(xy, np.float32), x3=(x3, np.float32), K=(T.K32, np.float32),
                                                                  mask=(np.ones((1, 1), np.int32), np.int32)).items()}
    out = twin.alloc(dict(poses=((1, 1, 3, 4), np.float32), info=((1, 1, 4), np.int32), cost=((1, 1, 2), np.float32)), solver.device, zero=True)
    with pytest.raises(_lib.CasaposeHipError, match=r"cp_pnp_host_f64, argument 0 \(float\*\): a CUDA tensor for a host twin"):
        twin.call("cp_pnp_f64", d["xy"], d["x3"], d["K"], 0, None, d["mask"], solver.table_host, 1, 1, 5, 1, 12.0, out["poses"], out["info"],
                  out["cost"], host=True)
    torch.cuda.synchronize()
    assert not any(bool(v.any()) for v in out.values())
    poses, info, cost, twin_info = solve_both(device, cases, 1, 1, T.K32, np.ones((1, 1), np.int32))
    compare_info(info, twin_info, "n = 5, one pair")
    assert info[0, 0] == 0 and info[0, 1] == 0 and info[0, 2] == 5
    T.assert_within_gates(poses, ref.poses[:1], ref, "device against pnp.pnp, n = 5, one pair")
    host = DevicePnP(None, 5).solve_host(xy, x3, T.K32, np.ones((1, 1), np.int32))
    T.assert_within_gates(host.reshape(1, 3, 4), ref.poses[:1], ref, "twin against pnp.pnp, n = 5, one pair")


@pytest.mark.parametrize("name", ["n10_outliers", "n11_outliers"])
def test_consensus_with_other_point_counts(device, name):
    cases = T.fixture_set(name)
    n = cases[0].points_3d.shape[0]
    poses, info, cost, twin_info = solve_both(device, cases, 1, len(cases), T.K32, np.ones((1, len(cases)), np.int32))
    compare_info(info, twin_info, "n = %d with outliers" % n)
    assert (info[:, 0] == 0).all() and (cost[:, 1] <= cost[:, 0]).all()
    for i, c in enumerate(cases):
        assert n - c.outliers <= info[i, 2] <= n
        assert abs(np.linalg.det(poses[i][:, :3].astype(np.float64)) - 1.0) < 1e-5 and poses[i][2, 3] > 0


def test_two_calls_are_bit_identical(device):
    cases = T.fixture_set("hard")
    xy, x3 = T.batch_of(cases, 3, 5)
    solver = DevicePnP(device, 9)
    first = solver.solve(xy, x3, T.K32, T.PERCAM_MASK).cpu().numpy()
    info, cost = solver.last_info.copy(), solver.last_cost.copy()
    second = solver.solve(xy, x3, T.K32, T.PERCAM_MASK).cpu().numpy()
    assert first.tobytes() == second.tobytes() and info.tobytes() == solver.last_info.tobytes() and cost.tobytes() == solver.last_cost.tobytes()


def test_collapsed_vote_gives_the_zero_pose(device):
    """Nine equal 2-D points in one pair of a batch (a voter can produce this; the twin passes it in tests/test_pnp_twin_host.py): the zero
    pose and status 3 for that pair, the neighbours as without it."""
    cases = T.fixture_set("hard")[:3]
    xy0, x30 = T.batch_of(cases, 1, 3)
    solver = DevicePnP(device, 9)
    full = solver.solve(xy0, x30, T.K32, np.ones((1, 3), np.int32)).cpu().numpy()
    xy, x3 = T.degenerate_batch("equal")
    got = solver.solve(xy, x3, T.K32, np.ones((1, 3), np.int32)).cpu().numpy()
    assert not got[0, 1].any() and solver.last_info[0, 1].tolist() == [3, -1, 0, 0]
    assert np.array_equal(got[0, 0], full[0, 0]) and np.array_equal(got[0, 2], full[0, 2])


def test_estimate_and_evaluate_poses_on_the_device(device):
    """points -> poses -> statistics with DevicePnP and DevicePoseEvaluator against the host chain, on a synthetic batch of 2 images and 3
    objects with noise-free keypoints; object 1 of image 1 is not voted (zero points: a miss).
    Tolerances: the counts and flags are equal.  The poses agree within the gates of the noise-free set.  A pose difference of (gate_R, gate_t)
    moves a camera-frame point of the mesh (radius r) by at most 3 r gate_R + sqrt(3) gate_t =: d mm and its pixel by at most 2 f d / z_min, so the
    batch sums of the mean errors move by at most b times that, plus the fp32 evaluator's own gates (tests/test_gpu_pose_eval.py: 4e-6 S mm,
    2e-6 (f + 640) px per pair)."""
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_estimation import pose_evaluation as E
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    oc, b = 3, 2
    ds = SyntheticSceneDataset(oc, (120, 160), length=2, seed=5, random_crop=False)
    batch = ds.batch(0, b)
    mesh, counts = ds.generate_object_vertex_array()
    h, w = batch["target_seg"].shape[1], batch["target_seg"].shape[2]
    points = batch["target_vert"].numpy()[:, :, 0, :, ::-1].astype(np.float64) / np.array([h, w], np.float64)   # (x, y) / (h, w), as the callers pass them
    points[1, 1] = 0.0
    seg = batch["target_seg"]
    args = (seg, seg, None, batch["poses_gt"], batch["keypoints3d"], batch["cam_mat"], batch["diameters"], batch["offsets"])
    kw = dict(evaluation_points=mesh, object_points_3d_count=counts, points_estimated=points, min_num=20)
    host, host_poses, _ = E.estimate_and_evaluate_poses(*args, **kw)
    solver = DevicePnP(device, 9)
    dev, dev_poses, _ = E.estimate_and_evaluate_poses(*args, solver=solver, evaluator=DevicePoseEvaluator(mesh, counts, device), **kw)
    assert len(dev) == len(host) == 8 and dev_poses.shape == host_poses.shape == (b, oc, 3, 4)
    assert host[6].sum() >= 1 and host[2].sum() >= 4, "the batch must hold a miss and several objects of the ground truth"
    for i in (0, 1, 2, 3, 6, 7):
        assert np.array_equal(np.asarray(dev[i]), np.asarray(host[i])), i
    ref = T.host_reference("clean")
    assert np.array_equal(np.abs(dev_poses).sum(axis=(2, 3)) == 0, np.abs(host_poses).sum(axis=(2, 3)) == 0)
    T.assert_within_gates(dev_poses, host_poses, ref, "device chain against host chain")
    gt = batch["poses_gt"].numpy()[:, :, 0].astype(np.float64)
    cam = np.einsum("boij,ovj->bovi", gt[..., :3], mesh.astype(np.float64)) + gt[:, :, None, :, 3]
    r, S, zmin, f = np.abs(mesh).max() * np.sqrt(3.0), np.abs(cam).max(), cam[..., 2].min(), float(batch["cam_mat"].max())
    d = 3.0 * r * ref.gate_R + np.sqrt(3.0) * ref.gate_t
    tol3, tol2 = b * (d + 4e-6 * S), b * (2.0 * f * d / zmin + 2e-6 * (f + 640.0))
    print("err_2d sums differ by %.3g (tolerance %.3g), err_3d sums by %.3g (tolerance %.3g)" % (
        np.abs(dev[4] - host[4]).max(), tol2, np.abs(dev[5] - host[5]).max(), tol3))
    assert np.abs(dev[4] - host[4]).max() <= tol2 and np.abs(dev[5] - host[5]).max() <= tol3


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import test_pnp_twin_host as T
from casapose_amd.pose_estimation.device_pnp import solver_from_environment
cases = T.fixture_set("hard")
xy, x3 = T.batch_of(cases, 3, 5)
solver = solver_from_environment(9, "cuda:0")
assert solver is not None and solver_from_environment(9, torch.device("cuda:0")) is solver
print("poses " + solver.solve(xy, x3, T.K32, T.PERCAM_MASK).cpu().numpy().tobytes().hex())
"""


def test_environment_switch_in_a_fresh_process(device, monkeypatch):
    """CASAPOSE_DEVICE_PNP=1: solver_from_environment builds the solver once, says `pnp: device`, and its poses are those of a DevicePnP built by
    hand; unset or 0 it returns None."""
    from casapose_amd.pose_estimation.device_pnp import solver_from_environment

    monkeypatch.delenv("CASAPOSE_DEVICE_PNP", raising=False)
    assert solver_from_environment(9, device) is None
    monkeypatch.setenv("CASAPOSE_DEVICE_PNP", "0")
    assert solver_from_environment(9, device) is None
    env = dict(os.environ, CASAPOSE_DEVICE_PNP="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines.count("pnp: device") == 1
    xy, x3 = T.batch_of(T.fixture_set("hard"), 3, 5)
    want = DevicePnP(device, 9).solve(xy, x3, T.K32, T.PERCAM_MASK).cpu().numpy()
    got = [ln for ln in lines if ln.startswith("poses ")]
    assert len(got) == 1 and bytes.fromhex(got[0][6:]) == want.tobytes()
