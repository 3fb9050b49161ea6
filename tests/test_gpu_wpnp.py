"""`cp_pnp_weighted_f64` on the GPU (csrc/pnp_weighted.hip through `DevicePnP.solve(..., cov=)`) against the weighted host path `pnp.pnp(..., cov=)`.
Cases, references and gates are those of tests/test_wpnp_host.py (gates from the weighted host path's own seed-to-seed spread, never from the
device or its twin).  `info` and `weighted` are compared with the host twin's, as tests/test_gpu_pnp.py compares `info`: a +-1 inlier tie
flipped by FMA contraction is allowed and said.  Then the chain from the voter's covariance to the solver on a synthetic scene, and the
CASAPOSE_UNCERTAINTY_PNP switch in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_pnp_twin_host as T
import test_wpnp_host as WH
from casapose_amd.pose_estimation.device_pnp import DevicePnP, affine_from_offsets
from test_gpu_pnp import compare_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def solve_both(device, wcases, b, oc, K, mask, crop):
    """-> (device poses [b*oc,3,4], device solver, twin solver): the same weighted call (floor 0) on the GPU and through the host twin"""
    n = wcases[0].case.points_3d.shape[0]
    xy, x3, cov = WH.wbatch(wcases, b, oc, crop)
    affine = affine_from_offsets(T.PERCAM_OFFSETS[:b]) if crop else None
    dev, twin = DevicePnP(device, n), DevicePnP(None, n)
    poses = dev.solve(xy, x3, K, mask, affine=affine, cov=cov, cov_floor=0.0)
    assert poses.is_cuda and tuple(poses.shape) == (b, oc, 3, 4)
    twin.solve_host(xy, x3, K, mask, affine=affine, cov=cov, cov_floor=0.0)
    compare_info(dev.last_info.reshape(b * oc, 4), twin.last_info.reshape(b * oc, 4), "weighted, b %d oc %d" % (b, oc))
    assert np.array_equal(dev.last_weighted, twin.last_weighted)
    return poses.cpu().numpy().reshape(b * oc, 3, 4), dev, twin


def test_one_block(device):
    """b = 1, oc = 1, n = 9; a case with a 30 px ellipse"""
    ws = WH.wset("shared")[3:4]
    poses, dev, _ = solve_both(device, ws, 1, 1, T.K32, np.ones((1, 1), np.int32), False)
    assert dev.last_info[0, 0, 0] == 0 and dev.last_weighted.tolist() == [[1]] and dev.last_cost[0, 0, 1] <= dev.last_cost[0, 0, 0]
    WH.within_gates(poses, WH.host_runs("shared")[3:4, 0], "device against pnp.pnp(cov=), one block")


def test_batch_shared_camera(device):
    """b = 3, oc = 5, mixed solve flags, K [3,3] shared, image pixels"""
    mask = T.PERCAM_MASK
    on = mask.reshape(15) != 0
    poses, dev, _ = solve_both(device, WH.wset("shared"), 3, 5, T.K32, mask, False)
    assert np.array_equal(dev.last_info.reshape(15, 4)[:, 0], np.where(on, 0, 1)) and not poses[~on].any()
    assert np.array_equal(dev.last_weighted.reshape(15), on.astype(np.int32))
    WH.within_gates(poses[on], WH.host_runs("shared")[on, 0], "device against pnp.pnp(cov=), shared K")


def test_batch_per_image_camera_and_affine(device):
    """b = 3, oc = 5, mixed solve flags, K [b,3,3], crop pixels and crop-pixel covariances with the crop->image affine of every image"""
    mask = T.PERCAM_MASK
    on = mask.reshape(15) != 0
    poses, dev, _ = solve_both(device, WH.wset("percam"), 3, 5, T.PERCAM_K, mask, True)
    assert np.array_equal(dev.last_weighted.reshape(15), on.astype(np.int32)) and not poses[~on].any()
    WH.within_gates(poses[on], WH.host_runs("percam")[on, 0], "device against pnp.pnp(cov=), per-image K and affine")
    cost = dev.last_cost.reshape(15, 2)
    for i in np.flatnonzero(on):
        maha = WH.mahalanobis_cost(WH.wset("percam")[i], poses[i])
        assert abs(cost[i, 1] - maha) <= 1e-3 * maha, (i, cost[i, 1], maha)


@pytest.mark.parametrize("name", ["n5", "n11"])
def test_other_point_counts(device, name):
    ws = WH.wset(name)
    poses, dev, _ = solve_both(device, ws, 1, len(ws), T.K32, np.ones((1, len(ws)), np.int32), False)
    assert (dev.last_info[..., 0] == 0).all() and (dev.last_weighted == 1).all()
    WH.within_gates(poses, WH.host_runs(name)[:, 0], "device against pnp.pnp(cov=), set %s" % name)


def test_two_calls_are_bit_identical(device):
    xy, x3, cov = WH.wbatch(WH.wset("shared"), 3, 5, False)
    solver = DevicePnP(device, 9)
    first = solver.solve(xy, x3, T.K32, T.PERCAM_MASK, cov=cov).cpu().numpy()
    info, cost, weighted = solver.last_info.copy(), solver.last_cost.copy(), solver.last_weighted.copy()
    second = solver.solve(xy, x3, T.K32, T.PERCAM_MASK, cov=cov).cpu().numpy()
    assert first.tobytes() == second.tobytes() and info.tobytes() == solver.last_info.tobytes() and cost.tobytes() == solver.last_cost.tobytes()
    assert weighted.tobytes() == solver.last_weighted.tobytes()


def test_an_unusable_covariance_falls_back_alone(device):
    """one pair with a singular covariance and one with a NaN among usable ones: those two are cp_pnp_f64's, bit for bit; the others are weighted"""
    xy, x3, cov = WH.wbatch(WH.wset("shared")[:5], 1, 5, False)
    ones = np.ones((1, 5), np.int32)
    solver = DevicePnP(device, 9)
    full = solver.solve(xy, x3, T.K32, ones, cov=cov, cov_floor=0.0).cpu().numpy()
    plain = solver.solve(xy, x3, T.K32, ones).cpu().numpy()
    assert solver.last_weighted is None
    plain_info, plain_cost = solver.last_info.copy(), solver.last_cost.copy()
    bad = cov.copy()
    bad[0, 1, 4] = (1.0, 2.0, 4.0)
    bad[0, 3, 0] = (1.0, np.nan, 1.0)
    got = solver.solve(xy, x3, T.K32, ones, cov=torch.from_numpy(bad).to(device), cov_floor=0.0).cpu().numpy()       # a device tensor is used where it lies
    assert solver.last_weighted.tolist() == [[1, 0, 1, 0, 1]]
    for i in (1, 3):
        assert got[0, i].tobytes() == plain[0, i].tobytes() and solver.last_info[0, i].tobytes() == plain_info[0, i].tobytes()
        assert solver.last_cost[0, i].tobytes() == plain_cost[0, i].tobytes() and not np.array_equal(full[0, i], plain[0, i])
    for i in (0, 2, 4):
        assert got[0, i].tobytes() == full[0, i].tobytes()
    zero = solver.solve(xy, x3, T.K32, ones, cov=np.zeros_like(cov)).cpu().numpy()       # rescued by the default floor
    assert (solver.last_weighted == 1).all()
    WH.within_gates(zero[0], plain[0], "isotropic floor against the unweighted solve")


# ---- the chain: voter -> covariance -> solver, everything on the device ------------------------------------------------------------------------------
def scene(device):
    """A synthetic batch of 2 images and 3 objects (120 x 160) with a vector field pointing at the projected keypoints, turned by N(0, 0.03) rad;
    object 1 of image 1 is removed from the estimated segmentation (not voted)."""
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

    ds = SyntheticSceneDataset(3, (120, 160), length=2, seed=5, random_crop=False)
    batch = ds.batch(0, 2)
    seg = batch["target_seg"].cpu().numpy().astype(np.float32)
    b, h, w, k = seg.shape
    kp_yx = batch["target_vert"].numpy()[:, :, 0].astype(np.float64)       # [b,oc,kp,2]
    lab = seg.argmax(-1)
    rng = np.random.default_rng(9)
    ys, xs = np.mgrid[0:h, 0:w] + 0.5
    field = np.zeros((b, h, w, 9, 2), np.float32)
    for bi in range(b):
        for o in range(k - 1):
            m = lab[bi] == o + 1
            ang = np.arctan2(kp_yx[bi, o, None, :, 0] - ys[m][:, None], kp_yx[bi, o, None, :, 1] - xs[m][:, None]) + rng.normal(0, 0.03, (int(m.sum()), 9))
            field[bi][m] = np.stack([np.sin(ang), np.cos(ang)], -1)       # (dy, dx)
    est = seg.copy()
    gone = lab[1] == 2
    est[1][gone] = np.eye(k, dtype=np.float32)[0]
    return batch, torch.from_numpy(est).to(device), torch.from_numpy(field.reshape(b, h, w, 18)).to(device)


def chain(device, solver):
    from casapose_amd.pose_estimation import pose_evaluation as E

    batch, est, field = scene(device)
    torch.manual_seed(21)       # the voter's and the covariance's seeds come from the default CPU generator
    stats, poses, pts = E.estimate_and_evaluate_poses(est, batch["target_seg"], field, batch["poses_gt"], batch["keypoints3d"], batch["cam_mat"],
                                                      batch["diameters"], batch["offsets"], min_num=20, solver=solver)
    voted = np.abs(pts.cpu().numpy()).sum(axis=(2, 3)) >= 0.01
    return np.asarray(poses), voted, batch


def test_the_chain_from_the_voter_to_the_weighted_solve(device, monkeypatch):
    solver = DevicePnP(device, 9)
    monkeypatch.delenv("CASAPOSE_UNCERTAINTY_PNP", raising=False)
    plain, voted, batch = chain(device, solver)
    assert solver.last_weighted is None       # with the switch unset no new code runs
    monkeypatch.setenv("CASAPOSE_UNCERTAINTY_PNP", "1")
    poses, voted2, _ = chain(device, solver)
    assert np.array_equal(voted, voted2) and voted.sum() == 5 and not voted[1, 1]
    assert np.array_equal(solver.last_weighted, voted.astype(np.int32)) and np.array_equal(solver.last_info[..., 0], np.where(voted, 0, 1))
    assert np.isfinite(poses).all() and (np.abs(poses[voted]).sum(axis=(1, 2)) > 0).all() and not poses[~voted].any()
    assert (poses[voted][:, 2, 3] > 0).all()
    assert not np.array_equal(poses[voted], plain[voted])
    # the host PnP takes the same covariance
    from casapose_amd.pose_estimation import pose_evaluation as E
    from casapose_amd.pose_estimation.ransac_voting import ransac_voting_layer_all_masks

    _, est, field = scene(device)
    onehot = torch.nn.functional.one_hot(torch.argmax(est, dim=3), est.shape[3])[..., 1:].to(torch.float32)
    pts, cov, = ransac_voting_layer_all_masks(onehot, field.reshape(2, 120, 160, 9, 2), 512, min_num=20, generator=torch.Generator().manual_seed(4),
                                              return_covariance=True)
    avail = np.ones((2, 3), np.int32)
    host, _ = E.estimate_poses(pts, batch["keypoints3d"], batch["cam_mat"], avail, batch["offsets"], rng=np.random.default_rng(0), cov=cov)
    dev, _ = E.estimate_poses(pts, batch["keypoints3d"], batch["cam_mat"], avail, batch["offsets"], solver=solver, cov=cov)
    assert np.array_equal(solver.last_weighted, voted.astype(np.int32))
    WH.within_gates(dev[voted], host[voted], "estimate_poses(cov=): device solver against the host PnP")


@pytest.mark.parametrize("filtered", [False, True])
def test_the_ls_voter_keeps_its_labels_and_its_covariance_reaches_either_pnp(device, filtered):
    """What training.test_step does under the switch: the covariance about the LS-voted keypoints over `voter.last_labels` -- the arg-max map, or
    with filter_estimates the component-filtered map, in which a 30-pixel speck added to object 0 no longer votes -- to poses_from_coords."""
    from casapose_amd import ops
    from casapose_amd.pose_estimation.keypoint_covariance import keypoint_covariance
    from casapose_amd.pose_estimation.voting_layers_2d import CoordLSVotingWeighted
    from casapose_amd.training import poses_from_coords

    batch, est, field = scene(device)
    est = est.clone()
    est[0, 2:7, 2:8] = torch.eye(4, device=device)[1]       # a speck of object 0 in a background corner, without directions
    seg = 10.0 * est
    voter = CoordLSVotingWeighted(name="coords_ls_voting", num_classes=4, num_points=9, filter_estimates=filtered)
    assert voter.last_labels is None
    coords = voter([seg, field, torch.zeros(2, 120, 160, 9, device=device)])
    lab = voter.last_labels
    argmax = ops.argmax_labels(seg.contiguous(), classes=4)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (2, 120, 160) and voter.last_labels is lab
    if filtered:
        assert not lab[0, 2:7, 2:8].any() and torch.equal(lab[1], argmax[1]) and int((lab != argmax).sum()) == 30
    else:
        assert torch.equal(lab, argmax)
    cov, wsum = keypoint_covariance(lab, field, coords.flip(-1), generator=torch.Generator().manual_seed(2), return_weight_sum=True)
    voted = np.array([[1, 1, 1], [1, 0, 1]], bool)
    assert np.array_equal(wsum.cpu().numpy().min(axis=2) > 0, voted) and not cov.cpu().numpy()[~voted].any()
    avail = torch.from_numpy(voted.astype(np.float32))
    solver = DevicePnP(device, 9)
    dev, _ = poses_from_coords(coords, avail, batch, solver=solver, cov=cov)
    assert np.array_equal(solver.last_weighted, voted.astype(np.int32))
    host, _ = poses_from_coords(coords, avail, batch, rng=np.random.default_rng(0), cov=cov)
    WH.within_gates(dev[:, :, 0][voted], host[:, :, 0][voted], "poses_from_coords(cov=): device solver against the host PnP")
    assert np.isfinite(dev).all() and (dev[:, :, 0][voted][:, 2, 3] > 0).all() and not dev[:, :, 0][~voted].any()


def test_the_inference_script_chain_under_the_switch(device, monkeypatch):
    """util_scripts/test_minimal.py's three lines -- voter([seg, dirs, conf]), then poses_pnp(coords, seg, keypoints, camera_matrix, K - 1) --
    under CASAPOSE_UNCERTAINTY_PNP=1: poses_pnp is given no covariance and no field, finds the voter that returned `coords`, and votes the
    covariance over that voter's labels and field.  The poses are those of the same call with the covariance passed by hand; a copy of the
    keypoints, which no voter returned, is refused by name; with the switch unset the voter keeps nothing and the call is the unweighted one."""
    from casapose_amd.pose_estimation import voting_layers_2d as V
    from casapose_amd.pose_estimation.keypoint_covariance import keypoint_covariance
    from casapose_amd.pose_estimation.pose_evaluation import poses_pnp

    batch, est, field = scene(device)
    seg, conf = 10.0 * est, torch.zeros(2, 120, 160, 9, device=device)
    kp3, cam = batch["keypoints3d"], batch["cam_mat"]
    solver = DevicePnP(device, 9)
    voted = np.array([[1, 1, 1], [1, 0, 1]], np.int32)

    monkeypatch.delenv("CASAPOSE_UNCERTAINTY_PNP", raising=False)
    voter = V.CoordLSVotingWeighted(name="coords_ls_voting", num_classes=4, num_points=9, filter_estimates=True)
    coords = voter([seg, field, conf])
    assert V.voter_of(coords) is None and voter.last_field is None
    plain = poses_pnp(coords, seg, kp3, cam, 3, min_num=20, solver=solver)
    assert solver.last_weighted is None

    monkeypatch.setenv("CASAPOSE_UNCERTAINTY_PNP", "1")
    coords = voter([seg, field, conf])
    assert V.voter_of(coords) is voter and V.voter_of(coords.clone()) is None
    torch.manual_seed(31)       # the covariance's seed comes from the default CPU generator
    got = poses_pnp(coords, seg, kp3, cam, 3, min_num=20, solver=solver)
    assert np.array_equal(solver.last_weighted, voted)
    torch.manual_seed(31)
    cov = keypoint_covariance(voter.last_labels, field, coords.flip(-1))
    want = poses_pnp(coords, seg, kp3, cam, 3, min_num=20, solver=solver, cov=cov)
    assert got.tobytes() == want.tobytes() and got.shape == (2, 3, 1, 3, 4) and not np.array_equal(got, plain)
    assert np.isfinite(got).all() and (got[:, :, 0][voted != 0][:, 2, 3] > 0).all() and not got[:, :, 0][voted == 0].any()
    torch.manual_seed(31)
    host = poses_pnp(coords, seg, kp3, cam, 3, min_num=20, rng=np.random.default_rng(0))       # the host PnP, the covariance voted the same way
    WH.within_gates(got[:, :, 0][voted != 0], host[:, :, 0][voted != 0], "poses_pnp under the switch: device solver against the host PnP")
    with pytest.raises(ValueError, match="poses_pnp: CASAPOSE_UNCERTAINTY_PNP=1 needs cov="):
        poses_pnp(coords.clone(), seg, kp3, cam, 3, min_num=20, solver=solver)


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import test_gpu_wpnp as G
from casapose_amd.pose_estimation.device_pnp import solver_from_environment
solver = solver_from_environment(9, "cuda:0")
poses, voted, _ = G.chain(torch.device("cuda:0"), solver)
poses, voted, _ = G.chain(torch.device("cuda:0"), solver)
print("weighted " + "".join(str(int(v)) for v in solver.last_weighted.reshape(-1)))
print("poses " + poses.astype(np.float32).tobytes().hex())
"""


def test_environment_switch_in_a_fresh_process(device, monkeypatch):
    """CASAPOSE_UNCERTAINTY_PNP=1 beside CASAPOSE_DEVICE_PNP=1, read in a child process: `pnp: uncertainty-weighted` is said once for two
    calls, and the poses are those of the chain run here by hand."""
    env = dict(os.environ, CASAPOSE_DEVICE_PNP="1", CASAPOSE_UNCERTAINTY_PNP="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines.count("pnp: uncertainty-weighted") == 1 and lines.count("pnp: device") == 1
    monkeypatch.setenv("CASAPOSE_UNCERTAINTY_PNP", "1")
    solver = DevicePnP(device, 9)
    want, voted, _ = chain(device, solver)
    got = [ln for ln in lines if ln.startswith("poses ")]
    assert len(got) == 1 and bytes.fromhex(got[0][6:]) == want.astype(np.float32).tobytes()
    assert [ln for ln in lines if ln.startswith("weighted ")] == ["weighted " + "".join(str(int(v)) for v in voted.reshape(-1))]
