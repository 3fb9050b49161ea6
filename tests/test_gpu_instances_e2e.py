"""Several instances of one object, end to end on a planted scene: 2 x 96 x 136, the production record with 8 objects of which two are present,
object 2 with three and object 7 with two instances in image 0 (one each in image 1), every instance a disc of its own size around the
projection of its object's origin, the vector field pointing exactly at the instance's projected keypoints.  One further disc of object 7 is
smaller than min_component, and R = 4 leaves slots empty.

First on the CPU: the fp64 restatement (tests/ls_reference.py voting over the slot map of tests/instance_reference.py) returns the planted
keypoints within 0.05 px, the project's voter gate, so the input itself is inside the gate.  Then on the GPU: InstanceLSVoting returns them within
the same gate and counts the discs, and poses_pnp_instances recovers every planted pose through the host PnP and through DevicePnP.  The pose
tolerances are the gates tests/test_gpu_pnp.py applies to its nine-point sets (T.host_reference("hard"): ten times the host path's own
seed-to-seed spread plus eight fp32 ulps: 4.5e-6 in R, 1.0e-3 mm in t), with that file's camera and distances (K32, 600 - 700 mm).

The object size is chosen for those gates, by this reasoning: the voter forms n = d / |d| in fp32, so |n| is off by e ~ 1e-7, which adds
-2 e w n n^T to a pixel's R = w (I - n n^T) and pulls a keypoint at distance D along the ray by e D per pixel; across a disc of radius r the
other pixels hold against that only with (r / D)^2 of their weight, so the keypoint moves by about e D (D / r)^2, and t_z by z / D times that.
With t_z's gate of 1e-3 mm at z = 650 mm and r = 9 px this asks for D^2 <= 1e-3 r^2 / (z e) = 1 250 px^2, D <= 35 px: keypoints within +-20 mm
(D <= 31 px at f = 572, z = 600) are inside it, the +-60 mm of the PnP fixtures (D up to 100 px) are not -- they would test the conditioning
of voting from a 20-pixel disc to a point 100 pixels away, not the instance path."""
import functools

import numpy as np
import pytest
import torch

import instance_reference as IR
import ls_reference as L
import test_pnp_twin_host as T
from casapose_amd.pose_estimation import pnp as P

B, H, W, OBJECTS, R, KP = 2, 96, 136, 8, 4, 9
MIN_COMPONENT = 50
VOTER_GATE = 0.05
CAM = np.array([[572.4114, 0.0, 68.0], [0.0, 573.57043, 48.0], [0.0, 0.0, 1.0]], np.float32)      # K32 with the principal point of the small image
# (image, object (1-based), disc centre (y, x), radius): per object the radii, hence the sizes, are distinct
PLANTED = [(0, 2, (22.0, 24.0), 12.0), (0, 2, (22.0, 66.0), 10.5), (0, 2, (24.0, 110.0), 9.0), (0, 7, (70.0, 30.0), 11.0), (0, 7, (68.0, 80.0), 8.5),
           (1, 2, (48.0, 40.0), 10.0), (1, 7, (48.0, 100.0), 9.5)]
SMALL = (0, 7, (76.0, 120.0), 3.0)


@functools.lru_cache(maxsize=None)
def scene():
    """-> (record float32 [B,H,W,36], labels, instances): instances [(image, object, rank, size, pose [3,4], keypoints (y, x) [9,2])] with rank
    the position of the disc among its object's in the image by size, descending"""
    rng = np.random.default_rng(31)
    X = rng.uniform(-20.0, 20.0, (OBJECTS, KP, 3))
    X[:, 0] = 0.0
    X = X.astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    labels = np.zeros((B, H, W), np.uint8)
    rec = np.zeros((B, H, W, 36), np.float32)
    Kd = CAM.astype(np.float64)
    found = []
    for n, o, (cy, cx), rad in PLANTED + [SMALL]:
        axis = rng.normal(size=3)
        Rm = P.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.2, 2.8))
        z = rng.uniform(600.0, 700.0)
        t = z * np.linalg.solve(Kd, np.array([cx, cy, 1.0]))                 # the object's origin (keypoint 0) projects to the disc's centre
        xy = P.project(X[o - 1].astype(np.float64), Kd, Rm, t)
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
        assert not labels[n][disc].any()
        labels[n][disc] = o
        rec[n][disc, 9:27] = (xy[:, ::-1][None] - np.stack([yy[disc], xx[disc]], -1)[:, None]).reshape(-1, 18).astype(np.float32)
        found.append([n, o, int(disc.sum()), np.concatenate([Rm, t[:, None]], axis=1), xy[:, ::-1]])
    rec[..., :9] = 10.0 * np.eye(9, dtype=np.float32)[labels]
    small = found.pop()
    assert small[2] < MIN_COMPONENT and all(f[2] >= 200 for f in found)
    instances = []
    for n in range(B):
        for o in (2, 7):
            mine = sorted((f for f in found if f[0] == n and f[1] == o), key=lambda f: -f[2])
            assert len({f[2] for f in mine}) == len(mine) < R
            instances += [(n, o, r, f[2], f[3], f[4]) for r, f in enumerate(mine)]
    return rec, labels, X, instances


def planted_tables():
    _, _, _, instances = scene()
    counts = np.zeros((B, OBJECTS, R), np.int32)
    kps = np.zeros((B, OBJECTS, R, KP, 2))
    poses = np.zeros((B, OBJECTS, R, 3, 4))
    for n, o, r, size, pose, yx in instances:
        counts[n, o - 1, r], kps[n, o - 1, r], poses[n, o - 1, r] = size, yx, pose
    return counts, kps, poses


def test_the_planted_scene_is_inside_the_voter_gate_in_fp64():
    rec, labels, _, instances = scene()
    counts, kps, _ = planted_tables()
    slots, inst = IR.instance_labels(labels, OBJECTS, R, MIN_COMPONENT)
    assert np.array_equal(inst[..., 0], counts) and len(instances) == 7 == int((counts > 0).sum())
    t32, _ = L.terms(rec, 36, 9, 27, 0, H)
    s, _ = L.sums(t32, slots, OBJECTS * R)
    got = L.solve(s, H).reshape(B, OBJECTS, R, KP, 2)
    on = counts > 0
    err = np.abs(got[on] - kps[on]).max()
    print("fp64 restatement against the planted keypoints: %.3g px" % err)
    assert err <= VOTER_GATE and not got[~on].any()


@pytest.fixture(scope="module")
def voted(device):
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    rec, _, _, _ = scene()
    out = torch.from_numpy(rec).to(device)
    seg, dirs, conf = torch.split(out, [9, 18, 9], dim=3)
    voter = InstanceLSVoting("instances", num_classes=OBJECTS + 1, num_points=KP, max_instances=R, min_component=MIN_COMPONENT)
    coords = voter([seg, dirs, conf])
    return voter, coords


@pytest.mark.gpu
def test_keypoints_and_counts(voted):
    voter, coords = voted
    counts, kps, _ = planted_tables()
    assert tuple(coords.shape) == (B, OBJECTS, R, KP, 2) and coords.dtype == torch.float32
    assert voter.last_counts.dtype == torch.int32 and voter.last_counts.is_cuda and np.array_equal(voter.last_counts.cpu().numpy(), counts)
    got, on = coords.cpu().numpy().astype(np.float64), counts > 0
    err = np.abs(got[on] - kps[on]).max()
    print("device keypoints against the planted ones: %.3g px" % err)
    assert err <= VOTER_GATE and not got[~on].any()
    slots, _ = IR.instance_labels(scene()[1], OBJECTS, R, MIN_COMPONENT)
    assert np.array_equal(voter.last_labels.cpu().numpy(), slots) and voter.slot_of(7, 1) == 26 and slots.max() == 26
    with pytest.raises(ValueError):
        voter.slot_of(9, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_planted_poses_are_recovered(voted, device, path):
    from casapose_amd.pose_estimation.device_pnp import DevicePnP
    from casapose_amd.pose_estimation.instance_voting import poses_pnp_instances

    voter, coords = voted
    counts, _, poses = planted_tables()
    X = scene()[2]
    solver = DevicePnP(device, KP) if path == "device" else None
    got = poses_pnp_instances(coords, voter.last_counts, X[None, :, None], CAM, rng=np.random.default_rng(0), solver=solver)
    assert got.shape == (B, OBJECTS, R, 3, 4) and got.dtype == np.float32
    on = counts > 0
    assert not got[~on].any()            # the disc below min_component, the missing instances and the absent objects
    T.assert_within_gates(got[on], poses[on], T.host_reference("hard"), "poses_pnp_instances (%s PnP) against the planted poses" % path)
    assert (got[on][:, 2, 3] > 0).all()
