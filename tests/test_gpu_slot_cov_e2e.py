"""InstanceLSVoting(covariance=True) and poses_pnp_instances(cov=) end to end on the two touching scenes of tests/test_gpu_vote_split_e2e.py
(48 x 64 and 60 x 80, split="votes", 8 objects x 4 instances), with the plain and with the robust voter:
  - last_cov / last_cov_stat are what ops.ls_slot_covariance gives for the voter's own slot map and keypoints (the cut-off the robust voter's,
    none for the plain one); the order of the atomics is free, so the comparison is to 1e-5 of the largest entry, the NaN pattern exact;
  - the keypoints of either voter are bit for bit the keypoints of the same voter with covariance=False;
  - DevicePnP is handed the covariances through poses_pnp_instances without a host copy and reports weighted == 1 exactly where the slot is
    solved and every one of its keypoints has a covariance;
  - the poses are those of the host twin cp_pnp_weighted_host_f64 on the same inputs: `info` compared as tests/test_gpu_wpnp.py compares it,
    `weighted` equal, the poses to 1e-5 (rotation entries; translation relative to its length) -- both run the same LM to a relative cost
    change of 1e-10, which fixes the minimum to about its square root;
  - the host loop (no solver) weights the same slots."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_vote_split_e2e as E
from test_gpu_pnp import compare_info

KP = 9
VOTERS = {"ls": dict(), "robust": dict(voter="robust", cutoff=4.0, passes=2)}
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voted(device):
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    def run(name, voter, covariance):
        out = torch.from_numpy(E.scene(name)[0]).to(device)
        seg, dirs, conf = torch.split(out, [9, 18, 9], dim=3)
        P = E.PARAMS
        v = InstanceLSVoting("instances", num_classes=E.OBJECTS + 1, num_points=KP, max_instances=E.R, min_component=P["min_size"], split="votes",
                             cell=P["cell"], vote_stride=E.STRIDE, min_votes=P["min_votes"], rel_percent=P["rel_percent"], nms_radius=P["nms_radius"],
                             gate=P["gate"], covariance=covariance, **VOTERS[voter])
        return v, v([seg, dirs, conf]), out
    return functools.lru_cache(maxsize=None)(run)


@pytest.mark.parametrize("voter", list(VOTERS))
@pytest.mark.parametrize("name", E.NAMES)
def test_the_voter_hands_out_the_ops_covariance_and_keeps_its_keypoints(voted, name, voter):
    from casapose_amd import ops

    v, coords, rec = voted(name, voter, True)
    plain, plain_coords, _ = voted(name, voter, False)
    assert plain.last_cov is None and plain.last_cov_stat is None
    assert torch.equal(coords.view(torch.int32), plain_coords.view(torch.int32))             # bit for bit
    assert torch.equal(v.last_labels, plain.last_labels)
    cov, stat = v.last_cov, v.last_cov_stat
    assert cov.is_cuda and cov.dtype == torch.float32 and tuple(cov.shape) == (1, E.OBJECTS, E.R, KP, 3) and tuple(stat.shape) == (1, E.OBJECTS, E.R, KP, 2)
    c2, s2 = ops.ls_slot_covariance(rec, 9, 27, E.OBJECTS * E.R, KP, v.last_labels, coords.reshape(1, E.OBJECTS * E.R, KP, 2).contiguous(),
                                    cutoff=4.0 if voter == "robust" else None)
    a, b = cov.cpu().numpy().reshape(-1, 3), c2.cpu().numpy().reshape(-1, 3)
    fin = np.isfinite(a).all(-1)
    assert np.array_equal(fin, np.isfinite(b).all(-1)) and np.array_equal(np.isnan(a).all(-1), ~fin)
    assert np.abs(a[fin] - b[fin]).max() <= 1e-5 * np.abs(b[fin]).max()
    assert np.abs(stat.cpu().numpy() - s2.cpu().numpy().reshape(stat.shape)).max() <= 1e-5 * float(s2.max())
    on = (v.last_counts > 0).cpu().numpy()
    assert on.sum() == len(E.scene(name)[5]) and fin.reshape(1, E.OBJECTS, E.R, KP)[on].all() and not fin.reshape(1, E.OBJECTS, E.R, KP)[~on].any()
    st = stat.cpu().numpy()
    print("%s %s: sigma2 %.3g .. %.3g px^2, kept %.4f .. %.4f, largest variance %.3g px^2" % (name, voter, st[on][..., 0].min(), st[on][..., 0].max(),
                                                                                             st[on][..., 1].min(), st[on][..., 1].max(), a[fin][:, [0, 2]].max()))
    assert (st[on][..., 1] <= 1.0).all() and ((st[on][..., 1] == 1.0).all() if voter == "ls" else (st[on][..., 1] < 1.0).any())


@pytest.mark.parametrize("voter", list(VOTERS))
@pytest.mark.parametrize("name", E.NAMES)
def test_the_device_pnp_is_weighted_where_a_slot_has_all_its_covariances_and_equals_the_twin(voted, device, name, voter):
    from casapose_amd.pose_estimation.device_pnp import DevicePnP
    from casapose_amd.pose_estimation.instance_voting import poses_pnp_instances

    v, coords, _ = voted(name, voter, True)
    _, _, _, X, cam, planted = E.scene(name)
    cov = v.last_cov.clone()
    # take one keypoint's covariance away from one found instance: that slot must fall back alone
    found = np.argwhere(v.last_counts.cpu().numpy() > 20)
    n0, o0, r0 = (int(i) for i in found[-1])
    cov[n0, o0, r0, 3] = float("nan")
    solver = DevicePnP(device, KP)
    poses, weighted = poses_pnp_instances(coords, v.last_counts, X[None, :, None], cam, rng=np.random.default_rng(0), solver=solver, cov=cov,
                                          return_weighted=True)
    assert poses.shape == (1, E.OBJECTS, E.R, 3, 4) and weighted.shape == (1, E.OBJECTS, E.R) and weighted.dtype == np.int32
    solved = v.last_counts.cpu().numpy() > 20
    want = solved & np.isfinite(cov.cpu().numpy()).all((-1, -2))
    assert np.array_equal(weighted, want.astype(np.int32)) and weighted.sum() == len(planted) - 1 and weighted[n0, o0, r0] == 0
    # the twin on the same inputs
    b, oc, R = 1, E.OBJECTS, E.R
    xy = np.ascontiguousarray(coords.cpu().numpy()[..., ::-1].reshape(b, oc * R, KP, 2))
    x3 = np.ascontiguousarray(np.repeat(np.broadcast_to(X[None], (b, oc, KP, 3)), R, axis=1))
    twin = DevicePnP(None, KP)
    tposes = twin.solve_host(xy, x3, cam, np.ascontiguousarray(solved.reshape(b, oc * R).astype(np.int32)), cov=cov.cpu().numpy().reshape(b, oc * R, KP, 3))
    compare_info(solver.last_info.reshape(oc * R, 4), twin.last_info.reshape(oc * R, 4), "%s %s" % (name, voter))
    assert np.array_equal(np.asarray(solver.last_weighted), np.asarray(twin.last_weighted))
    tposes = np.asarray(tposes, np.float64).reshape(1, oc, R, 3, 4)
    d_r = np.abs(poses[..., :3] - tposes[..., :3]).max()
    d_t = (np.linalg.norm(poses[..., 3] - tposes[..., 3], axis=-1) / np.maximum(np.linalg.norm(tposes[..., 3], axis=-1), 1.0)).max()
    print("%s %s: device against the twin: rotation entries %.3g, translation %.3g of its length" % (name, voter, d_r, d_t))
    assert d_r <= 1e-5 and d_t <= 1e-5 and not poses[~solved].any()
    # the host loop weights the same slots
    _, hw = poses_pnp_instances(coords.cpu().numpy(), v.last_counts.cpu().numpy(), X[None, :, None], cam, rng=np.random.default_rng(0), cov=cov.cpu().numpy(),
                                return_weighted=True)
    assert np.array_equal(hw, weighted)
    # and without cov nothing is weighted and the result is the call's of before
    p0 = poses_pnp_instances(coords, v.last_counts, X[None, :, None], cam, rng=np.random.default_rng(0), solver=solver)
    p1, w1 = poses_pnp_instances(coords, v.last_counts, X[None, :, None], cam, rng=np.random.default_rng(0), solver=solver, return_weighted=True)
    assert np.array_equal(p0, p1) and not w1.any() and solver.last_weighted is None
