"""CASAPOSE_INSTANCE_PNP and util_scripts/minimal_instances.py: how the variable is read and what it refuses, that InstanceLSVoting takes
`covariance` and with False makes the calls it made before, that poses_pnp_instances hands `cov` on (to a solver as [b, oc*R, kp, 3], to the
host PnP with the floor and the fall-back), and -- shown without a GPU, with the stand-ins of tests/test_robust_vote_scripts.py for the
dataset, the network, the voter and the PnP -- that with the switch unset or `plain` the script builds the voter it built before, prints what
it printed and writes the CSV it wrote, for both splits and both voters, and under `weighted` says so once and adds the column `weighted` after
whatever columns are there.  No GPU."""
import csv
import os

import numpy as np
import pytest
import torch

from test_instances_scripts import CFG, NAMES, Annotated, Frames, Net
from test_robust_vote_scripts import script  # noqa: F401  (the fixture)
from test_vote_split_scripts import OLD_HEADER

SWITCHES = ("CASAPOSE_MAX_INSTANCES", "CASAPOSE_INSTANCE_SPLIT", "CASAPOSE_INSTANCE_VOTER", "CASAPOSE_INSTANCE_PNP", "CASAPOSE_UNCERTAINTY_PNP",
            "CASAPOSE_MASK_REFINE", "CASAPOSE_DEVICE_PNP")
LINE = "instances: covariance-weighted PnP"


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def test_the_switch_is_parsed_as_specified(monkeypatch):
    from casapose_amd.pose_estimation.instance_voting import instance_pnp_from_environment as read

    assert read() == "plain"
    monkeypatch.setenv("CASAPOSE_INSTANCE_PNP", "plain")
    assert read() == "plain"                               # without CASAPOSE_MAX_INSTANCES too: it is the existing path
    for raw in ("Weighted", "WEIGHTED", "", "1", "cov", "uncertainty"):
        monkeypatch.setenv("CASAPOSE_INSTANCE_PNP", raw)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_PNP must be unset, `plain` or `weighted`"):
            read()
    monkeypatch.setenv("CASAPOSE_INSTANCE_PNP", "weighted")
    for instances in (None, "1"):                       # one instance per object: the switch belongs to the instance path
        monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False) if instances is None else monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", instances)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_PNP=weighted .*CASAPOSE_MAX_INSTANCES"):
            read()
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "4")
    assert read() == "weighted"
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "40")      # the other variable's own refusal comes through
    with pytest.raises(ValueError, match="CASAPOSE_MAX_INSTANCES must be"):
        read()


def test_the_voter_calls_the_op_with_its_own_keypoints_and_otherwise_calls_what_it_called(monkeypatch):
    from casapose_amd import ops
    from casapose_amd.pose_estimation import instance_voting as IV

    calls = []

    class Cuda(torch.Tensor):
        is_cuda = True

    def plain(rec, do, co, slots, kp, slot_map, sigmoid_weights=False):
        calls.append(("ls", do, co, slots, kp, sigmoid_weights))
        return torch.full((rec.shape[0], slots, kp, 2), 3.0)

    def robust(rec, do, co, slots, kp, slot_map, cutoff, passes, sigmoid_weights, return_sums):
        calls.append(("robust", do, co, slots, kp, cutoff, passes, sigmoid_weights, return_sums))
        sums = torch.ones(rec.shape[0], slots, kp, 5, dtype=torch.float64)
        return torch.full((rec.shape[0], slots, kp, 2), 5.0), sums, 0.5 * sums

    def covariance(rec, do, co, slots, kp, slot_map, keypoints, cutoff=None, sigmoid_weights=False, return_sums=False):
        calls.append(("cov", do, co, slots, kp, float(keypoints.reshape(-1)[0]), tuple(keypoints.shape), cutoff, sigmoid_weights, return_sums))
        return torch.full((rec.shape[0], slots, kp, 3), 2.0), torch.full((rec.shape[0], slots, kp, 2), 0.5)

    monkeypatch.setattr(ops, "argmax_labels", lambda rec, classes, offset: torch.zeros(rec.shape[:3], dtype=torch.uint8))
    monkeypatch.setattr(ops, "ccl_instance_labels", lambda lab0, objects, R, min_size: (lab0, torch.zeros(lab0.shape[0], objects, R, 2, dtype=torch.int32)))
    monkeypatch.setattr(ops, "ls_vote_slots", plain)
    monkeypatch.setattr(ops, "ls_vote_slots_robust", robust)
    monkeypatch.setattr(ops, "ls_slot_covariance", covariance)
    rec = torch.zeros(1, 4, 8, 36).as_subclass(Cuda)
    inp = [rec[..., :9], rec[..., 9:27], rec[..., 27:]]
    monkeypatch.setattr(IV, "_as_record", lambda seg, direct, conf: (rec, (1, 9, 27)))
    for kw in (dict(), dict(covariance=False)):
        v = IV.InstanceLSVoting("v", 9, max_instances=2, **kw)
        assert tuple(v(inp).shape) == (1, 8, 2, 9, 2) and calls == [("ls", 9, 27, 16, 9, False)] and v.last_cov is None and v.last_cov_stat is None
        del calls[:]
        v = IV.InstanceLSVoting("v", 9, max_instances=2, voter="robust", cutoff=3.0, passes=1, sigmoid_weights=True, **kw)
        v(inp)
        assert calls == [("robust", 9, 27, 16, 9, 3.0, 1, True, True)] and v.last_cov is None
        del calls[:]
    v = IV.InstanceLSVoting("v", 9, max_instances=2, covariance=True)
    v(inp)
    assert calls == [("ls", 9, 27, 16, 9, False), ("cov", 9, 27, 16, 9, 3.0, (1, 16, 9, 2), None, False, False)]      # the plain voter: no cut-off
    assert tuple(v.last_cov.shape) == (1, 8, 2, 9, 3) and tuple(v.last_cov_stat.shape) == (1, 8, 2, 9, 2) and bool((v.last_cov == 2.0).all())
    del calls[:]
    v = IV.InstanceLSVoting("v", 9, max_instances=2, voter="robust", cutoff=3.0, passes=1, sigmoid_weights=True, covariance=True)
    v(inp)
    assert calls[1] == ("cov", 9, 27, 16, 9, 5.0, (1, 16, 9, 2), 3.0, True, False)                                   # the robust voter's cut-off
    del calls[:]
    v = IV.InstanceLSVoting("v", 9, max_instances=2, voter="robust", cutoff=3.0, passes=0, covariance=True)
    v(inp)
    assert calls[1][7] is None                                                                                    # no reweighted pass: no cut-off


def test_poses_pnp_instances_hands_the_covariances_on(monkeypatch):
    from casapose_amd.pose_estimation import instance_voting as IV
    from casapose_amd.pose_estimation import pnp as P

    b, oc, R, kp = 1, 2, 2, 9
    rng = np.random.default_rng(1)
    X = rng.uniform(-0.05, 0.05, (oc, kp, 3))
    K = np.array([[300.0, 0.0, 80.0], [0.0, 300.0, 60.0], [0.0, 0.0, 1.0]])
    coords = np.zeros((b, oc, R, kp, 2), np.float32)
    for o in range(oc):
        for r in range(R):
            xy = P.project(X[o], K, P.rodrigues(rng.normal(size=3)), np.array([0.02 * r, 0.01 * o, 0.6]))
            coords[0, o, r] = xy[:, ::-1] + rng.normal(0, 0.3, (kp, 2))
    counts = np.array([[[100, 100], [100, 5]]])
    cov = np.tile(np.array([4.0, 0.5, 1.0], np.float32), (b, oc, R, kp, 1))
    cov[0, 0, 1, 2] = np.nan                                 # one keypoint without a covariance: that slot is solved unweighted
    seen = []
    real = P.pnp_rvec_t

    def spy(points_3d, points_2d, camera_matrix, init_pose=None, rng=None, cov=None):
        seen.append(None if cov is None else np.array(cov))
        return real(points_3d, points_2d, camera_matrix, init_pose=init_pose, rng=rng, cov=cov)

    monkeypatch.setattr(P, "pnp_rvec_t", spy)
    plain = IV.poses_pnp_instances(coords, counts, X, K, rng=np.random.default_rng(0))
    assert plain.shape == (1, 2, 2, 3, 4) and all(c is None for c in seen) and len(seen) == 3
    del seen[:]
    poses, weighted = IV.poses_pnp_instances(coords, counts, X, K, rng=np.random.default_rng(0), cov=cov, return_weighted=True)
    assert weighted.tolist() == [[[1, 0], [1, 0]]] and weighted.dtype == np.int32          # the NaN slot falls back, the small slot is not solved
    assert len(seen) == 3 and seen[0][0] == pytest.approx([4.0 + P.COV_FLOOR, 0.5, 1.0 + P.COV_FLOOR])       # the floor poses_pnp applies
    assert np.array_equal(poses[0, 0, 1], plain[0, 0, 1]) and not poses[0, 1, 1].any()                        # the fall-back is the unweighted solve
    assert not np.array_equal(poses[0, 0, 0], plain[0, 0, 0])
    p2, w2 = IV.poses_pnp_instances(coords, counts, X, K, rng=np.random.default_rng(0), return_weighted=True)
    assert np.array_equal(p2, plain) and not w2.any()
    with pytest.raises(ValueError, match="cov must be"):
        IV.poses_pnp_instances(coords, counts, X, K, cov=cov[:, :, :1])

    class Solver:
        def solve(self, xy, x3, cams, mask, affine=None, cov=None):
            self.got = cov
            self.last_info = np.zeros(mask.shape + (4,), np.int32)
            self.last_weighted = None if cov is None else (mask * 7 // 7).astype(np.int32)
            return np.zeros(mask.shape + (3, 4), np.float32)

    s = Solver()
    t = torch.from_numpy(cov)
    _, w = IV.poses_pnp_instances(coords, counts, X, K, solver=s, cov=t, return_weighted=True)
    assert isinstance(s.got, torch.Tensor) and tuple(s.got.shape) == (1, 4, 9, 3) and s.got.data_ptr() == t.data_ptr()       # where it lies, reshaped only
    assert w.tolist() == [[[1, 1], [1, 0]]]
    IV.poses_pnp_instances(coords, counts, X, K, solver=s)
    assert s.got is None


def test_the_script_refuses_what_it_refused(script, monkeypatch, tmp_path):  # noqa: F811
    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the switches were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(script.test_minimal, "main", no_device)
    args = ["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)]
    monkeypatch.setenv("CASAPOSE_INSTANCE_PNP", "weighted")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_PNP=weighted .*CASAPOSE_MAX_INSTANCES"):
        script.main(args)
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    monkeypatch.setenv("CASAPOSE_INSTANCE_PNP", "cov")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_PNP must be"):
        script.main(args)
    monkeypatch.setenv("CASAPOSE_INSTANCE_PNP", "weighted")
    for other in ("CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE"):                 # both stay refused, with the message they had
        monkeypatch.setenv(other, "1")
        with pytest.raises(ValueError, match=r"CASAPOSE_MAX_INSTANCES=2 does not combine with %s=1 \(keypoint covariances and the mask refinement are per object\)" % other):
            script.main(args)
        monkeypatch.delenv(other)


def run_script(script, monkeypatch, tmp_path, capsys, pnp_switch, voter, split):  # noqa: F811
    """the script with stand-ins for everything that needs a device or a dataset -> (voters built, PnP calls, printed text, raw CSV bytes)"""
    built, solved = [], []

    class Voter:
        def __init__(self, name, num_classes, num_points, max_instances, **kw):
            built.append((name, num_classes, num_points, max_instances, kw))
            self.last_counts = torch.zeros(1, 8, 2, dtype=torch.int32)
            self.last_counts[0, 3, 1] = 77
            self.last_counts[0, 5, 0] = 60
            self.last_instances = torch.zeros(1, 8, 2, 4 if kw.get("split") == "votes" else 2, dtype=torch.int32)
            self.last_instances[0, 3, 1, 1] = 31
            self.last_kept = torch.full((1, 8, 2, 9), 0.75) if kw.get("voter") == "robust" else None
            self.last_cov = torch.ones(1, 8, 2, 9, 3) if kw.get("covariance") else None

        def __call__(self, inp):
            return torch.zeros(1, 8, 2, 9, 2)

    def pnp(coords, counts, keypoints, camera_matrix, min_num, rng, **kw):
        solved.append(sorted(kw))
        out = np.zeros((1, 8, 2, 3, 4), np.float32)
        out[0, 3, 1] = np.arange(12).reshape(3, 4)
        out[0, 5, 0] = 1 + np.arange(12).reshape(3, 4)
        if not kw:
            return out
        assert kw["cov"] is not None and kw["return_weighted"] is True
        weighted = np.zeros((1, 8, 2), np.int32)
        weighted[0, 3, 1] = 1                                  # (5, 0) fell back
        return out, weighted

    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    for name, value in (("CASAPOSE_INSTANCE_PNP", pnp_switch), ("CASAPOSE_INSTANCE_VOTER", voter), ("CASAPOSE_INSTANCE_SPLIT", split)):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
    for name, stand_in in (("ImageOnlyDataset", Frames), ("VectorfieldDataset", Annotated), ("InstanceLSVoting", Voter), ("poses_pnp_instances", pnp),
                           ("latest_checkpoint", lambda path: None)):
        monkeypatch.setattr(script, name, stand_in)
    monkeypatch.setattr(script.Classifiers, "get", staticmethod(lambda name: Net))
    for name, stand_in in (("is_available", lambda: True), ("set_device", lambda d: None), ("current_device", lambda: 0), ("synchronize", lambda d=None: None)):
        monkeypatch.setattr(torch.cuda, name, stand_in)
    out = str(tmp_path / ("run_%s_%s_%s" % (pnp_switch, voter, split)))
    script.main(["-c", CFG, "--outf", out, "--datatest", str(tmp_path), "--write_poses", "1"])
    return built, solved, capsys.readouterr().out, open(out + "/poses_est.csv", "rb").read()


@pytest.mark.parametrize("voter", [None, "robust"])
@pytest.mark.parametrize("split", [None, "votes"])
def test_plain_and_unset_are_the_same_path_and_weighted_adds_the_column(script, monkeypatch, tmp_path, capsys, split, voter):  # noqa: F811
    kw = {"split": "votes" if split else "components", **({"voter": "robust"} if voter else {})}
    unset = run_script(script, monkeypatch, tmp_path, capsys, None, voter, split)
    plain = run_script(script, monkeypatch, tmp_path, capsys, "plain", voter, split)
    assert unset[0] == plain[0] == [("coords_ls_voting", 9, 9, 2, kw)]                      # no `covariance` argument at all
    assert unset[1] == plain[1] and all(call == [] for call in unset[1])                   # the PnP is called with the arguments it had
    assert unset[3] == plain[3] and LINE not in unset[2] and LINE not in plain[2]          # the CSV byte for byte
    assert [ln for ln in unset[2].splitlines() if ln.startswith("instances:")] == [ln for ln in plain[2].splitlines() if ln.startswith("instances:")]
    rows = list(csv.reader(unset[3].decode().splitlines()))
    assert rows[0] == OLD_HEADER + (["votes"] if split else []) + (["kept"] if voter else [])

    built, solved, printed, raw = run_script(script, monkeypatch, tmp_path, capsys, "weighted", voter, split)
    assert built == [("coords_ls_voting", 9, 9, 2, dict(kw, covariance=True))]
    assert solved and all(call == ["cov", "return_weighted"] for call in solved)
    assert printed.count(LINE) == 1 and printed.count("instances: up to 2 per object") == 1
    lines = [ln for ln in printed.splitlines() if ln.startswith("instances:")]
    assert lines[-1] == LINE and lines[:-1] == [ln for ln in unset[2].splitlines() if ln.startswith("instances:")]
    new_rows = list(csv.reader(raw.decode().splitlines()))
    assert new_rows[0] == rows[0] + ["weighted"] and len(new_rows) == len(rows)
    assert all(r[:-1] == old for r, old in zip(new_rows, rows))                             # every earlier column as it was
    by_object = {(r[0], r[1]): r[-1] for r in new_rows[1:]}
    assert by_object[("000000", NAMES[3])] == "1" and by_object[("000000", NAMES[5])] == "0" and by_object[("000000", NAMES[0])] == "0"
    assert all(len(r) == len(new_rows[0]) and r[-1] in ("0", "1") for r in new_rows[1:])
