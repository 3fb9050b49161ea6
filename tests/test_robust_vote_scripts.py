"""CASAPOSE_INSTANCE_VOTER and util_scripts/minimal_instances.py: how the variable is read and what it refuses, that InstanceLSVoting takes the
voter by name, and -- shown without a GPU, with stand-ins for the dataset, the network, the voter and the PnP -- that with the switch unset or
`ls` the script builds the voter it built before, prints what it printed and writes the CSV it wrote, and under `robust` says so once and adds
the column `kept` after whatever columns are there.  No GPU."""
import csv
import os

import numpy as np
import pytest
import torch

from test_instances_scripts import CFG, NAMES, Annotated, Frames, Net
from test_vote_split_scripts import OLD_HEADER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("CASAPOSE_MAX_INSTANCES", "CASAPOSE_INSTANCE_SPLIT", "CASAPOSE_INSTANCE_VOTER", "CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE",
            "CASAPOSE_DEVICE_PNP")
LINE = "instances: robust voter (cutoff 4 px, 2 passes)"


@pytest.fixture
def script(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "util_scripts"))
    import minimal_instances

    return minimal_instances


def test_the_switch_is_parsed_as_specified(monkeypatch):
    from casapose_amd.pose_estimation.instance_voting import instance_voter_from_environment as read

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert read() == "ls"
    monkeypatch.setenv("CASAPOSE_INSTANCE_VOTER", "ls")
    assert read() == "ls"                                  # without CASAPOSE_MAX_INSTANCES too: it is the existing path
    for raw in ("Robust", "ROBUST", "", "1", "tukey", "ransac"):
        monkeypatch.setenv("CASAPOSE_INSTANCE_VOTER", raw)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_VOTER must be unset, `ls` or `robust`"):
            read()
    monkeypatch.setenv("CASAPOSE_INSTANCE_VOTER", "robust")
    for instances in (None, "1"):                       # one instance per object: the switch belongs to the instance path
        monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False) if instances is None else monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", instances)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_VOTER=robust .*CASAPOSE_MAX_INSTANCES"):
            read()
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "4")
    assert read() == "robust"
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "40")      # the other variable's own refusal comes through
    with pytest.raises(ValueError, match="CASAPOSE_MAX_INSTANCES must be"):
        read()


def test_the_voter_is_taken_by_name():
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    v = InstanceLSVoting("v", 9)
    assert v.voter == "ls" and v.last_kept is None
    v = InstanceLSVoting("v", 9, split="votes", voter="robust")
    assert (v.voter, v.cutoff, v.passes, v.split) == ("robust", 4.0, 2, "votes")
    v = InstanceLSVoting("v", 9, voter="robust", cutoff=2, passes=0)
    assert (v.cutoff, v.passes) == (2.0, 0)
    with pytest.raises(ValueError, match="voter must be one of"):
        InstanceLSVoting("v", 9, voter="ransac")
    for kw in (dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(passes=-1), dict(passes=9), dict(passes=1.5)):
        with pytest.raises(ValueError, match="cutoff must be finite and > 0 and passes an integer in 0..8"):
            InstanceLSVoting("v", 9, voter="robust", **kw)


def test_the_plain_voter_is_called_as_before(monkeypatch):
    """voter="ls" (the default) goes through ops.ls_vote_slots with the arguments it had and never touches the robust entry"""
    from casapose_amd import ops
    from casapose_amd.pose_estimation import instance_voting as IV

    calls = []

    class Cuda(torch.Tensor):
        is_cuda = True

    def labels(rec, classes, offset):
        return torch.zeros(rec.shape[:3], dtype=torch.uint8)

    def ccl(lab0, objects, R, min_size):
        return lab0, torch.zeros(lab0.shape[0], objects, R, 2, dtype=torch.int32)

    def plain(rec, do, co, slots, kp, slot_map, sigmoid_weights=False):
        calls.append(("ls", do, co, slots, kp, sigmoid_weights))
        return torch.zeros(rec.shape[0], slots, kp, 2)

    def robust(rec, do, co, slots, kp, slot_map, cutoff, passes, sigmoid_weights, return_sums):
        calls.append(("robust", do, co, slots, kp, cutoff, passes, sigmoid_weights, return_sums))
        plain_sums = torch.ones(rec.shape[0], slots, kp, 5, dtype=torch.float64)
        plain_sums[:, 1:] = 0.0
        return torch.zeros(rec.shape[0], slots, kp, 2), plain_sums, 0.25 * plain_sums

    monkeypatch.setattr(ops, "argmax_labels", labels)
    monkeypatch.setattr(ops, "ccl_instance_labels", ccl)
    monkeypatch.setattr(ops, "ls_vote_slots", plain)
    monkeypatch.setattr(ops, "ls_vote_slots_robust", robust)
    rec = torch.zeros(1, 4, 8, 36).as_subclass(Cuda)
    inp = [rec[..., :9], rec[..., 9:27], rec[..., 27:]]
    monkeypatch.setattr(IV, "_as_record", lambda seg, direct, conf: (rec, (1, 9, 27)))     # so != 0: the cached labels are not asked
    v = IV.InstanceLSVoting("v", 9, max_instances=2)
    assert tuple(v(inp).shape) == (1, 8, 2, 9, 2) and calls == [("ls", 9, 27, 16, 9, False)] and v.last_kept is None
    del calls[:]
    v = IV.InstanceLSVoting("v", 9, max_instances=2, voter="robust", cutoff=3.0, passes=1, sigmoid_weights=True)
    assert tuple(v(inp).shape) == (1, 8, 2, 9, 2) and calls == [("robust", 9, 27, 16, 9, 3.0, 1, True, True)]
    kept = v.last_kept
    assert kept.dtype == torch.float32 and tuple(kept.shape) == (1, 8, 2, 9)
    assert bool((kept[0, 0, 0] == 0.25).all()) and not kept[0, 0, 1].any() and not kept[0, 1:].any()      # the traces' ratio; 0 for an empty slot


def test_the_script_refuses_robust_without_instances_before_any_device_work(script, monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the switches were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(script.test_minimal, "main", no_device)
    monkeypatch.setenv("CASAPOSE_INSTANCE_VOTER", "robust")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_VOTER=robust .*CASAPOSE_MAX_INSTANCES"):
        script.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)])
    monkeypatch.setenv("CASAPOSE_INSTANCE_VOTER", "tukey")
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_VOTER"):
        script.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)])


def run_script(script, monkeypatch, tmp_path, capsys, voter, split):
    """the script with stand-ins for everything that needs a device or a dataset -> (voters built, printed text, raw CSV bytes)"""
    built = []

    class Voter:
        def __init__(self, name, num_classes, num_points, max_instances, **kw):
            built.append((name, num_classes, num_points, max_instances, kw))
            self.last_counts = torch.zeros(1, 8, 2, dtype=torch.int32)
            self.last_counts[0, 3, 1] = 77
            self.last_instances = torch.zeros(1, 8, 2, 4 if kw.get("split") == "votes" else 2, dtype=torch.int32)
            self.last_instances[0, 3, 1, 1] = 31
            self.last_kept = None
            if kw.get("voter") == "robust":
                self.last_kept = torch.zeros(1, 8, 2, 9)
                self.last_kept[0, 3, 1] = torch.linspace(0.5, 0.9, 9)          # mean 0.7

        def __call__(self, inp):
            return torch.zeros(1, 8, 2, 9, 2)

    def pnp(coords, counts, keypoints, camera_matrix, min_num, rng):
        out = np.zeros((1, 8, 2, 3, 4), np.float32)
        out[0, 3, 1] = np.arange(12).reshape(3, 4)
        return out

    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    for name, value in (("CASAPOSE_INSTANCE_VOTER", voter), ("CASAPOSE_INSTANCE_SPLIT", split)):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
    for name, stand_in in (("ImageOnlyDataset", Frames), ("VectorfieldDataset", Annotated), ("InstanceLSVoting", Voter), ("poses_pnp_instances", pnp),
                           ("latest_checkpoint", lambda path: None)):
        monkeypatch.setattr(script, name, stand_in)
    monkeypatch.setattr(script.Classifiers, "get", staticmethod(lambda name: Net))
    for name, stand_in in (("is_available", lambda: True), ("set_device", lambda d: None), ("current_device", lambda: 0), ("synchronize", lambda d=None: None)):
        monkeypatch.setattr(torch.cuda, name, stand_in)
    out = str(tmp_path / ("run_%s_%s" % (voter, split)))
    script.main(["-c", CFG, "--outf", out, "--datatest", str(tmp_path), "--write_poses", "1"])
    return built, capsys.readouterr().out, open(out + "/poses_est.csv", "rb").read()


@pytest.mark.parametrize("split", [None, "votes"])
def test_ls_and_unset_are_the_same_path_and_robust_adds_the_column(script, monkeypatch, tmp_path, capsys, split):
    votes = split == "votes"
    unset = run_script(script, monkeypatch, tmp_path, capsys, None, split)
    ls = run_script(script, monkeypatch, tmp_path, capsys, "ls", split)
    assert unset[0] == ls[0] == [("coords_ls_voting", 9, 9, 2, {"split": "votes" if votes else "components"})]      # no `voter` argument at all
    assert unset[2] == ls[2] and LINE not in unset[1] and LINE not in ls[1]                                          # the CSV byte for byte
    assert [ln for ln in unset[1].splitlines() if ln.startswith("instances:")] == [ln for ln in ls[1].splitlines() if ln.startswith("instances:")]
    rows = list(csv.reader(unset[2].decode().splitlines()))
    assert rows[0] == OLD_HEADER + (["votes"] if votes else [])

    built, printed, raw = run_script(script, monkeypatch, tmp_path, capsys, "robust", split)
    assert built == [("coords_ls_voting", 9, 9, 2, {"split": "votes" if votes else "components", "voter": "robust"})]
    assert printed.count(LINE) == 1 and printed.count("instances: up to 2 per object") == 1
    robust_rows = list(csv.reader(raw.decode().splitlines()))
    assert robust_rows[0] == rows[0] + ["kept"] and len(robust_rows) == len(rows) == 1 + 2 * 8
    assert all(r[:-1] == old for r, old in zip(robust_rows, rows))               # every earlier column as it was
    assert robust_rows[4][:2] == ["000000", NAMES[3]] and float(robust_rows[4][-1]) == pytest.approx(0.7, abs=1e-6)
    assert robust_rows[1][-1] == "0" and all(len(r) == len(robust_rows[0]) for r in robust_rows)
