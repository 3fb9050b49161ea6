"""CASAPOSE_INSTANCE_SPLIT and util_scripts/minimal_instances.py: how the variable is read and what it refuses, that InstanceLSVoting takes the
split by name, and -- shown without a GPU, with stand-ins for the dataset, the network, the voter and the PnP -- that with the switch unset the
script builds the voter it built before and writes the CSV header it wrote before, and under `votes` says so once and adds the column.  No GPU."""
import csv
import os

import numpy as np
import pytest
import torch

from test_instances_scripts import CFG, NAMES, Annotated, Frames, Net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("CASAPOSE_MAX_INSTANCES", "CASAPOSE_INSTANCE_SPLIT", "CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE", "CASAPOSE_DEVICE_PNP")
OLD_HEADER = ["name", "object"] + ["r%d%d" % (i, j) for i in range(1, 4) for j in range(1, 4)] + ["t1", "t2", "t3", "instance", "pixels"]


@pytest.fixture
def script(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "util_scripts"))
    import minimal_instances

    return minimal_instances


def test_the_switch_is_parsed_as_specified(monkeypatch):
    from casapose_amd.pose_estimation.instance_voting import instance_split_from_environment as read

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert read() == "components"
    monkeypatch.setenv("CASAPOSE_INSTANCE_SPLIT", "components")
    assert read() == "components"
    for raw in ("vote", "VOTES", "", "1", "hough"):
        monkeypatch.setenv("CASAPOSE_INSTANCE_SPLIT", raw)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SPLIT"):
            read()
    monkeypatch.setenv("CASAPOSE_INSTANCE_SPLIT", "votes")
    for instances in (None, "1"):                       # one instance per object: nothing to split
        monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False) if instances is None else monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", instances)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SPLIT=votes .*CASAPOSE_MAX_INSTANCES"):
            read()
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "4")
    assert read() == "votes"
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "40")      # the other variable's own refusal comes through
    with pytest.raises(ValueError, match="CASAPOSE_MAX_INSTANCES must be"):
        read()


def test_the_voter_takes_the_split_by_name():
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    v = InstanceLSVoting("v", 9)
    assert v.split == "components" and v.last_peaks is None
    v = InstanceLSVoting("v", 9, split="votes", min_component=30, gate=3.0)
    assert v.split == "votes" and v.min_component == 30
    assert v.split_params == dict(cell=4, vote_stride=2, min_votes=12, rel_percent=25, nms_radius=2, gate=3.0)
    with pytest.raises(ValueError, match="split must be one of"):
        InstanceLSVoting("v", 9, split="hough")


def test_the_script_refuses_votes_without_instances_before_any_device_work(script, monkeypatch, tmp_path):
    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the switches were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(script.test_minimal, "main", no_device)
    monkeypatch.setenv("CASAPOSE_INSTANCE_SPLIT", "votes")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SPLIT=votes .*CASAPOSE_MAX_INSTANCES"):
        script.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)])
    monkeypatch.setenv("CASAPOSE_INSTANCE_SPLIT", "hough")
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SPLIT"):
        script.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)])


@pytest.mark.parametrize("split", [None, "components", "votes"])
def test_the_csv_and_the_voter_under_the_switch(script, monkeypatch, tmp_path, capsys, split):
    """stand-ins for everything that needs a device or a dataset.  Unset or `components`: the voter is built with the arguments it was built with
    before this switch existed plus split="components", nothing new is printed and the header is the old one.  `votes`: split="votes", the line
    once, the column `votes` with the peak's votes."""
    built = []

    class Voter:
        def __init__(self, name, num_classes, num_points, max_instances, **kw):
            built.append((name, num_classes, num_points, max_instances, kw))
            self.last_counts = torch.zeros(1, 8, 2, dtype=torch.int32)
            self.last_counts[0, 3, 1] = 77
            self.last_instances = torch.zeros(1, 8, 2, 4 if kw.get("split") == "votes" else 2, dtype=torch.int32)
            self.last_instances[0, 3, 1, 1] = 31

        def __call__(self, inp):
            return torch.zeros(1, 8, 2, 9, 2)

    def pnp(coords, counts, keypoints, camera_matrix, min_num, rng):
        out = np.zeros((1, 8, 2, 3, 4), np.float32)
        out[0, 3, 1] = np.arange(12).reshape(3, 4)
        return out

    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    if split is not None:
        monkeypatch.setenv("CASAPOSE_INSTANCE_SPLIT", split)
    for name, stand_in in (("ImageOnlyDataset", Frames), ("VectorfieldDataset", Annotated), ("InstanceLSVoting", Voter), ("poses_pnp_instances", pnp),
                           ("latest_checkpoint", lambda path: None)):
        monkeypatch.setattr(script, name, stand_in)
    monkeypatch.setattr(script.Classifiers, "get", staticmethod(lambda name: Net))
    for name, stand_in in (("is_available", lambda: True), ("set_device", lambda d: None), ("current_device", lambda: 0), ("synchronize", lambda d=None: None)):
        monkeypatch.setattr(torch.cuda, name, stand_in)
    out = str(tmp_path / "run")
    script.main(["-c", CFG, "--outf", out, "--datatest", str(tmp_path), "--write_poses", "1"])
    printed = capsys.readouterr().out
    rows = list(csv.reader(open(out + "/poses_est.csv")))
    votes = split == "votes"
    assert built == [("coords_ls_voting", 9, 9, 2, {"split": "votes" if votes else "components"})]
    assert printed.count("instances: up to 2 per object") == 1 and printed.count("instances: split by centre votes") == (1 if votes else 0)
    assert rows[0] == OLD_HEADER + (["votes"] if votes else [])
    assert len(rows) == 1 + 2 * 8 and all(len(r) == len(rows[0]) for r in rows)
    assert rows[4][:2] == ["000000", NAMES[3]] and rows[4][14:] == (["1", "77", "31"] if votes else ["1", "77"])
    assert rows[1][14:] == (["0", "0", "0"] if votes else ["0", "0"])
