"""CASAPOSE_MAX_INSTANCES and util_scripts/minimal_instances.py: how the variable is read, which switch combinations are refused before any
device work, that with the variable unset the script is util_scripts/test_minimal.py's main() and nothing else (shown without a GPU, with
stand-ins for the dataset, the network, the voters and the PnP), and, on the GPU, the poses_est.csv of CASAPOSE_MAX_INSTANCES=2 on the synthetic
folder of tests/test_gpu_frames.py."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "config_8.ini")
NAMES = "obj_000001,obj_000005,obj_000006,obj_000008,obj_000009,obj_000010,obj_000011,obj_000012".split(",")
SWITCHES = ("CASAPOSE_MAX_INSTANCES", "CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE", "CASAPOSE_DEVICE_PNP")


@pytest.fixture
def script(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "util_scripts"))
    import minimal_instances

    return minimal_instances


def test_the_variable_is_parsed_as_specified(monkeypatch):
    from casapose_amd.pose_estimation.instance_voting import max_instances_from_environment as read

    monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False)
    assert read() is None
    for raw, want in (("1", None), (" 1 ", None), ("2", 2), ("4", 4), ("16", 16), (" 3", 3)):
        monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", raw)
        assert read() == want
    for raw in ("0", "17", "-2", "", "two", "2.0", "4,4"):
        monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", raw)
        with pytest.raises(ValueError, match="CASAPOSE_MAX_INSTANCES"):
            read()


def test_the_one_instance_voter_says_that_it_ignores_the_switch(monkeypatch, recwarn):
    """test_minimal.py and test_casapose.py do not read the switch; the voter they build warns instead of ignoring it in silence"""
    from casapose_amd.pose_estimation.voting_layers_2d import CoordLSVotingWeighted

    for value in (None, "1"):
        monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False) if value is None else monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", value)
        CoordLSVotingWeighted("v", 9, filter_estimates=True)
    assert len(recwarn) == 0
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "4")
    with pytest.warns(UserWarning, match="CASAPOSE_MAX_INSTANCES is set.*minimal_instances.py"):
        CoordLSVotingWeighted("v", 9, filter_estimates=True)


@pytest.mark.parametrize("other", ["CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE"])
def test_refused_combinations_name_both_switches(script, monkeypatch, tmp_path, other):
    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the switches were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "3")
    monkeypatch.setenv(other, "1")
    with pytest.raises(ValueError, match="CASAPOSE_MAX_INSTANCES=3 .*%s=1" % other):
        script.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)])
    monkeypatch.setenv(other, "0")                     # the other switch off: the script goes on to ask for the device
    with pytest.raises(AssertionError, match="the device was asked for"):
        script.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)])


class Frames:
    def __init__(self, root):
        pass

    def __len__(self):
        return 2

    def __getitem__(self, i):
        return {"name": "%06d" % i}

    def frame_shape(self):
        return 480, 640, 3

    def generate_dataset(self, batch, device=None):
        return iter([torch.zeros(1, 480, 640, 3)] * 2), 2


class Annotated:
    def __init__(self, **kw):
        pass

    def generate_dataset(self, *a, **k):
        return iter([{"keypoints3d": np.zeros((1, 8, 1, 9, 3), np.float32), "cam_mat": np.eye(3, dtype=np.float32)[None]}]), None


class Net:
    layers = ()

    def __init__(self, **kw):
        pass

    def summary(self):
        pass

    def __call__(self, inputs, training=False):
        return torch.zeros(1, 480, 640, 36)


@pytest.mark.parametrize("value", [None, "1"])
def test_unset_takes_the_old_path(script, monkeypatch, tmp_path, capsys, value):
    """stand-ins for everything that needs a device or a dataset: the old voter and poses_pnp are what main() calls, the new ones are never
    touched, and the files have the old columns"""
    calls = []

    class OldVoter:
        def __init__(self, name, num_classes, num_points, filter_estimates):
            calls.append(("CoordLSVotingWeighted", num_classes, num_points, filter_estimates))

        def __call__(self, inp):
            return torch.zeros(1, 8, 9, 2)

    def old_pnp(coords, seg, keypoints, camera_matrix, no_objects, min_num, rng):
        calls.append(("poses_pnp", no_objects, min_num))
        out = np.zeros((1, 8, 1, 3, 4), np.float32)
        out[0, 3, 0] = np.arange(12).reshape(3, 4)
        return out

    def new(*a, **k):
        raise AssertionError("the instance path was taken with the switch unset")

    if value is not None:
        monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", value)
    old_script = script.test_minimal
    for name, stand_in in (("ImageOnlyDataset", Frames), ("VectorfieldDataset", Annotated), ("CoordLSVotingWeighted", OldVoter), ("poses_pnp", old_pnp),
                           ("latest_checkpoint", lambda path: None)):
        monkeypatch.setattr(old_script, name, stand_in)
    for name in ("InstanceLSVoting", "poses_pnp_instances", "ImageOnlyDataset", "VectorfieldDataset", "parse_config"):
        monkeypatch.setattr(script, name, new)
    assert not hasattr(old_script, "InstanceLSVoting")            # test_minimal.py does not know the instance path
    monkeypatch.setattr(old_script.Classifiers, "get", staticmethod(lambda name: Net))
    for name, stand_in in (("is_available", lambda: True), ("set_device", lambda d: None), ("current_device", lambda: 0), ("synchronize", lambda d=None: None)):
        monkeypatch.setattr(torch.cuda, name, stand_in)
    out = str(tmp_path / "run")
    res = script.main(["-c", CFG, "--outf", out, "--datatest", str(tmp_path), "--write_poses", "1"])
    assert calls == [("CoordLSVotingWeighted", 9, 9, True), ("poses_pnp", 8, 200), ("poses_pnp", 8, 200)]
    assert "instances:" not in capsys.readouterr().out
    rows = list(csv.reader(open(out + "/poses_est.csv")))
    assert rows[0] == ["name", "object"] + ["r%d%d" % (i, j) for i in range(1, 4) for j in range(1, 4)] + ["t1", "t2", "t3"]
    assert len(rows) == 1 + 2 * 8 and all(len(r) == 14 for r in rows) and rows[4][:2] == ["000000", NAMES[3]]
    assert [float(v) for v in rows[4][2:]] == [0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 7, 11]
    assert sorted(res["poses"]) == ["000000", "000001"] and res["poses"]["000000"].shape == (8, 3, 4)


@pytest.mark.gpu
def test_two_instances_on_the_synthetic_folder(script, device, monkeypatch, tmp_path, capsys):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.data_handler.vectorfield_dataset import write_ndds_scene
    from casapose_amd.pose_models.tfkeras import Classifiers

    frames = 3
    data, models, out = str(tmp_path / "data"), str(tmp_path / "models"), str(tmp_path / "run")
    write_ndds_scene(data, models, SyntheticSceneDataset(8, (480, 640), length=frames, seed=5), frames, NAMES)
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=9, input_shape=(480, 640, 3), weights=None, device=device, seed=21)
    os.makedirs(out + "/frozen_model")
    net.save_weights(out + "/frozen_model/result_w.h5")
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    res = script.main(["-c", CFG, "--outf", out, "--manualseed", "7", "--datatest", data, "--datameshes", models, "--load_h5_weights", "1",
                       "--object", ",".join(NAMES), "--write_poses", "1", "--min_object_size_test", "20"])
    assert capsys.readouterr().out.count("instances: up to 2 per object") == 1
    rows = list(csv.reader(open(out + "/poses_est.csv")))
    assert rows[0] == ["name", "object"] + ["r%d%d" % (i, j) for i in range(1, 4) for j in range(1, 4)] + ["t1", "t2", "t3", "instance", "pixels"]
    assert all(len(r) == 16 for r in rows) and sorted(res["poses"]) == ["%06d" % i for i in range(frames)]
    at, found, second = 1, 0, 0
    for i in range(frames):
        got = res["poses"]["%06d" % i]
        assert got.shape == (8, 2, 3, 4) and np.isfinite(got).all()
        for o in range(8):
            inst = [r for r in range(2) if got[o, r].any()]
            found += len(inst)
            second += inst[-1:] == [1]
            for r in inst or [0]:
                row = rows[at]
                at += 1
                assert row[:2] == ["%06d" % i, NAMES[o]] and int(row[14]) == r
                assert np.allclose([float(v) for v in row[2:14]], np.concatenate([got[o, r, :, :3].reshape(-1), got[o, r, :, 3]]), rtol=1e-7, atol=1e-7)
                assert (int(row[15]) > 20) if inst else (row[14:] == ["0", "0"] and not got[o].any())
    assert at == len(rows)
    print("instances found in %d frames: %d, second instances: %d" % (frames, found, second))
    assert found > 0 and second > 0, "no instance rows, or no object with a second instance: only the zero rows were checked"
