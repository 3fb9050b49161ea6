"""The verified score in the scripts: CASAPOSE_POSE_SCORE=1 (training.test_step, test_casapose.py, io_utils.write_poses) and
CASAPOSE_INSTANCE_SCORE=verify (util_scripts/minimal_instances.py): how the switches are read, what is refused before any device work, the rows
write_poses and write_bop_instances write, and the columns of poses_est.csv -- shown without a GPU, with stand-ins for the dataset, the network,
the voter, the PnP and the verifier, in the style of tests/test_slot_cov_scripts.py."""
import csv
import os

import numpy as np
import pytest
import torch

import contour_cases as CC
from test_instances_scripts import CFG, NAMES, Annotated, Frames, Net, script  # noqa: F401
from test_mask_refine_scripts import IDENTITY, Dataset, write_obj

SWITCHES = ("CASAPOSE_MAX_INSTANCES", "CASAPOSE_INSTANCE_SPLIT", "CASAPOSE_INSTANCE_VOTER", "CASAPOSE_INSTANCE_PNP", "CASAPOSE_INSTANCE_SCORE",
            "CASAPOSE_POSE_SCORE", "CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE", "CASAPOSE_DEVICE_PNP")
OLD_HEADER = ["name", "object"] + ["r%d%d" % (i, j) for i in range(1, 4) for j in range(1, 4)] + ["t1", "t2", "t3", "instance", "pixels"]
LINE = "instances: verified scores"


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


# ---- the switches ---------------------------------------------------------------------------------------------------------------------------
def test_pose_score_switch_is_read_like_the_refiners(monkeypatch, capsys):
    from casapose_amd.pose_estimation import pose_verify as V

    monkeypatch.setattr(V.pose_score_enabled, "said", False)
    assert not V.pose_score_enabled()
    monkeypatch.setenv("CASAPOSE_POSE_SCORE", "0")
    assert not V.pose_score_enabled() and capsys.readouterr().out == ""
    assert V.verifier_from_environment(None, None, None, "cuda:0") is None
    monkeypatch.setenv("CASAPOSE_POSE_SCORE", "1")
    assert V.pose_score_enabled() and V.pose_score_enabled()
    assert capsys.readouterr().out.count("score: verified poses") == 1              # said once


def test_instance_score_switch_is_parsed_as_specified(monkeypatch):
    from casapose_amd.pose_estimation.pose_verify import instance_score_from_environment as read

    assert read() == "none"
    monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", "none")
    assert read() == "none"                                # without CASAPOSE_MAX_INSTANCES too: it is the existing path
    for raw in ("Verify", "VERIFY", "", "1", "score", "votes"):
        monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", raw)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SCORE must be unset, `none` or `verify`"):
            read()
    monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", "verify")
    for instances in (None, "1"):
        monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False) if instances is None else monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", instances)
        with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SCORE=verify .*CASAPOSE_MAX_INSTANCES"):
            read()
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "4")
    assert read() == " verify ".strip()
    monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", " verify ")
    assert read() == "verify"


def test_the_script_refuses_the_switch_without_instances(script, monkeypatch, tmp_path):  # noqa: F811
    def no_device(*a, **k):
        raise AssertionError("the device was asked for before the switches were checked")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(script.test_minimal, "main", no_device)
    args = ["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)]
    monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", "verify")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SCORE=verify .*CASAPOSE_MAX_INSTANCES"):
        script.main(args)
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", "iou")
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SCORE must be"):
        script.main(args)


def test_test_step_refuses_before_the_forward_pass(monkeypatch):
    from casapose_amd.training import test_step

    class Net_:      # any use of the network, the options or the loss factors would raise: the offsets are looked at first
        @property
        def device(self):
            return "cpu"

    class Verifier:
        last_scores = last_counts = None

    bad = np.array([[16.0, 96.0, 448.0, 448.0, 0.0, 0.0, 0.0, 1.0, 640.0, 480.0]])
    with pytest.raises(ValueError, match="CASAPOSE_POSE_SCORE=1 needs frames that reach the network as they are"):
        test_step(Net_(), {"offsets": bad}, None, None, verifier=Verifier())
    opt = type("Opt", (), {"estimate_coords": False, "datameshes": "", "object": "a"})()
    with pytest.raises(ValueError, match="CASAPOSE_POSE_SCORE=1 needs estimate_coords = 1"):
        test_step(Net_(), {"offsets": np.array([IDENTITY])}, opt, None, verifier=Verifier())
    monkeypatch.setenv("CASAPOSE_POSE_SCORE", "1")                  # what test_casapose.py runs: no verifier is handed over
    with pytest.raises(ValueError, match="CASAPOSE_POSE_SCORE=1 needs frames that reach the network as they are"):
        test_step(Net_(), {"offsets": bad}, None, None)
    with pytest.raises(ValueError, match="CASAPOSE_POSE_SCORE=1 needs estimate_coords = 1"):
        test_step(Net_(), {"offsets": np.array([IDENTITY])}, opt, None)
    opt.estimate_coords = True                                      # without meshes: refused by name, before the forward pass
    with pytest.raises(ValueError, match="CASAPOSE_POSE_SCORE=1 needs the objects' mesh files"):
        test_step(Net_(), {"offsets": np.array([IDENTITY])}, opt, None)


def test_mesh_errors_name_the_switch_and_the_refiners_texts_stay(tmp_path, monkeypatch):
    from casapose_amd.pose_estimation import mask_refine as M
    from casapose_amd.pose_estimation import pose_verify as V

    def no_device(*a, **k):
        raise AssertionError("a verifier was built before the meshes were checked")

    meshes = CC.meshes()[:2]
    names = ["block", "ball"]
    for name, (v, f) in zip(names, meshes):
        (tmp_path / name).mkdir()
        write_obj(tmp_path / name / (name + ".obj"), v, f if name == "block" else [])
    monkeypatch.setattr(V, "DevicePoseVerifier", no_device)
    with pytest.raises(ValueError, match=r"^CASAPOSE_POSE_SCORE=1 needs meshes with faces to render: .*ball\.obj holds vertices only$"):
        V.verifier_for_dataset(Dataset(meshes), str(tmp_path), names, "cuda:0")
    with pytest.raises(ValueError, match="^CASAPOSE_POSE_SCORE=1 needs a mesh for every object: lamp has none under"):
        V.verifier_for_dataset(Dataset(meshes), str(tmp_path), ["block", "lamp"], "cuda:0")
    with pytest.raises(ValueError, match="^CASAPOSE_POSE_SCORE=1 needs the objects' mesh files under --datameshes"):
        V.verifier_for_dataset(object(), str(tmp_path), names, "cuda:0")
    with pytest.raises(ValueError) as e:                      # the refiner's own text, byte for byte
        M.refiner_for_meshes(None, None, "nowhere", names, "cuda:0")
    assert str(e.value) == "CASAPOSE_MASK_REFINE=1 needs the objects' mesh files under --datameshes (got 'nowhere')"
    bad = np.array([IDENTITY])
    bad[0, 7] = 0.5
    with pytest.raises(ValueError) as e:
        M.require_image_frame(bad)
    assert str(e.value) == ("CASAPOSE_MASK_REFINE=1 needs frames that reach the network as they are: the batch's offsets hold a crop, shift, rotation or "
                            "scale (h_crop, w_crop, dx, dy, angle, scale = [0.0, 0.0, 0.0, 0.0, 0.0, 0.5]), so the label map and the camera matrix do not "
                            "share a frame")
    assert V.require_image_frame is M.require_image_frame


def test_verifier_for_dataset_builds_a_host_verifier(tmp_path):
    from casapose_amd.pose_estimation import pose_verify as V

    meshes = CC.meshes()
    names = ["block", "occluder", "cut"]
    for name, (v, f) in zip(names, meshes):
        (tmp_path / name).mkdir()
        write_obj(tmp_path / name / (name + ".obj"), v, f)
    v = V.verifier_for_dataset(Dataset(meshes), str(tmp_path), names, None)
    assert isinstance(v, V.DevicePoseVerifier) and v.objects == 3 and v.sample_offset == 0.5 and v.device is None and 0 < v.near < v.far


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
def poses_for_rows():
    gt = np.zeros((3, 1, 3, 4), np.float32)
    gt[0, 0], gt[1, 0] = np.arange(12).reshape(3, 4) + 1, np.arange(12).reshape(3, 4) + 2        # object 2 is not in the frame
    est = np.zeros((3, 3, 4), np.float32)
    est[0] = 0.5 * np.arange(12).reshape(3, 4)                                                   # object 1 is in the frame and not found
    return gt, est


def test_write_poses_rows_with_and_without_scores(tmp_path):
    from casapose_amd.utils.io_utils import write_poses

    gt, est = poses_for_rows()
    names = ["obj_000001", "obj_000005", "obj_000006"]
    plain, scored = str(tmp_path / "plain") + "/", str(tmp_path / "scored") + "/"
    write_poses(gt, est, names, ["000002_rgb_000031"], plain, 0.25)
    write_poses(gt, est, names, ["000002_rgb_000031"], scored, 0.25, scores=np.array([0.7283950617283951, 0.9, 0.4]))
    R, t = "0.0 0.5 1.0 2.0 2.5 3.0 4.0 4.5 5.0", "1.5 3.5 5.5"
    zero_R, zero_t = " ".join(["0.0"] * 9), " ".join(["0.0"] * 3)
    header = open(plain + "bop_evaluation.csv").readline()
    # without `scores`: the bytes the function has always written -- score 1.0 for a found estimate, 0.0 for the zero pose
    assert open(plain + "bop_evaluation.csv").read() == header + "2,31,1,1.0,%s,%s,0.25\n2,31,5,0.0,%s,%s,0.25\n" % (R, t, zero_R, zero_t)
    # with them: repr(float) for the found estimate, still 0.0 for the zero pose whatever its score says
    assert open(scored + "bop_evaluation.csv").read() == header + "2,31,1,0.7283950617283951,%s,%s,0.25\n2,31,5,0.0,%s,%s,0.25\n" % (R, t, zero_R, zero_t)
    for sub in ("all_poses", "filtered_poses"):
        for fn in sorted(os.listdir(plain + sub)):
            assert open(plain + sub + "/" + fn, "rb").read() == open(scored + sub + "/" + fn, "rb").read()
    with pytest.raises(ValueError, match="scores holds one value per object"):
        write_poses(gt, est, names, ["000002_rgb_000031"], scored, 0.25, scores=np.zeros(2))


def test_write_bop_instances_rows(tmp_path):
    from casapose_amd.pose_estimation import bop_scores
    from casapose_amd.utils.io_utils import BOP_HEADER, write_bop_instances

    poses = np.zeros((2, 3, 3, 4), np.float32)
    poses[0, 1], poses[1, 0], poses[1, 2] = np.arange(12).reshape(3, 4), 1 + np.arange(12).reshape(3, 4), 2 + np.arange(12).reshape(3, 4)
    scores = np.array([[9.0, 0.125, 9.0], [0.75, 9.0, 1 / 3]])
    path = str(tmp_path / "bop_instances.csv")
    write_bop_instances(path, "000004_000017", ["obj_000005", "obj_000011"], poses, scores, 0.5)
    write_bop_instances(path, ["000023"], ["obj_000005", "obj_000011"], poses[:, :1], scores[:, :1])
    rows = list(csv.reader(open(path)))
    assert open(path).readline() == BOP_HEADER and len(rows) == 1 + 3 + 1
    assert [r[:4] + r[-1:] for r in rows[1:]] == [["4", "17", "5", "0.125", "0.5"], ["4", "17", "11", "0.75", "0.5"], ["4", "17", "11", repr(1 / 3), "0.5"],
                                                 ["0", "23", "11", "0.75", "-1.0"]]
    assert rows[1][4] == "0.0 1.0 2.0 4.0 5.0 6.0 8.0 9.0 10.0" and rows[1][5] == "3.0 7.0 11.0"
    with pytest.raises(ValueError, match="holds no number"):
        write_bop_instances(path, "frame", ["obj_000005", "obj_000011"], poses, scores)
    back = bop_scores.read_bop_results(path)           # the scorer's own reader takes the file as it is
    assert back["score"].tolist() == [0.125, 0.75, 1 / 3, 0.75] and back["obj_id"].tolist() == [5, 11, 11, 11] and back["im_id"].tolist() == [17, 17, 17, 23]
    assert np.array_equal(back["pose"][2], poses[1, 2]) and back["time"].tolist() == [0.5, 0.5, 0.5, -1.0]


class AnnotatedFrame(Annotated):
    """the stand-in with the offsets a VectorfieldDataset's batch carries"""
    offsets = IDENTITY

    def generate_dataset(self, *a, **k):
        batches, _ = super().generate_dataset(*a, **k)
        return iter([dict(b, offsets=np.array([self.offsets], np.float32)) for b in batches]), None


class CroppedFrame(AnnotatedFrame):
    offsets = [16.0, 96.0, 448.0, 448.0, 0.0, 0.0, 0.0, 1.0, 640.0, 480.0]


# ---- minimal_instances.py's columns ---------------------------------------------------------------------------------------------------------
def run_script(script, monkeypatch, tmp_path, capsys, score, pnp_switch=None, voter=None, split=None, annotated=AnnotatedFrame):  # noqa: F811
    """the script with stand-ins for everything that needs a device or a dataset -> (verifier calls, printed text, poses_est.csv bytes, run folder)"""
    from casapose_amd.pose_estimation import pose_verify as V

    verified = []

    class Voter:
        def __init__(self, name, num_classes, num_points, max_instances, **kw):
            self.last_counts = torch.zeros(1, 8, 2, dtype=torch.int32)
            self.last_counts[0, 3, 1], self.last_counts[0, 5, 0] = 77, 60
            self.last_instances = torch.zeros(1, 8, 2, 4 if kw.get("split") == "votes" else 2, dtype=torch.int32)
            self.last_kept = torch.full((1, 8, 2, 9), 0.75) if kw.get("voter") == "robust" else None
            self.last_cov = torch.ones(1, 8, 2, 9, 3) if kw.get("covariance") else None
            self.last_labels = torch.zeros(1, 480, 640, dtype=torch.uint8)

        def __call__(self, inp):
            return torch.zeros(1, 8, 2, 9, 2)

    def pnp(coords, counts, keypoints, camera_matrix, min_num, rng, **kw):
        out = np.zeros((1, 8, 2, 3, 4), np.float32)
        out[0, 3, 1], out[0, 5, 0] = np.arange(12).reshape(3, 4), 1 + np.arange(12).reshape(3, 4)
        return (out, np.zeros((1, 8, 2), np.int32)) if kw else out

    def for_dataset(dataset, path_meshes, objects, device):
        verified.append(("verifier", isinstance(dataset, Annotated), list(objects)))
        return "the verifier"

    def verify(verifier, poses, slot_map, field, keypoints3d, camera_matrix, dir_off=0, **kw):
        verified.append(("verify", verifier, tuple(np.shape(poses)), tuple(slot_map.shape), tuple(field.shape), dir_off, sorted(kw)))
        scores = np.zeros((1, 8, 2))
        scores[0, 3, 1], scores[0, 5, 0], scores[0, 0, 0] = 0.8125, 1 / 3, 0.99      # (0, 0) was not found: its score is not written
        return scores

    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    for name, value in (("CASAPOSE_INSTANCE_SCORE", score), ("CASAPOSE_INSTANCE_PNP", pnp_switch), ("CASAPOSE_INSTANCE_VOTER", voter), ("CASAPOSE_INSTANCE_SPLIT", split)):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
    for name, stand_in in (("ImageOnlyDataset", Frames), ("VectorfieldDataset", annotated), ("InstanceLSVoting", Voter), ("poses_pnp_instances", pnp),
                           ("latest_checkpoint", lambda path: None)):
        monkeypatch.setattr(script, name, stand_in)
    monkeypatch.setattr(V, "verifier_for_dataset", for_dataset)
    monkeypatch.setattr(V, "verify_instance_estimates", verify)
    monkeypatch.setattr(script.Classifiers, "get", staticmethod(lambda name: Net))
    for name, stand_in in (("is_available", lambda: True), ("set_device", lambda d: None), ("current_device", lambda: 0), ("synchronize", lambda d=None: None)):
        monkeypatch.setattr(torch.cuda, name, stand_in)
    out = str(tmp_path / ("run_%s_%s_%s_%s" % (score, pnp_switch, voter, split)))
    script.main(["-c", CFG, "--outf", out, "--datatest", str(tmp_path), "--write_poses", "1"])
    return verified, capsys.readouterr().out, open(out + "/poses_est.csv", "rb").read(), out


@pytest.mark.parametrize("others", [(None, None, None), ("weighted", "robust", "votes")])
def test_none_and_unset_are_the_same_path_and_verify_adds_the_column(script, monkeypatch, tmp_path, capsys, others):  # noqa: F811
    unset = run_script(script, monkeypatch, tmp_path, capsys, None, *others)
    none = run_script(script, monkeypatch, tmp_path, capsys, "none", *others)
    assert unset[0] == none[0] == [] and unset[2] == none[2] and LINE not in unset[1] and LINE not in none[1]     # the CSV byte for byte
    assert not os.path.exists(unset[3] + "/bop_instances.csv") and not os.path.exists(none[3] + "/bop_instances.csv")
    rows = list(csv.reader(unset[2].decode().splitlines()))
    assert rows[0] == OLD_HEADER + (["votes", "kept", "weighted"] if others[0] else [])

    calls, printed, raw, folder = run_script(script, monkeypatch, tmp_path, capsys, "verify", *others)
    assert calls[0] == ("verifier", True, NAMES) and len(calls) == 3            # one verifier, one verification per frame
    assert calls[1] == ("verify", "the verifier", (1, 8, 2, 3, 4), (1, 480, 640), (1, 480, 640, 36), 9, [])     # the network's output is the field
    assert printed.count(LINE) == 1 and printed.count("instances: up to 2 per object") == 1
    lines = [ln for ln in printed.splitlines() if ln.startswith("instances:")]
    assert lines[-1] == LINE and lines[:-1] == [ln for ln in unset[1].splitlines() if ln.startswith("instances:")]
    new_rows = list(csv.reader(raw.decode().splitlines()))
    assert new_rows[0] == rows[0] + ["score"] and len(new_rows) == len(rows)
    assert all(r[:-1] == old for r, old in zip(new_rows, rows))                  # every earlier column as it was
    by_object = {(r[0], r[1]): r[-1] for r in new_rows[1:]}
    assert by_object[("000000", NAMES[3])] == "0.8125" and by_object[("000001", NAMES[5])] == repr(1 / 3) and by_object[("000000", NAMES[0])] == "0.0"
    bop = list(csv.reader(open(folder + "/bop_instances.csv")))
    assert len(bop) == 1 + 2 * 2 and [r[:4] for r in bop[1:]] == [["0", "0", "8", "0.8125"], ["0", "0", "10", repr(1 / 3)], ["0", "1", "8", "0.8125"],
                                                                 ["0", "1", "10", repr(1 / 3)]]
    assert all(float(r[-1]) > 0 for r in bop[1:])                                # the frame's seconds


def test_the_annotated_frames_offsets_are_checked(script, monkeypatch, tmp_path, capsys):  # noqa: F811
    """the camera matrix is the first annotated frame's: offsets that are not the identity, or none at all, are refused by name before a
    verifier is built; without the switch neither matters"""
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SCORE=verify needs frames that reach the network as they are"):
        run_script(script, monkeypatch, tmp_path, capsys, "verify", annotated=CroppedFrame)
    with pytest.raises(ValueError, match="CASAPOSE_INSTANCE_SCORE=verify needs the offsets of the annotated frame"):
        run_script(script, monkeypatch, tmp_path, capsys, "verify", annotated=Annotated)
    assert run_script(script, monkeypatch, tmp_path, capsys, None, annotated=CroppedFrame)[0] == []
    assert run_script(script, monkeypatch, tmp_path, capsys, None, annotated=Annotated)[0] == []
