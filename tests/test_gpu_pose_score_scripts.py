"""The verified score through the scripts on the GPU: test_casapose.py under CASAPOSE_POSE_SCORE=1 and util_scripts/minimal_instances.py under
CASAPOSE_INSTANCE_SCORE=verify, on a synthetic folder in the reference's on-disk format.  With random weights the scores say nothing about the
poses; the runs must complete, give scores in [0, 1] and leave every other column as it was."""
import csv
import os

import numpy as np
import pytest
from scipy.spatial import ConvexHull

from test_instances_scripts import CFG, NAMES, script  # noqa: F401

pytestmark = pytest.mark.gpu


def folder(tmp_path, frames, seed):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.data_handler.vectorfield_dataset import write_ndds_scene

    data, models = str(tmp_path / "data"), str(tmp_path / "models")
    scene = SyntheticSceneDataset(8, (480, 640), length=frames, seed=seed)
    write_ndds_scene(data, models, scene, frames, NAMES)
    for o, name in enumerate(NAMES):      # the exported models hold vertices only; the verifier renders, so give them their convex hull's faces
        v = np.asarray(scene.mesh_vertex_array[o], np.float64)
        faces = ConvexHull(v).simplices
        with open(os.path.join(models, name, name + ".ply"), "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
                    "property list uchar int vertex_indices\nend_header\n" % (len(v), len(faces)))
            f.write("".join("%r %r %r\n" % tuple(float(c) for c in p) for p in v) + "".join("3 %d %d %d\n" % tuple(int(i) for i in t) for t in faces))
    return data, models


def test_test_script_verifies_its_poses_under_the_switch(device, tmp_path, monkeypatch, capsys):
    """test_casapose.py has no line for the switch: training.test_step reads it, verifies the final poses of every batch inside the measured
    time and keeps the scores on the one verifier of the run; the script's own files are what they were.  write_poses(scores=) writes them."""
    import test_casapose
    from casapose_amd.pose_estimation import pose_verify as V
    from casapose_amd.utils.io_utils import write_poses

    data, models = folder(tmp_path, 2, 3)
    args = ["-c", CFG, "--manualseed", "7", "--datatest", data, "--datameshes", models, "--net", "", "--pretrained", "0", "--write_poses", "1"]
    monkeypatch.delenv("CASAPOSE_POSE_SCORE", raising=False)
    test_casapose.main(args + ["--outf", str(tmp_path / "plain")])
    monkeypatch.setenv("CASAPOSE_POSE_SCORE", "1")
    monkeypatch.setattr(V.pose_score_enabled, "said", False)
    monkeypatch.setattr(V, "_verifiers", {})
    capsys.readouterr()
    test_casapose.main(args + ["--outf", str(tmp_path / "scored")])
    assert capsys.readouterr().out.count("score: verified poses") == 1
    plain = list(csv.reader(open(str(tmp_path / "plain") + "/poses_out/bop_evaluation.csv")))
    scored = list(csv.reader(open(str(tmp_path / "scored") + "/poses_out/bop_evaluation.csv")))
    assert len(plain) == len(scored) > 1 and [r[:6] for r in plain] == [r[:6] for r in scored]       # the verification changes no pose
    assert len(V._verifiers) == 1                                                                  # one verifier, built once
    verifier = list(V._verifiers.values())[0]
    scores, counts = verifier.last_scores, verifier.last_counts                                      # of the last batch
    assert scores.shape == (1, 8) and counts.shape == (1, 8, 8) and (counts[..., 0] > 0).any()       # something was rendered
    assert ((scores >= 0.0) & (scores <= 1.0)).all() and (scores[counts[..., 0] == 0] == 0.0).all()
    poses = np.zeros((8, 3, 4), np.float32)
    poses[counts[0, :, 0] > 0] = np.eye(3, 4, dtype=np.float32)                                      # stand-ins for the estimates that were found
    again = str(tmp_path / "again") + "/"
    write_poses(np.ones((8, 1, 3, 4), np.float32), poses, NAMES, ["000000_rgb_000001"], again, 0.5, scores=scores[0])
    rows = list(csv.reader(open(again + "bop_evaluation.csv")))[1:]
    assert [r[3] for r in rows] == [repr(float(s)) if poses[o].any() else "0.0" for o, s in enumerate(scores[0])]


def test_instance_script_writes_verified_scores(script, device, monkeypatch, tmp_path, capsys):  # noqa: F811
    from casapose_amd.pose_estimation import bop_scores
    from casapose_amd.pose_models.tfkeras import Classifiers

    frames = 2
    data, models = folder(tmp_path, frames, 5)
    out = str(tmp_path / "run")
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=9, input_shape=(480, 640, 3), weights=None, device=device, seed=21)
    os.makedirs(out + "/frozen_model")
    net.save_weights(out + "/frozen_model/result_w.h5")
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    monkeypatch.setenv("CASAPOSE_INSTANCE_SCORE", "verify")
    res = script.main(["-c", CFG, "--outf", out, "--manualseed", "7", "--datatest", data, "--datameshes", models, "--load_h5_weights", "1",
                       "--object", ",".join(NAMES), "--write_poses", "1", "--min_object_size_test", "20"])
    assert capsys.readouterr().out.count("instances: verified scores") == 1
    rows = list(csv.reader(open(out + "/poses_est.csv")))
    assert rows[0][-3:] == ["instance", "pixels", "score"] and all(len(r) == 17 for r in rows)
    found = [r for r in rows[1:] if int(r[15]) > 0]
    assert found and all(0.0 <= float(r[16]) <= 1.0 for r in found) and all(r[16] == "0.0" for r in rows[1:] if int(r[15]) == 0)
    bop = bop_scores.read_bop_results(out + "/bop_instances.csv")
    assert len(bop["score"]) == len(found) == sum(int(res["poses"][n][o, r].any()) for n in res["poses"] for o in range(8) for r in range(2))
    assert bop["score"].tolist() == [float(r[16]) for r in found] and set(bop["im_id"].tolist()) <= set(range(frames)) and (bop["scene_id"] == 0).all()
    assert (bop["time"] > 0).all() and np.isin(bop["obj_id"], [int(n[4:]) for n in NAMES]).all()
