"""util_scripts/test_instances.py: on the GPU the two files of a run on the built-in scenes with an untrained network, and the two refusals
(no CASAPOSE_MAX_INSTANCES; a folder as the source), which name their reason."""
import csv
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "config_8.ini")
NAMES = ["obj_%06d" % i for i in range(1, 9)]


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("test_instances_script", os.path.join(ROOT, "util_scripts", "test_instances.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_a_run_on_the_synthetic_scenes_writes_both_files(script, device, monkeypatch, tmp_path, capsys):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_estimation.instance_evaluation import SUMMARY_COLUMNS

    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    for name in ("CASAPOSE_INSTANCE_SPLIT", "CASAPOSE_INSTANCE_VOTER", "CASAPOSE_INSTANCE_PNP", "CASAPOSE_DEVICE_PNP"):
        monkeypatch.delenv(name, raising=False)
    out = str(tmp_path / "run")
    res = script.main(["-c", CFG, "--outf", out, "--evalf", out + "/eval", "--manualseed", "7", "--datatest", "synthetic:4", "--imagesize_test", "128", "160",
                       "--object", ",".join(NAMES), "--min_object_size_test", "20", "--net", ""])
    ds = SyntheticSceneDataset(8, (128, 160), 9, length=4, seed=8, random_crop=False, instances=2)
    truth = sum(int(ds.batch(i, 1)["instance_count"].sum()) for i in range(4))
    said = capsys.readouterr().out
    assert "instances: up to 2 per object" in said and "recall ADD(-S)" in said and "precision ADD(-S)" in said
    rows = list(csv.reader(open(out + "/eval/instance_evaluation.csv")))
    assert rows[0] == ["object"] + list(SUMMARY_COLUMNS) and [r[0] for r in rows[1:]] == NAMES + ["all"]
    assert int(rows[-1][1]) == truth == sum(int(r[1]) for r in rows[1:-1]) == res["summary"]["all"]["gt"]
    matches = list(csv.reader(open(out + "/eval/instance_matches.csv")))
    assert matches[0] == ["image", "object", "instance", "slot", "err_2d", "err_3d", "valid_3d", "valid_2d"] and len(matches) - 1 == truth
    assert res["tallies"].shape == (4, 8, 5) and res["gt_rec"].shape == (4, 8, 2, 5)
    assert int(rows[-1][3]) == sum(1 for m in matches[1:] if int(m[3]) >= 0)          # matched
    assert np.array_equal(res["tallies"][..., 0], np.stack([ds.batch(i, 1)["instance_count"][0].numpy() for i in range(4)]))
    print("untrained network, synthetic:4 at 128 x 160, R = 2: %s" % res["summary"]["all"])


def test_without_the_variable_it_exits_naming_it(script, monkeypatch, tmp_path):
    monkeypatch.delenv("CASAPOSE_MAX_INSTANCES", raising=False)
    with pytest.raises(SystemExit, match="CASAPOSE_MAX_INSTANCES"):
        script.main(["-c", CFG, "--outf", str(tmp_path), "--datatest", "synthetic:4"])
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "1")
    with pytest.raises(SystemExit, match="CASAPOSE_MAX_INSTANCES"):
        script.main(["-c", CFG, "--outf", str(tmp_path), "--datatest", "synthetic:4"])
    assert not os.path.exists(str(tmp_path / "instance_evaluation.csv"))


def test_with_a_folder_source_it_exits_naming_the_source(script, monkeypatch, tmp_path):
    monkeypatch.setenv("CASAPOSE_MAX_INSTANCES", "2")
    with pytest.raises(SystemExit, match="folder reader has no instance axis"):
        script.main(["-c", CFG, "--outf", str(tmp_path), "--datatest", str(tmp_path)])
    with pytest.raises(SystemExit, match=str(tmp_path).replace("\\", "/")):
        script.main(["-c", CFG, "--outf", str(tmp_path), "--datatest", str(tmp_path)])
