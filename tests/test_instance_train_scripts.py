"""CASAPOSE_TRAIN_INSTANCES in train_casapose.py: how the variable is read (without a GPU), and on the GPU one epoch of
`--data synthetic:8 --batchsize 2` with CASAPOSE_TRAIN_INSTANCES=2, which must log finite losses."""
import csv
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "config_8.ini")
ENV = "CASAPOSE_TRAIN_INSTANCES"


def test_the_variable_is_parsed_as_specified(monkeypatch):
    import train_casapose

    read = train_casapose.train_instances_from_environment
    monkeypatch.delenv(ENV, raising=False)
    assert read("synthetic:8") == 1 and read("/some/folder") == 1
    for raw, want in (("2", 2), ("16", 16), (" 4 ", 4)):
        monkeypatch.setenv(ENV, raw)
        assert read("synthetic:8") == want and read("synthetic") == want
    for raw in ("1", "17", "0", "-3", "", "two", "2.0"):
        monkeypatch.setenv(ENV, raw)
        with pytest.raises(SystemExit, match=ENV):
            read("synthetic:8")
    monkeypatch.setenv(ENV, "2")
    with pytest.raises(SystemExit, match=ENV + ".*synthetic"):
        read("/some/folder")


def test_the_switch_reaches_the_training_source_alone(monkeypatch):
    """--data gets the instance axis, --datatest keeps one instance per object; unset, both are what they were"""
    from types import SimpleNamespace

    import train_casapose

    opt = SimpleNamespace(no_points=9)
    monkeypatch.setenv(ENV, "3")
    train = train_casapose.open_dataset("synthetic:8", opt, 2, (48, 64), True, 1)
    test = train_casapose.open_dataset("synthetic:4", opt, 2, (48, 64), False, 2)
    assert train.instances == 3 and test.instances == 1 and len(train) == 8
    assert tuple(train.batch(0, 2)["target_vert"].shape) == (2, 2, 3, 9, 2) and tuple(test.batch(0, 2)["target_vert"].shape) == (2, 2, 1, 9, 2)
    monkeypatch.delenv(ENV)
    assert train_casapose.open_dataset("synthetic:8", opt, 2, (48, 64), True, 1).instances == 1


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ("1", "17"))
def test_the_script_exits_with_the_variables_name(device, tmp_path, monkeypatch, bad):
    import train_casapose

    monkeypatch.setenv(ENV, bad)
    with pytest.raises(SystemExit, match=ENV):
        train_casapose.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--workers", "0", "--data", "synthetic:8", "--datatest", "", "--epochs", "1",
                             "--batchsize", "2", "--imagesize", "128", "160", "--estimate_coords", "0"])


@pytest.mark.gpu
def test_a_folder_source_is_refused(device, tmp_path, monkeypatch):
    import train_casapose

    monkeypatch.setenv(ENV, "2")
    with pytest.raises(SystemExit, match=ENV):
        train_casapose.main(["-c", CFG, "--outf", str(tmp_path / "run"), "--workers", "0", "--data", str(tmp_path), "--datatest", "", "--epochs", "1",
                             "--batchsize", "2", "--imagesize", "128", "160", "--estimate_coords", "0"])


@pytest.mark.gpu
def test_one_epoch_on_two_instances_logs_finite_losses(device, tmp_path, monkeypatch):
    import train_casapose

    monkeypatch.setenv(ENV, "2")
    monkeypatch.delenv("CASAPOSE_TRAIN_INSTANCE_RULE", raising=False)
    out = str(tmp_path / "run")
    train_casapose.main(["-c", CFG, "--outf", out, "--manualseed", "7", "--workers", "0", "--data", "synthetic:8", "--datatest", "", "--epochs", "1",
                         "--batchsize", "2", "--imagesize", "128", "160", "--loginterval", "1", "--estimate_coords", "0"])
    rows = list(csv.reader(open(out + "/loss_train.csv")))
    assert rows[0][:7] == ["epoch", "batchid", "loss", "mask_loss", "vertex_loss", "proxy_loss", "keypoint_loss"] and len(rows) == 1 + 4
    vals = np.array([[float(v) for v in r[2:7]] for r in rows[1:]])
    assert np.isfinite(vals).all() and (vals[:, 1:4] > 0).all()
