"""The shaded mesh renderer on the GPU: `cp_render_shaded_f32` (csrc/shade.hip) against its host twin on the cases of
tests/test_shade_twin_host.py, MeshSceneDataset's device path against its twin path, and train_casapose.py on a `meshes:` source.

Kernel and twin run the same header (csrc/shade_math.h) on the same inputs -- exact int64 coverage, fp64 without FMA contraction, integer minima
-- so keys, labels, depths and drop counts are compared byte for byte.  The image is fp64 arithmetic rounded once to fp32: 2.4e-7 (two fp32
ulps of 1) bounds it, with equality expected when the background is supplied (the procedural background calls sin / cos, the device's against
the host's).  With noise the Philox words are the same and the device's logf / sinf / cosf meet the host's: 1e-6, the bound of
tests/test_gpu_scenes.py.

Besides the cases of the host test: one frame of 96 rows with 8 instances of a subdivision-3 icosphere (1280 faces: five 256-triangle chunks per
instance) at widths 128, 37 (the element-wise store path) and 72."""
import csv
import os

import numpy as np
import pytest
import torch

import raster_reference as RR
import test_masks_twin_host as TM
import test_shade_twin_host as TS
from casapose_amd.data_handler.mesh_scene import MeshSceneDataset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "config_8.ini")
NOISY_TOL = 1e-6


def to_host(out):
    host = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    host["keys"] = host["keys"].view(np.uint64)
    return host


def compare(got, want, what, noisy=False):
    assert np.array_equal(got["keys"], want["keys"]), (what, np.argwhere(got["keys"] != want["keys"])[:5])
    assert np.array_equal(got["label"], want["label"]) and np.array_equal(got["dropped"], want["dropped"]), what
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), what
    err = np.abs(got["img"].astype(np.float64) - want["img"].astype(np.float64)).max()
    print("%s: kernel img differs from the twin by at most %.3g%s" % (what, err, " (with noise)" if noisy else ""))
    assert err <= (NOISY_TOL if noisy else TS.TOL), (what, err)
    return err


def icospheres(W):
    """96 x W: 8 instances of one subdivision-3 icosphere spread over the frame, neighbours overlapping"""
    cam = (150.0, 150.0, W / 2.0 + 0.3, 47.6)
    v, f = RR.icosphere(3)
    meshes = [((v * np.array([40.0, 30.0, 50.0])).astype(np.float32), f)]
    rng = np.random.default_rng(8)
    inst = [(0, 10 + 30 * k, RR.pose_at(cam, W * (k + 0.5) / 8.0 + rng.uniform(-3, 3), 48.0 + rng.uniform(-30, 30), 500.0 + 40.0 * k,
                                        RR.rotation(rng.normal(size=3), rng.uniform(0, 3)))) for k in range(8)]
    return meshes, [dict(cam=cam, instances=inst)], 96, W, 100.0, 2000.0


@pytest.mark.parametrize("offset", TM.OFFSETS)
@pytest.mark.parametrize("name", TS.SCENES)
def test_kernel_matches_its_host_twin(device, name, offset):
    (meshes, frames, H, W, near, far), want, _ = TS.shaded(name, offset)
    colors, flat, lights, bg = TS.vertex_colors(meshes), TS.flat_colors(meshes), TS.lights_for(len(frames)), TS.background_for(len(frames), H, W)
    r = TS.renderer_for(meshes, colors, flat, device)
    got = to_host(r.render(frames, lights, H, W, near, far, offset, background=bg))
    compare(got, want, "%s at offset %.1f" % (name, offset))   # a supplied background: equality is expected, the bound is asserted
    again = to_host(r.render(frames, lights, H, W, near, far, offset, background=bg))   # fresh buffers, the same bytes
    assert all(again[k].tobytes() == got[k].tobytes() for k in ("img", "label", "depth", "dropped", "keys"))


@pytest.mark.parametrize("W", (128, 37, 72))
def test_icospheres_match_the_twin_with_and_without_noise(device, W):
    meshes, frames, H, W, near, far = icospheres(W)
    assert len(meshes[0][1]) == 1280
    colors, flat, lights = TS.vertex_colors(meshes), TS.flat_colors(meshes), TS.lights_for(1)
    host, dev = TS.renderer_for(meshes, colors, flat), TS.renderer_for(meshes, colors, flat, device)
    for noise in (False, True):
        for colours in (True, False):   # the procedural background throughout; vertex colours, then the flat colour (a null pointer)
            want = host.render_host(frames, lights, H, W, near, far, 0.5, noise=noise, colors=colours)
            got = to_host(dev.render(frames, lights, H, W, near, far, 0.5, noise=noise, colors=colours))
            compare(got, want, "8 icospheres at W = %d, %s" % (W, "vertex colours" if colours else "flat colour"), noise)
    assert len(np.unique(want["label"])) >= 8 and (want["label"] == 0).sum() > 0.1 * H * W
    nodepth = to_host(dev.render(frames, lights, H, W, near, far, 0.5, noise=True, colors=False, depth=False))   # a null depth pointer
    assert nodepth["depth"] is None and nodepth["img"].tobytes() == got["img"].tobytes() and nodepth["label"].tobytes() == got["label"].tobytes()


def test_a_batch_equals_its_frames_and_the_mask_renderers_label(device):
    meshes, frames, H, W, near, far = TM.CASES["batch_of_three"]()
    colors, flat, lights, bg = TS.vertex_colors(meshes), TS.flat_colors(meshes), TS.lights_for(3), TS.background_for(3, H, W)
    r = TS.renderer_for(meshes, colors, flat, device)
    whole = to_host(r.render(frames, lights, H, W, near, far, 0.5, background=bg, noise=True))
    for f in range(3):
        one = to_host(r.render(frames[f:f + 1], lights[f:f + 1], H, W, near, far, 0.5, background=bg[f:f + 1], noise=True, instances_max=3))
        assert all(one[k][0].tobytes() == whole[k][f].tobytes() for k in ("img", "label", "depth", "dropped", "keys")), f
    labels, _ = TM.renderer_for(meshes, device).render(frames, H, W, near, far, 0.5)
    assert np.array_equal(whole["label"], labels)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return TS.write_mesh_folder(tmp_path_factory.mktemp("meshes") / "models")


@pytest.mark.parametrize("instances", (1, 3))
def test_dataset_on_the_device_equals_its_twin(device, folder, instances):
    ds = MeshSceneDataset(folder, 2, TS.SIZE, length=8, seed=4, instances=instances)
    want, got = ds.batch(0, 4), ds.batch(0, 4, device=device)
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        if k != "img":
            assert np.array_equal(got[k].cpu().numpy(), want[k].numpy()), k
    assert got["img"].is_cuda and got["target_seg"].is_cuda and got["filtered_seg"].is_cuda
    err = np.abs(got["img"].cpu().numpy().astype(np.float64) - want["img"].numpy()).max()
    print("dataset, %d instances: device img differs from the twin's by at most %.3g (with noise)" % (instances, err))
    assert err <= NOISY_TOL


def test_an_earlier_batch_does_not_change(device, folder):
    ds = MeshSceneDataset(folder, 2, TS.SIZE, length=8, seed=4, instances=2)
    it, n = ds.generate_dataset(2, 1, 2, device=device)
    assert n == 4
    first = next(it)
    kept = {k: first[k].clone() for k in first}
    second, third = next(it), next(it)
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], kept[k]) for k in first)
    assert not torch.equal(first["img"], second["img"]) and first["img"].data_ptr() not in (second["img"].data_ptr(), third["img"].data_ptr())
    again = ds.batch(0, 2, device=device)
    assert all(torch.equal(first[k], again[k]) for k in first)


@pytest.mark.parametrize("train_instances", (None, 2))
def test_scripts_run_on_a_mesh_folder(device, folder, tmp_path, monkeypatch, train_instances):
    """train_casapose.py then test_casapose.py on `meshes:`, at the smallest size tests/test_gpu_scripts.py uses for `synthetic`; the first run
    renders with the host twin, the one with CASAPOSE_TRAIN_INSTANCES=2 on the device.  test_casapose.py's folder branch hands the spec to
    VectorfieldDataset, which serves it from a MeshSceneDataset."""
    import test_casapose
    import train_casapose

    if train_instances:
        monkeypatch.setenv("CASAPOSE_TRAIN_INSTANCES", str(train_instances))
        monkeypatch.setenv("CASAPOSE_DEVICE_SCENES", "1")
    out = str(tmp_path / "run")
    common = ["-c", CFG, "--outf", out, "--manualseed", "7", "--workers", "0", "--object", "obj_000001,obj_000004"]
    train_casapose.main(common + ["--data", "meshes:%s:8" % folder, "--datatest", "meshes:%s:4" % folder, "--epochs", "1", "--batchsize", "4",
                                  "--imagesize", "128", "160", "--saveinterval", "1", "--loginterval", "1", "--validationinterval", "1"]
                        + (["--estimate_coords", "0"] if train_instances else []))   # the keypoint loss is per object: training.py refuses it with instances
    rows = list(csv.reader(open(out + "/loss_train.csv")))
    assert len(rows) == 1 + 2 and np.isfinite([[float(v) for v in r[2:7]] for r in rows[1:]]).all()
    assert os.path.exists(out + "/frozen_model/result_w.h5") and len(list(csv.reader(open(out + "/test_summary.csv")))) == 2
    summary = list(csv.reader(open(out + "/test_summary.csv")))
    assert len(summary[0]) == len(summary[1]) == 7 + 2 + 2 and np.isfinite([float(v) for v in summary[1]]).all()   # a validation epoch with its pose columns
    monkeypatch.delenv("CASAPOSE_TRAIN_INSTANCES", raising=False)
    res = test_casapose.main(common + ["--datatest", "meshes:%s:4" % folder, "--load_h5_weights", "1", "--imagesize_test", "128", "160"])
    ev = list(csv.reader(open(out + "/test_summary_eval.csv")))
    assert len(ev) == 2 and len(ev[1]) == 5 + 3 + 3 and len(list(csv.reader(open(out + "/loss_test_eval.csv")))) == 1 + 4
    assert np.all(np.isfinite(res["loss"])) and res["valid_3d"].shape == (2,)


def test_the_triangle_tie_on_the_device(device):
    """the roof of tests/test_shade_twin_host.py, the scene built so that the winner would depend on the order of arrival if the key did not decide
    it: kernel = twin byte for byte in either face order, and the ridge carries triangle 0"""
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [64.0]]], axis=1)
    frames = [dict(cam=TS.KA_CAM, instances=[(0, 4, pose)])]
    light = TS.frame_record((0.6, 0.0, -0.8), 0.3, 0.6, 1)[None]
    for swap in (False, True):
        want = TS.renderer_for([TS.roof(swap)], None, [(0.4, 0.6, 0.8)]).render_host(frames, light, 64, 64, 1.0, 1000.0, 0.5)
        got = to_host(TS.renderer_for([TS.roof(swap)], None, [(0.4, 0.6, 0.8)], device).render(frames, light, 64, 64, 1.0, 1000.0, 0.5))
        compare(got, want, "roof, faces %s" % ("swapped" if swap else "in order"))
        on = want["label"] > 0   # the roof itself: no library call enters its pixels
        assert np.array_equal(got["img"][on], want["img"][on]) and ((got["keys"][0, 22:42, 32] & np.uint64(0xFFFFFF)) == 0).all()
