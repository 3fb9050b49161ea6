"""The mask renderer on the GPU: `cp_render_masks_u8` (csrc/masks.hip) against its host twin on the cases of tests/test_masks_twin_host.py, and
`MaskRenderer.render` / the BOP converter's `renderer="device"` on top of it.

Kernel and twin run the same header (csrc/mask_math.h) on the same inputs -- exact int64 coverage, fp64 depths without FMA contraction rounded once
to fp32, integer minima and sums -- so labels and records are compared byte for byte, and two launches give the same bytes.

Besides the cases of the host test: one 480 x 640 frame with 8 instances of a subdivision-5 icosphere (20 480 triangles each, LM's scale; small
triangles on the per-lane path, 80 blocks per instance), compared with the twin."""
import json
import os

import numpy as np
import pytest

import raster_reference as RR
import test_masks_twin_host as T
from casapose_amd.data_handler import bop_converter as BC

pytestmark = pytest.mark.gpu


def on_device(device, meshes, frames, H, W, near, far, offset, workspace_cap=None):
    return T.renderer_for(meshes, device).render(frames, H, W, near, far, offset, workspace_cap)


@pytest.mark.parametrize("offset", T.OFFSETS)
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_kernel_matches_its_host_twin(device, name, offset):
    (meshes, frames, H, W, near, far), labels, records, _, _ = T.rendered(name, offset)
    T.check_case_content(name, labels, records)
    got_labels, got_records = on_device(device, meshes, frames, H, W, near, far, offset)
    assert got_labels.dtype == np.uint8 and got_records.dtype == np.int32
    assert np.array_equal(got_records, records), np.argwhere(got_records != records)[:5]
    assert np.array_equal(got_labels, labels), np.argwhere(got_labels != labels)[:5]
    again_labels, again_records = on_device(device, meshes, frames, H, W, near, far, offset)   # fresh buffers, the same bytes
    assert again_labels.tobytes() == got_labels.tobytes() and again_records.tobytes() == got_records.tobytes()


def lm_scale_frame():
    cam = (572.4114, 573.57043, 325.2611, 242.04899)
    v, f = RR.icosphere(5)
    meshes = [((v * np.array([60.0, 45.0, 80.0])).astype(np.float32), f)]
    rng = np.random.default_rng(8)
    inst = []
    for k in range(8):
        R = RR.rotation(rng.normal(size=3), rng.uniform(0, 3))
        inst.append((0, 10 + 30 * k, RR.pose_at(cam, 120.0 + 60.0 * k + rng.uniform(-10, 10), 240.0 + rng.uniform(-120, 120), 500.0 + 90.0 * k, R)))
    return meshes, [dict(cam=cam, instances=inst)], 480, 640, 100.0, 2000.0


def test_lm_scale_frame_matches_the_twin(device):
    meshes, frames, H, W, near, far = lm_scale_frame()
    assert len(meshes[0][1]) == 20480
    labels, records = T.renderer_for(meshes).render_host(frames, H, W, near, far, 0.5)
    assert (records[0, :, 0] > 2000).all() and (records[0, :, 0] > records[0, :, 1]).any() and (labels == 0).sum() > 100000   # overlapping neighbours
    got_labels, got_records = on_device(device, meshes, frames, H, W, near, far, 0.5)
    assert np.array_equal(got_records, records) and np.array_equal(got_labels, labels)
    again_labels, again_records = on_device(device, meshes, frames, H, W, near, far, 0.5)
    assert again_labels.tobytes() == got_labels.tobytes() and again_records.tobytes() == got_records.tobytes()


def test_chunked_render_equals_one_call(device):
    """seven frames under a workspace cap that holds three of them: three chunks (3 + 3 + 1), the renderer one chunk ahead of the consumer"""
    meshes, frames, H, W, near, far = T.three_ellipsoids()
    inst = frames[0]["instances"]
    many = [dict(cam=(100.0 + k, 101.0, 31.7 - k, 23.4 + 0.5 * k), instances=list(inst[:k % 4])) for k in range(7)]
    r = T.renderer_for(meshes, device)
    one = r.chunk_frames(1, 3, H, W)   # frames per launch cannot be asked for directly: derive the cap from one frame's bytes
    cap = 3 * int(r.lib.cp_render_masks_workspace_bytes(1, 3, H, W)) + 5
    assert one == 1 and r.chunk_frames(7, 3, H, W, cap) == 3
    chunks = list(r.render_chunks(many, H, W, near, far, 0.5, cap))
    assert [lo for lo, _, _ in chunks] == [0, 3, 6] and [len(l) for _, l, _ in chunks] == [3, 3, 1]
    capped = r.render(many, H, W, near, far, 0.5, cap)
    whole = r.render(many, H, W, near, far, 0.5)
    twin = r.render_host(many, H, W, near, far, 0.5)
    for a, b, c in zip(capped, whole, twin):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert (whole[0][0] == 0).all() and (whole[0][3] > 0).sum() > 300
    with pytest.raises(ValueError, match="workspace cap"):
        r.render(many, H, W, near, far, 0.5, 100)


def test_converted_tree_runs_through_the_drivers(device, tmp_path):
    """A BOP-layout folder with config_8.ini's eight objects at 480 x 640 (no scene_gt_info.json, no mask_visib/), converted with the masks and
    the counts rendered on the device, evaluates through test_casapose.py and trains a step through train_casapose.py, both unmodified.  With
    random weights the numbers mean nothing; the runs must complete, with finite losses, and write their reports."""
    import csv

    from PIL import Image

    import test_casapose
    import train_casapose

    cam = (572.4114, 573.57043, 325.2611, 242.04899)
    ids = (1, 5, 6, 8, 9, 10, 11, 12)
    bop, scene = tmp_path / "bop", tmp_path / "bop" / "test" / "000001"
    os.makedirs(bop / "models_eval")
    os.makedirs(scene / "rgb")
    rng = np.random.default_rng(4)
    for obj in ids:
        axes = rng.uniform(35.0, 70.0, 3)
        v, f = T.ellipsoid(2, axes)
        T.write_ply(bop / "models_eval" / ("obj_%06d.ply" % obj), v, f)
        T.write_ply(bop / "models_eval" / ("obj_%06d_keypoints.ply" % obj), T.keypoints_of(axes))
    json.dump({str(o): {"diameter": 140.0} for o in ids}, open(bop / "models_eval" / "models_info.json", "w"))
    gt = {}
    for i in range(2):
        gt[str(i)] = []
        for k, obj in enumerate(ids):
            P = RR.pose_at(cam, 70.0 + 70.0 * k + rng.uniform(-20, 20), 240.0 + rng.uniform(-150, 150), rng.uniform(650.0, 1100.0),
                           RR.rotation(rng.normal(size=3), rng.uniform(0, 3)))
            gt[str(i)].append({"cam_R_m2c": P[:, :3].reshape(-1).tolist(), "cam_t_m2c": P[:, 3].tolist(), "obj_id": obj})
        Image.fromarray(rng.integers(0, 255, (480, 640, 3), dtype=np.uint8)).save(scene / "rgb" / ("%06d.png" % i))
    json.dump(gt, open(scene / "scene_gt.json", "w"))
    json.dump({str(i): {"cam_K": [cam[0], 0.0, cam[2], 0.0, cam[1], cam[3], 0.0, 0.0, 1.0], "depth_scale": 1.0} for i in range(2)},
              open(scene / "scene_camera.json", "w"))
    settings = dict(near=100, far=2000, width=640, height=480, filetype_in="png", mask="render", copy_meshes=True, draw_debug_image=False,
                    gt_info="render")
    BC.generate_data(str(bop), str(tmp_path / "conv"), settings, model_folder="models_eval", image_folder="test")
    first = json.load(open(tmp_path / "conv" / "test" / "000001" / "rgb" / "000000.json"))
    assert len(first["objects"]) == 8 and all(o["px_count_all"] > 200 for o in first["objects"])
    data, meshes, cfg = str(tmp_path / "conv" / "test"), str(tmp_path / "conv" / "models"), os.path.join(T.ROOT, "config", "config_8.ini")
    out = str(tmp_path / "run")
    res = test_casapose.main(["-c", cfg, "--outf", out, "--manualseed", "7", "--datatest", data, "--datameshes", meshes, "--net", "", "--pretrained", "0"])
    assert len(list(csv.reader(open(out + "/loss_test_eval.csv")))) == 3 and np.all(np.isfinite(res["loss"]))
    train_casapose.main(["-c", cfg, "--outf", str(tmp_path / "train"), "--manualseed", "7", "--workers", "0", "--data", data, "--datatest", "",
                         "--datameshes", meshes, "--epochs", "1", "--batchsize", "2", "--imagesize", "128", "160", "--saveinterval", "1",
                         "--loginterval", "1"])
    rows = list(csv.reader(open(str(tmp_path / "train") + "/loss_train.csv")))
    assert len(rows) == 2 and np.all(np.isfinite([float(x) for x in rows[1][2:7]]))


def test_converter_on_the_device_writes_what_the_host_writes(device, tmp_path):
    T.write_bop_tree(tmp_path / "bop")
    for which in ("host", "device"):
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / which), T.settings_for(renderer=which), model_folder="models", model_folder_out="models",
                         image_folder="test")
    names = sorted(os.listdir(tmp_path / "host" / "test" / "000002" / "rgb"))
    assert names == sorted(os.listdir(tmp_path / "device" / "test" / "000002" / "rgb")) and len(names) == 8
    for n in names:
        a = open(tmp_path / "host" / "test" / "000002" / "rgb" / n, "rb").read()
        b = open(tmp_path / "device" / "test" / "000002" / "rgb" / n, "rb").read()
        assert a == b, n
    assert json.load(open(tmp_path / "device" / "test" / "000002" / "rgb" / "000000.json"))["objects"][0]["px_count_all"] > 100
