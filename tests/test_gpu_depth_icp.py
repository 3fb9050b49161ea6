"""cp_depth_icp_step_f64 (csrc/depth_icp.hip), DeviceDepthRefiner and util_scripts/refine_poses.py on the GPU.

The device and the host twin compile one header (csrc/icp_math.h: fp64, no contraction, a fixed order of summation), and the renderer's device
and host planes are the same bytes (tests/test_gpu_masks.py), so every comparison here is bit for bit: one step on every case for three
splits and two workspace fills, the whole loop, and the loop cut into chunks.  The twin itself is held against the NumPy restatement on the
CPU (tests/test_icp_twin_host.py).  No test here hands the kernel an index out of range: refusals are the twin's and the self-test's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import icp_cases as IC
import icp_reference as IR
import test_icp_twin_host as TH
import vsd_cases as VC
import vsd_reference as VR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_host = {}


def host_step(name, tile):
    if name not in _host:
        _host[name] = TH.run_step(TH.arrays_of(name, tile))
    return _host[name]


# ---- 1. one step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TH.CASES) + ["crafted"])
def test_one_step_is_the_host_twins_bytes(hip_lib, device, name):
    tile = hip_lib.cp_depth_icp_tile()
    a = TH.arrays_of(name, tile)
    want, tiles = host_step(name, tile), TH.tiles_of(a, tile)
    assert min(tiles) >= 0                                                  # nothing out of range reaches the kernel
    for split, fill in ((1, 0xFF), (3, 0xA5), (8, 0xFF)):
        TH.same_bytes(TH.run_step(a, device, split=split, fill=fill), want, tiles, "%s, split %d" % (name, split))
    evaluated = TH.run_step(a, device, update=0, split=3)
    assert evaluated["poses"].tobytes() == a["poses"].tobytes() and evaluated["stats"].tobytes() == want["stats"].tobytes()
    assert evaluated["status"].tobytes() == want["status"].tobytes()


def test_two_calls_in_a_row(hip_lib, device):
    """the second call starts from the first one's poses and the same planes, on the device as on the host"""
    tile = hip_lib.cp_depth_icp_tile()
    a = TH.arrays_of("block 37 x 50", tile)
    TH.same_bytes(TH.run_step(a, device, split=3, calls=2), TH.run_step(a, calls=2), TH.tiles_of(a, tile), "two calls")


def test_a_wave_takes_a_second_tile_beside_an_empty_and_a_refused_job(hip_lib, device):
    """72 x 96 under a full-frame box: 70 x 94 = 6580 pixels, seven tiles of 1024 with the last one part full -- more than the four waves of
    split 1, so three waves take a second tile.  In the same call an empty record and a job refused for its gate (its indices are in range):
    no tiles, so not a word of their records is written, and a word read for them would be the fill's NaN in their stats"""
    tile = hip_lib.cp_depth_icp_tile()
    H, W = 72, 96
    a = IC.crafted_step(H, W, [(0, 0, W - 1, H - 1), (-1, -1, -1, -1), (0, 0, W - 1, H - 1)], 11)
    a.update(H=H, W=W, gates=np.array([40.0, 40.0, 0.0]))
    tiles = TH.tiles_of(a, tile)
    assert tiles == [-(-70 * 94 // tile), 0, -1] and tiles[0] > 4 and 70 * 94 % tile != 0
    want = TH.run_step(a)
    assert want["status"].tolist() == [0, 1, 3] and (want["partials"][0, :tiles[0], 28] > 0).all() and not want["stats"][1:].any()
    for split, fill in ((1, 0xFF), (3, 0xA5)):
        got = TH.run_step(a, device, split=split, fill=fill)
        TH.same_bytes(got, want, tiles, "seven tiles, split %d" % split)
        assert (got["partials"][0, tiles[0]:].view(np.uint8) == fill).all() and (got["partials"][1:].view(np.uint8) == fill).all()


# ---- 2. the loop ---------------------------------------------------------------------------------------------------------------------------
def same_result(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: the poses differ" % what
    for k in ("status", "pixels_first", "pixels_last", "rms_first", "rms_last", "step_status", "step_stats"):
        assert got[1][k].tobytes() == want[1][k].tobytes(), "%s: info[%r] differs" % (what, k)


@pytest.mark.parametrize("name", ["block", "block 37 x 50", "two sizes", "unchanged"])
def test_refine_is_the_host_loops_bytes(device, name):
    case = IC.two_sizes() if name == "two sizes" else TH.CASES[name]()
    got, want = TH.refine(case, device), TH.refine(case)
    same_result(got, want, name)
    kept = got[1]["status"] != 0
    assert np.array_equal(got[0][kept], case["poses"][kept])
    rot, tr = IC.errors(case, got[0])
    assert (~kept).any() and (rot[~kept] < IC.CONVERGED_DEG).all() and (tr[~kept] < IC.CONVERGED_MM).all()


def test_refine_300_jobs_and_chunks(device):
    """300 estimates of one image: two render frames; under a cap of one frame two chunks, with the same bytes"""
    case = IC.many_jobs()
    want = TH.refine(case, iterations=3)
    got = TH.refine(case, device, iterations=3)
    cut = TH.refine(case, device, iterations=3, workspace_cap=900000)
    same_result(got, want, "300 jobs")
    same_result(cut, want, "300 jobs in two chunks")
    assert got[2].last_chunks == 1 and cut[2].last_chunks == 2 and got[2].last_renders == 4 * 300
    assert (got[1]["status"] == 0).sum() > 250


def test_refine_refuses_by_name(device):
    case = IC.unchanged()
    r = TH.refiner_of(case, device)
    for kw, word in ((dict(iterations=0), "iterations"), (dict(gate=-1.0), "gate"), (dict(split=0), "split"), (dict(workspace_cap=1000), "workspace cap")):
        with pytest.raises(ValueError, match=word):
            r.refine(case["poses"], case["K"], case["obj"], case["img"], case["depths"], case["diameters"], **kw)
    with pytest.raises(ValueError, match="image_index"):
        r.refine(case["poses"], case["K"], case["obj"], case["img"] + 3, case["depths"], case["diameters"])


# ---- 3. the script, end to end ---------------------------------------------------------------------------------------------------------------
def mssd(verts, P, Q):
    v = np.asarray(verts, np.float64)
    return float(np.linalg.norm((v @ P[:, :3].T + P[:, 3]) - (v @ Q[:, :3].T + Q[:, 3]), axis=1).max())


def test_refine_script_end_to_end(device, tmp_path):
    import test_masks_twin_host as TM
    from casapose_amd.pose_estimation.bop_scores import read_bop_results
    from casapose_amd.pose_estimation.bop_vsd import DEFAULT_FAR, DEFAULT_NEAR
    from casapose_amd.utils.io_utils import write_poses
    from PIL import Image

    H, W, cam = TM.H, TM.W, TM.BOP_CAM
    root = tmp_path / "bop"
    meshes, poses = TM.write_bop_tree(root)                    # models/ (objects 1 and 5, with faces), test/000002 with two images
    scene_dir = root / "test" / "000002"
    os.makedirs(scene_dir / "depth")
    K = VC.K_of(cam)
    (scene_dir / "scene_camera.json").write_text(json.dumps({str(i): {"cam_K": K.reshape(-1).tolist(), "depth_scale": 0.1} for i in range(2)}))
    ids = [1, 5]
    diam = {o: 2.0 * max(a) for o, a in TM.OBJECTS.items()}
    ref = VR.Scene([meshes[o] for o in ids], DEFAULT_NEAR, DEFAULT_FAR)
    sensors = []
    for im in range(2):
        inst = [(ids.index(o), 1, P) for o, P in poses[im]]
        d = VC.sensor_depth(ref, inst, cam, H, W, (64, 30, 90, 70, 380.0) if im == 0 else (0, 0, 3, 3, 380.0), (40, 40, 47, 46))
        raw = np.rint(d.astype(np.float64) * 10.0).astype(np.uint16)
        Image.fromarray(raw).save(scene_dir / "depth" / ("%06d.png" % im))
        sensors.append(raw.astype(np.float32) * np.float32(0.1))
    # estimates 3-8 degrees and up to (6, 6, 20) mm off; object 1 of image 1 is not found
    rng = np.random.default_rng(31)
    gt_of = [{o: P for o, P in poses[im]} for im in range(2)]
    est = [{o: IC.perturbed(gt_of[im][o], rng, (3.0, 8.0), (6.0, 6.0, 20.0)).astype(np.float32) for o in ids} for im in range(2)]
    est[1][1] = np.zeros((3, 4), np.float32)
    out_dir = str(tmp_path / "run") + "/"
    for im in range(2):
        write_poses(np.stack([gt_of[im][o].astype(np.float32) for o in ids])[:, None], np.stack([est[im][o] for o in ids]), TM.NAMES, "000002_rgb_%06d" % im,
                    out_dir, time_needed=None if im == 0 else 0.25)
    in_file = out_dir + "bop_evaluation.csv"
    before = read_bop_results(in_file)
    rows = [(im, o, 2 * im + k) for im in range(2) for k, o in enumerate(ids)]

    # the reference's loop, on the numbers of the file: every estimate comes closer in MSSD
    for im, o, r in rows:
        if not est[im][o].any():
            continue
        pose, status, _ = IR.refine(ref, ids.index(o), before["pose"][r], cam, sensors[im], diam[o])
        assert status == IR.OK and mssd(meshes[o][0], pose, gt_of[im][o]) < mssd(meshes[o][0], before["pose"][r], gt_of[im][o]), (im, o, status)

    out_file = str(tmp_path / "refined.csv")
    common = ["--dataset_path", str(root), "--split", "test", "--model_folder", "models"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "util_scripts", "refine_poses.py"), "--result_file", in_file, "--out", out_file] + common,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "4 rows, 3 estimates: 3 refined; kept unchanged: none" in r.stdout
    lines_in, lines_out = open(in_file).read().splitlines(True), open(out_file).read().splitlines(True)
    assert len(lines_in) == len(lines_out) == 5 and lines_in[0] == lines_out[0] and lines_in[3] == lines_out[3]      # the header; "not found"
    after = read_bop_results(out_file)
    for k in ("scene_id", "im_id", "obj_id", "score"):
        assert np.array_equal(before[k], after[k])
    assert after["time"][0] == after["time"][1] == -1.0 and after["time"][2] == 0.25 and after["time"][3] > 0.25
    for im, o, r in rows:
        if est[im][o].any():
            e0, e1 = mssd(meshes[o][0], before["pose"][r], gt_of[im][o]), mssd(meshes[o][0], after["pose"][r], gt_of[im][o])
            print("image %d object %d: MSSD %.3f -> %.3f mm" % (im, o, e0, e1))
            assert e1 < e0, (im, o, e0, e1)

    scores = []
    for path in (in_file, out_file):
        out_json = path + ".json"
        s = subprocess.run([sys.executable, os.path.join(ROOT, "util_scripts", "bop_score.py"), "--result_file", path, "--image_width", "640", "--vsd",
                            "--out", out_json] + common, capture_output=True, text=True, timeout=600)
        assert s.returncode == 0, s.stderr[-3000:]
        with open(out_json) as f:
            scores.append(json.load(f))
    print("AR_VSD %.4f -> %.4f, AR %.4f -> %.4f" % (scores[0]["AR_VSD"], scores[1]["AR_VSD"], scores[0]["AR"], scores[1]["AR"]))
    assert scores[1]["AR_VSD"] > scores[0]["AR_VSD"] and scores[1]["AR"] >= scores[0]["AR"]
