"""cp_mask_edt_u16, cp_contour_step_f64 (csrc/mask_contour.hip), DeviceMaskRefiner and the inference scripts' path under CASAPOSE_MASK_REFINE=1
on the GPU.

The device and the host twins compile one header (csrc/contour_math.h: exact integers; fp64, no contraction, a fixed order of summation), and
the renderer's device and host planes are the same bytes (tests/test_gpu_masks.py), so every comparison here is bit for bit: the field on
every case of the twin's table with its refusals, one step on every case for three splits and two workspace fills, the whole loop, and the
loop cut into chunks.  The twins themselves are held against SciPy and the NumPy restatement on the CPU (tests/test_contour_twin_host.py).
A refused job is range-checked before it addresses anything, on the device as in the twin."""
import weakref

import numpy as np
import pytest
import torch

import contour_cases as CC
import test_contour_twin_host as TH

pytestmark = pytest.mark.gpu

_host = {}


def host_step(name, tile):
    if name not in _host:
        _host[name] = TH.run_step(TH.arrays_of(name, tile))
    return _host[name]


# ---- 1. the field --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TH.edt_cases()))
def test_field_is_the_host_twins_bytes(device, name):
    labels, jobs, G = TH.edt_cases()[name]
    want = TH.host_edt(name)
    for fill in (0xFF, 0x00):
        got = TH.run_edt(labels, jobs, G, device, fill=fill)
        assert got["planes"].tobytes() == want["planes"].tobytes(), (name, np.argwhere(got["planes"] != want["planes"])[:4].tolist())
        assert got["status"].tobytes() == want["status"].tobytes()


def test_field_refusals_on_the_device(device):
    labels, _, G = TH.edt_cases()["48 x 64"]
    big = 2 ** 31 - 1
    jobs = [(0, 1), (1, 1), (-1, 1), (0, 0), (0, 256), (0, -1), (big, big), (0, 3)]
    got, want = TH.run_edt(labels, jobs, G, device), TH.run_edt(labels, jobs, G)
    assert got["status"].tolist() == [0, 3, 3, 3, 3, 3, 3, 0] and got["planes"].tobytes() == want["planes"].tobytes()
    assert (got["planes"][1:7] == TH.PLANE_FILL).all() and (got["rows"][1:7].view(np.uint8) == 0xA5).all()      # not a byte of theirs is written


# ---- 2. one step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TH.CASES) + ["crafted"])
def test_one_step_is_the_host_twins_bytes(hip_lib, device, name):
    tile = hip_lib.cp_contour_tile()
    a = TH.arrays_of(name, tile)
    want, tiles = host_step(name, tile), TH.tiles_of(a, tile)
    assert min(tiles) >= 0
    for split, fill in ((1, 0xFF), (3, 0xA5), (8, 0xFF)):
        TH.same_bytes(TH.run_step(a, device, split=split, fill=fill), want, tiles, "%s, split %d" % (name, split))
    evaluated = TH.run_step(a, device, update=0, split=3)
    assert evaluated["poses"].tobytes() == a["poses"].tobytes() and evaluated["stats"].tobytes() == want["stats"].tobytes()
    assert evaluated["status"].tobytes() == want["status"].tobytes()


def test_two_calls_in_a_row(hip_lib, device):
    """the second call starts from the first one's poses and the same planes, on the device as on the host"""
    tile = hip_lib.cp_contour_tile()
    a = TH.arrays_of("block 37 x 50", tile)
    TH.same_bytes(TH.run_step(a, device, split=3, calls=2), TH.run_step(a, calls=2), TH.tiles_of(a, tile), "two calls")


def test_a_wave_takes_a_second_tile_beside_an_empty_and_a_refused_job(hip_lib, device):
    """72 x 96 under a full-frame box: 70 x 94 = 6580 pixels, seven tiles of 1024 with the last one part full -- more than the four waves of
    split 1, so three waves take a second tile.  The plane and the label both have a lattice of holes, so every tile has contour pixels near
    seeds.  In the same call an empty record and a job refused for its gate (its indices are in range): no tiles, so not a word of their
    records is written, and a word read for them would be the fill's NaN in their stats"""
    tile = hip_lib.cp_contour_tile()
    H, W, G = 72, 96, 4
    yy, xx = np.mgrid[0:H, 0:W]
    z = (1000.0 + 0.4 * xx - 0.3 * yy + 4.0 * np.sin(0.35 * xx) * np.cos(0.3 * yy)).astype(np.float32)
    planes = np.full((2, H, W), 0xFFFFFFFF, np.uint32)
    planes[0] = np.where((xx % 5 == 2) & (yy % 4 == 1), np.uint32(0xFFFFFFFF), z.view(np.uint32))
    records = np.full((2, 11), -1, np.int32)
    records[0, 2:6] = (0, 0, W - 1, H - 1)
    labels = np.where((xx % 6 == 3) & (yy % 5 == 2), 0, 1).astype(np.uint8)[None]
    a = dict(planes=planes, records=records, fields=TH.run_edt(labels, [(0, 1)], G)["planes"], cams=np.array([[400.0, 410.0, W / 2 - 0.3, H / 2 + 0.2]]),
             poses=np.tile(np.hstack([np.eye(3), [[0.0], [0.0], [1000.0]]]).reshape(12), (2, 1)),
             jobs=np.array([(0, 0, 0, G), (0, 1, 0, G), (0, 0, 0, 0)], np.int32), H=H, W=W, offset=0.25)
    tiles = TH.tiles_of(a, tile)
    assert tiles == [-(-70 * 94 // tile), 0, -1] and tiles[0] > 4 and 70 * 94 % tile != 0
    want = TH.run_step(a)
    assert want["status"].tolist()[1:] == [1, 3] and (want["partials"][0, :tiles[0], 28] > 0).all() and not want["stats"][1:].any()
    for split, fill in ((1, 0xFF), (3, 0xA5)):
        got = TH.run_step(a, device, split=split, fill=fill)
        TH.same_bytes(got, want, tiles, "seven tiles, split %d" % split)
        assert (got["partials"][0, tiles[0]:].view(np.uint8) == fill).all() and (got["partials"][1:].view(np.uint8) == fill).all()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------
def same_result(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), "%s: the poses differ" % what
    for k in ("status", "pixels_first", "pixels_last", "rms_first", "rms_last", "step_status", "step_stats"):
        assert got[1][k].tobytes() == want[1][k].tobytes(), "%s: info[%r] differs" % (what, k)


@pytest.mark.parametrize("name", ["block", "block 37 x 50", "two images", "others", "unchanged"])
def test_refine_is_the_host_loops_bytes(device, name):
    case = TH.CASES[name]()
    got, want = TH.refine(case, device), TH.refine(case)
    same_result(got, want, name)
    kept = got[1]["status"] != 0
    assert np.array_equal(got[0][kept], case["poses"][kept]) and (~kept).any()
    if name.startswith("block"):
        assert CC.inside(case, got[0])[~kept].all()


def test_refine_300_jobs_and_chunks(hip_lib, device):
    """300 estimates of one image: two render frames; under a cap of one frame two chunks, with the same bytes"""
    case = CC.many_jobs()
    one_frame = (int(hip_lib.cp_render_masks_workspace_bytes(1, 256, 37, 50)) + int(hip_lib.cp_contour_step_workspace_bytes(256, 37, 50)) +
                 2 * int(hip_lib.cp_mask_edt_workspace_bytes(256, 37, 50)))
    want = TH.refine(case, iterations=3)
    got = TH.refine(case, device, iterations=3)
    cut = TH.refine(case, device, iterations=3, workspace_cap=one_frame + 100)
    same_result(got, want, "300 jobs")
    same_result(cut, want, "300 jobs in two chunks")
    assert got[2].last_chunks == 1 and cut[2].last_chunks == 2 and got[2].last_renders == 4 * 300 and cut[2].last_fields == 2
    assert (got[1]["status"] == 0).sum() > 200


def test_refine_refuses_by_name(device):
    case = CC.unchanged()
    r = TH.refiner_of(case, device)
    labels = torch.from_numpy(np.array(case["labels"])).to(device)
    for kw, word in ((dict(iterations=0), "iterations"), (dict(gate=0), "gate"), (dict(split=0), "split"), (dict(workspace_cap=1000), "workspace cap")):
        with pytest.raises(ValueError, match=word):
            r.refine(case["poses"], case["K"], case["obj"], case["img"], labels, case["label_of"], **kw)
    with pytest.raises(ValueError, match="device tensor"):
        r.refine(case["poses"], case["K"], case["obj"], case["img"], case["labels"], case["label_of"])


# ---- 4. the inference scripts' path ------------------------------------------------------------------------------------------------------------
def test_inference_path_under_the_switch(device, monkeypatch, tmp_path):
    """util_scripts/test_minimal.py's lines on a synthetic frame -- voter([seg, dirs, conf]), then poses_pnp, which under CASAPOSE_MASK_REFINE=1
    aligns its poses with the label map of the voter that returned the keypoints, with a refiner built from the evaluation vertices of the
    dataset the script built last and the faces of its mesh files.  The segmentation is the block scene's label map at 48 x 64 (three objects), the keypoint field points at the
    keypoints of poses a few degrees and millimetres off, so PnP returns those poses: the block's refined pose is closer to the truth in the
    image plane, the small ellipsoid has too few contour pixels and keeps its PnP pose, an object that was not found stays the zero pose, and
    with the switch unset nothing is refined."""
    from casapose_amd.pose_estimation import mask_refine as M
    from casapose_amd.pose_estimation.pose_evaluation import poses_pnp
    from casapose_amd.pose_estimation.voting_layers_2d import CoordLSVotingWeighted

    H, W, cam = 48, 64, CC.CAM
    meshes = CC.meshes()
    names = ["block", "occluder", "cut"]
    for name, (v, f) in zip(names, meshes):
        d = tmp_path / name
        d.mkdir()
        with open(d / (name + ".obj"), "w") as out:
            out.write("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in v) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))

    class Dataset:      # what mask_refine asks of the VectorfieldDataset a script built last
        path_meshes, objectsofinterest, last_offsets = str(tmp_path), names, np.array([0.0, 0, H, W, 0, 0, 0, 1, W, H], np.float32)

        def generate_object_vertex_array(self):
            vmax = max(len(m[0]) for m in meshes)
            arr = np.zeros((3, vmax, 3), np.float32)
            for i, (v, _) in enumerate(meshes):
                arr[i, :len(v)] = v
            return arr, np.array([[len(m[0])] for m in meshes], np.int32)

    occ, cut = CC.placements(W)
    truth = [CC.IC.BLOCK_GT, occ, cut]
    start = CC.block_starts()[0]
    off = [start[1], CC.others()["poses"][0], np.zeros((3, 4))]                     # the third object is not found
    K = CC.IC.VC.K_of(cam)
    kp3 = np.stack([np.concatenate([v.mean(0, keepdims=True), v[np.linspace(0, len(v) - 1, 8).astype(int)]]) for v, _ in meshes]).astype(np.float32)
    lab = CC.label_map(H, W)
    seg = np.zeros((1, H, W, 4), np.float32)
    field = np.zeros((1, H, W, 9, 2), np.float32)
    ys, xs = np.mgrid[0:H, 0:W] + 0.5
    for o in range(2):
        m = lab == o + 1
        cam_pts = kp3[o].astype(np.float64) @ off[o][:, :3].T + off[o][:, 3]
        u, v = cam[0] * cam_pts[:, 0] / cam_pts[:, 2] + cam[2], cam[1] * cam_pts[:, 1] / cam_pts[:, 2] + cam[3]
        ang = np.arctan2(v[None] - ys[m][:, None], u[None] - xs[m][:, None])
        field[0][m] = np.stack([np.sin(ang), np.cos(ang)], -1)
    seg[0] = 10.0 * np.eye(4, dtype=np.float32)[np.where(lab == 3, 0, lab)]           # the cut object is not segmented
    seg_d, dirs_d, conf_d = (torch.from_numpy(a).to(device) for a in (seg, field.reshape(1, H, W, 18), np.zeros((1, H, W, 9), np.float32)))
    voter = CoordLSVotingWeighted(name="coords_ls_voting", num_classes=4, num_points=9, filter_estimates=True)
    voter.min_component = 20

    from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset

    dataset = Dataset()
    monkeypatch.setattr(VectorfieldDataset, "last_instance", weakref.ref(dataset))
    monkeypatch.setattr(M, "_refiners", {})

    def run():      # the script's two lines; under the switch poses_pnp finds the voter and the dataset by itself
        coords = voter([seg_d, dirs_d, conf_d])
        poses = poses_pnp(coords, seg_d, torch.from_numpy(kp3[None, :, None]), torch.from_numpy(K[None]), 3, min_num=20, rng=np.random.default_rng(0))
        return np.asarray(poses), (list(M._refiners.values()) or [(None, None)])[-1][1]

    monkeypatch.delenv("CASAPOSE_MASK_REFINE", raising=False)
    plain, none = run()
    again, _ = run()
    assert none is None and plain.shape == (1, 3, 1, 3, 4) and plain.tobytes() == again.tobytes() and not plain[0, 2].any()
    for o in range(2):                                  # PnP returns the poses the field points at
        assert CC.IC.IR.mean_vertex_distance(meshes[o][0], plain[0, o, 0], off[o]) < 2.0, (o, plain[0, o, 0], off[o])
    monkeypatch.setenv("CASAPOSE_MASK_REFINE", "1")
    refined, refiner = run()
    again, same = run()
    assert same is refiner and len(M._refiners) == 1 and again.tobytes() == refined.tobytes()        # one refiner, built once
    info = refiner.last_info
    assert refined.shape == plain.shape and refined.dtype == plain.dtype and not refined[0, 2].any()
    # the block is refined; the small ellipsoid's contour has fewer than min_pixels pixels: its PnP pose comes back as it went in
    assert info["status"].tolist() == [0, 1] and info["status_names"][1] == "few_pixels" and refiner.last_fields == 2 and refiner.sample_offset == 0.5
    assert refined[0, 1].tobytes() == plain[0, 1].tobytes() and info["pixels_first"][1] < M.DEFAULT_MIN_PIXELS <= info["pixels_first"][0]
    before, after = plain[0, 0, 0].astype(np.float64), refined[0, 0, 0].astype(np.float64)
    e0, e1 = np.linalg.norm((before - truth[0])[:2, 3]), np.linalg.norm((after - truth[0])[:2, 3])
    r0, r1 = CC.IC.IR.rotation_error_deg(before, truth[0]), CC.IC.IR.rotation_error_deg(after, truth[0])
    print("block: %.3f -> %.3f mm in the image plane, %.2f -> %.2f degrees, rms %.3f -> %.3f pixels" % (e0, e1, r0, r1, info["rms_first"][0], info["rms_last"][0]))
    assert e1 < 0.5 * e0 and info["rms_last"][0] < info["rms_first"][0]      # the host loop on the same start: 3.29 -> 0.72 mm
    # the same estimates through the host loop: the device's bytes
    host = M.DeviceMaskRefiner([m[0] for m in meshes], [m[1] for m in meshes], None, refiner.near, refiner.far)
    want, _ = host.refine(plain[0, :2, 0].astype(np.float64), K, [0, 1], [0, 0], voter.last_labels.cpu().numpy(), [1, 2], host=True)
    assert refined[0, :2, 0].tobytes() == want.astype(refined.dtype).tobytes()
    # a batch with a crop is refused by name, and so are keypoints that no voter returned
    dataset.last_offsets = np.array([16.0, 96, H, W, 0, 0, 0, 1, W, H], np.float32)
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1"):
        run()
    dataset.last_offsets = None                         # no annotated frame drawn: refused too, not passed over
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1 needs the offsets"):
        run()
    dataset.last_offsets = np.array([0.0, 0, H, W, 0, 0, 0, 1, W, H], np.float32)
    other = Dataset()                                   # another dataset: its own refiner, not the first one's
    monkeypatch.setattr(VectorfieldDataset, "last_instance", weakref.ref(other))
    assert run()[1] is not refiner and len(M._refiners) == 1
    coords = voter([seg_d, dirs_d, conf_d]).clone()
    with pytest.raises(ValueError, match="poses_pnp: CASAPOSE_MASK_REFINE=1 needs the keypoints tensor"):
        poses_pnp(coords, seg_d, torch.from_numpy(kp3[None, :, None]), torch.from_numpy(K[None]), 3, min_num=20, rng=np.random.default_rng(0))
