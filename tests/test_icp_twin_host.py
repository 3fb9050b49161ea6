"""cp_depth_icp_step_host_f64 -- the host twin of the depth refinement's step, the same header the device kernels compile -- against the NumPy
restatement (tests/icp_reference.py), and `DeviceDepthRefiner.refine(host=True)` against the reference's loop.  No GPU is needed.  The helpers
`step_arrays` and `run_step` also serve tests/test_gpu_depth_icp.py."""
import ctypes as C
import os

import numpy as np
import pytest

import icp_cases as IC
import icp_reference as IR
import vsd_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
JUMP, DAMPING, MIN_PIXELS = 0.75, 1e-6, 32


# ---- one step through the entry point ---------------------------------------------------------------------------------------------------
def step_arrays(case, gate=0.25):
    """the host arrays of one step over a case whose images have one size: every estimate rendered by the renderer's host twin into frames of
    up to 256 slots, one job per estimate -> dict(planes, records, depth, cams, jobs, gates, poses, H, W)"""
    from casapose_amd.data_handler.bop_converter import MAX_INSTANCES, MaskRenderer

    H, W = case["depths"][0].shape
    assert all(d.shape == (H, W) for d in case["depths"])
    by_image = {}
    for i, m in enumerate(case["img"]):
        by_image.setdefault(int(m), []).append(i)
    imax = min(MAX_INSTANCES, max(len(r) for r in by_image.values()))
    frames, jobs, order = [], [], []
    for m, rows in by_image.items():
        for lo in range(0, len(rows), imax):
            part = rows[lo:lo + imax]
            jobs += [(m, len(frames) * imax + k, 0, 0) for k in range(len(part))]
            order += part
            frames.append(dict(cam=case["cam"], instances=[(int(case["obj"][i]), 1, case["poses"][i]) for i in part]))
    renderer = MaskRenderer(None, {i: m for i, m in enumerate(case["meshes"])})
    planes, records = VR.render_planes(renderer, frames, H, W, IC.NEAR, IC.FAR)
    poses = np.zeros((len(frames) * imax, 12))
    poses[[j[1] for j in jobs]] = case["poses"][order].reshape(-1, 12)
    return dict(planes=planes.reshape(-1, H, W), records=np.ascontiguousarray(records.reshape(-1, 11)), depth=np.stack(case["depths"]).astype(np.float32),
                cams=np.tile(np.asarray(case["cam"], np.float64), (len(case["depths"]), 1)), jobs=np.asarray(jobs, np.int32),
                gates=gate * case["diameters"][order], poses=poses, H=H, W=W, order=np.asarray(order))


def run_step(a, device=None, split=1, fill=0xA5, update=1, jump=JUMP, damping=DAMPING, min_pixels=MIN_PIXELS, calls=1):
    """cp_depth_icp_step_f64 on `device`, or its host twin (device None), over `step_arrays`' dict; the workspace pre-filled with the byte
    `fill` -> dict(poses [nplanes, 12], stats [njobs, 4], status [njobs], partials [njobs, max tiles, 29]) as NumPy arrays"""
    from casapose_amd import _lib, twin

    lib = _lib.load()
    njobs, nplanes, H, W = len(a["jobs"]), len(a["planes"]), a["H"], a["W"]
    size = int(lib.cp_depth_icp_workspace_bytes(njobs, H, W))
    assert size > 0 and size % (29 * 8 * njobs) == 0
    stream = None
    if device is not None:
        import torch

        stream = torch.cuda.current_stream(device).cuda_stream
    arg = {k: twin.array(a[k], a[k].dtype, device) for k in ("planes", "records", "depth", "cams", "jobs", "gates")}
    arg["poses"] = twin.array(a["poses"].copy(), np.float64, device)           # rewritten in place: the caller's stay as they are
    out = twin.alloc(dict(stats=((njobs, 4), np.float64), status=((njobs,), np.int32)), device)
    work = twin.array(np.full(size, fill, np.uint8), np.uint8, device)
    for _ in range(calls):
        twin.call("cp_depth_icp_step_f64", arg["planes"], arg["records"], nplanes, H, W, arg["depth"], arg["cams"], len(a["depth"]), arg["jobs"],
                  arg["gates"], njobs, float(jump), float(damping), int(min_pixels), int(update), int(split), arg["poses"], out["stats"], out["status"],
                  work, size, host=device is None, stream=stream)
    back = lambda t: t if device is None else t.cpu().numpy()   # noqa: E731
    return dict(poses=back(arg["poses"]), stats=back(out["stats"]), status=back(out["status"]),
                partials=back(work).view(np.float64).reshape(njobs, -1, 29))


def tiles_of(a, tile):
    """the tiles each job's clipped box has (0 for an empty one, -1 for a refused job)"""
    out = []
    for (m, p, _, _), g in zip(a["jobs"].tolist(), a["gates"]):
        if not (0 <= m < len(a["depth"]) and 0 <= p < len(a["planes"]) and g > 0):
            out.append(-1)
            continue
        x, y, w, h = a["records"][p, 2:6].tolist()
        x0, y0, x1, y1 = max(x, 1), max(y, 1), min(x + w, a["W"] - 2), min(y + h, a["H"] - 2)
        out.append(0 if w < 0 or h < 0 or x0 > x1 or y0 > y1 else -(-(x1 - x0 + 1) * (y1 - y0 + 1) // tile))
    return out


def job_sums(got, n, tiles):
    """job n's 28 sums and count from its tile records, added in index order"""
    s = np.zeros(29)
    for t in range(tiles):
        s = s + got["partials"][n, t]
    return s[:28], int(s[28])


def same_bytes(a, b, tiles, what=""):
    """the results of two runs of one step are the same bytes: poses, stats, status and every job's tile records"""
    for k in ("poses", "stats", "status"):
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differ" % (what, k)
    for n, t in enumerate(tiles):
        if t > 0:
            assert a["partials"][n, :t].tobytes() == b["partials"][n, :t].tobytes(), "%s: the tile records of job %d differ" % (what, n)


def crafted(tile):
    """a box that ends inside the first tile, one that spans three tiles (the last one half full), one across the border, an empty record and
    a box in column 0, which the clipping empties"""
    bw = 64
    rows_a, rows_b = tile // bw - 6, (5 * tile // 2) // bw
    H, W = rows_b + 10, bw + 6
    boxes = [(3, 3, bw - 1, rows_a - 1), (3, 3, bw - 1, rows_b - 1), (-5, -4, 30, 20), (-1, -1, -1, -1), (0, 5, 0, 10)]
    a = IC.crafted_step(H, W, boxes, 3)
    a.update(H=H, W=W)
    return a


def check_against_reference(a, got, tile):
    """counts equal; every sum within N 2^-52 sum |term| (the bound of adding N fp64 terms in any order); the updated pose within
    64 eps cond(A_damped) |xi| of the reference's solve of the twin's own sums, every entry of R and t alike"""
    tiles = tiles_of(a, tile)
    worst = 0.0
    for n, (m, p, _, _) in enumerate(a["jobs"].tolist()):
        if tiles[n] < 0:
            continue
        g = float(a["gates"][n])
        J, r, _, _ = IR.terms(a["planes"][p], a["depth"][m], a["cams"][m], g, JUMP * g)
        want = IR.sums(J, r)
        s, count = job_sums(got, n, tiles[n])
        assert count == want["count"] == got["stats"][n, 0], (n, count, want["count"])
        iu = np.triu_indices(6)
        value = np.concatenate([want["A"][iu], want["b"], [want["rr"]]])
        bound = max(count, 1) * EPS * np.concatenate([want["absA"][iu], want["absb"], [want["rr"]]])
        assert (np.abs(s - value) <= bound).all(), (n, count, np.abs(s - value) / np.maximum(bound, 1e-300))
        if count:
            worst = max(worst, float((np.abs(s - value) / np.maximum(bound, 1e-300)).max()))
        status, _ = IR.solve(want, DAMPING, MIN_PIXELS)
        assert got["status"][n] == status, (n, got["status"][n], status)
        before = a["poses"][p].reshape(3, 4)
        if status != IR.OK:
            assert np.array_equal(got["poses"][p], a["poses"][p]) and got["stats"][n, 2] == 0 and got["stats"][n, 3] == 0
            continue
        A = np.zeros((6, 6))
        A[iu] = s[:21]
        A = A + np.triu(A, 1).T
        M = IR.damped(A, DAMPING)
        xi = np.linalg.solve(M, s[21:27])
        tol = 64 * EPS * np.linalg.cond(M) * np.linalg.norm(xi)
        diff = np.abs(got["poses"][p].reshape(3, 4) - IR.update(before, xi))
        assert diff.max() <= tol, (n, diff.max(), tol)
        assert abs(got["stats"][n, 1] - np.sqrt(s[27] / count)) <= 4 * EPS * got["stats"][n, 1]
        assert abs(got["stats"][n, 2] - np.linalg.norm(xi[:3])) <= tol and abs(got["stats"][n, 3] - np.linalg.norm(xi[3:])) <= tol
    return worst


CASES = {"block": lambda: IC.block(), "block 37 x 50": lambda: IC.block(37, 50), "ellipsoids": IC.ellipsoids, "300 jobs": IC.many_jobs,
         "unchanged": IC.unchanged}
_arrays = {}


def arrays_of(name, tile):
    if name not in _arrays:
        _arrays[name] = crafted(tile) if name == "crafted" else step_arrays(CASES[name]())
    return _arrays[name]


# ---- the twin against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + ["crafted"])
def test_twin_step_against_reference(hip_lib, name):
    tile = hip_lib.cp_depth_icp_tile()
    a = arrays_of(name, tile)
    got = run_step(a)
    worst = check_against_reference(a, got, tile)
    print("%s: %d jobs, tiles %s, worst sum error / bound %.3f" % (name, len(a["jobs"]), sorted(set(tiles_of(a, tile))), worst))
    solved = got["status"] == 0
    assert solved.any() and not np.array_equal(got["poses"][a["jobs"][solved, 1]], a["poses"][a["jobs"][solved, 1]])
    slots = np.ones(len(a["poses"]), bool)
    slots[a["jobs"][solved, 1]] = False
    assert np.array_equal(got["poses"][slots], a["poses"][slots])          # no other pose is written
    if name == "crafted":
        assert tiles_of(a, tile) == [1, 3, 1, 0, 0] and got["status"].tolist() == [0, 0, 0, 1, 1]
    if name == "unchanged":
        assert got["status"].tolist() == IC.unchanged()["want"].tolist()


@pytest.mark.parametrize("name", ["block 37 x 50", "crafted"])
def test_twin_does_not_depend_on_the_workspace_or_the_split(hip_lib, name):
    tile = hip_lib.cp_depth_icp_tile()
    a = arrays_of(name, tile)
    first = run_step(a, fill=0x00)
    for fill, split in ((0xFF, 1), (0xA5, 3), (0x00, 64)):
        same_bytes(run_step(a, fill=fill, split=split), first, tiles_of(a, tile), "fill %#x, split %d" % (fill, split))
    evaluated = run_step(a, update=0)
    assert np.array_equal(evaluated["poses"], a["poses"]) and evaluated["stats"].tobytes() == first["stats"].tobytes()
    assert evaluated["status"].tobytes() == first["status"].tobytes()


def test_twin_refuses_jobs_out_of_range_and_reads_nothing_for_them(hip_lib):
    tile = hip_lib.cp_depth_icp_tile()
    a = dict(arrays_of("crafted", tile))
    good = run_step(a)
    n, big = len(a["planes"]), 2 ** 31 - 1
    a["jobs"] = np.concatenate([a["jobs"][:2], np.array([(1, 0, 0, 0), (-1, 0, 0, 0), (0, n, 0, 0), (0, -1, 0, 0), (big, big, 0, 0), (0, 2, 0, 0), (0, 2, 0, 0),
                                                          (0, 2, 0, 0)], np.int32)])
    a["gates"] = np.concatenate([a["gates"][:2], [40.0] * 5, [0.0, -1.0, np.nan]])
    got = run_step(a)
    assert got["status"].tolist() == [0, 0] + [3] * 8 and not got["stats"][2:].any()
    assert got["stats"][:2].tobytes() == good["stats"][:2].tobytes() and got["poses"].tobytes()[:2 * 96] == good["poses"].tobytes()[:2 * 96]
    assert np.array_equal(got["poses"][2:], a["poses"][2:])
    assert (got["partials"][2:].view(np.uint8) == 0xA5).all()              # not a word of a refused job's records is written


# ---- the whole loop ----------------------------------------------------------------------------------------------------------------------
def refiner_of(case, device=None, **kw):
    from casapose_amd.pose_estimation.depth_refine import DeviceDepthRefiner

    return DeviceDepthRefiner([m[0] for m in case["meshes"]], [m[1] for m in case["meshes"]], device, IC.NEAR, IC.FAR, **kw)


def refine(case, device=None, **kw):
    r = refiner_of(case, device)
    return r.refine(case["poses"], case["K"], case["obj"], case["img"], case["depths"], case["diameters"], host=device is None, **kw) + (r,)


@pytest.mark.parametrize("name", ["block", "block 37 x 50", "two sizes", "unchanged", "ellipsoids"])
def test_host_loop_against_the_references_loop(name):
    case = IC.two_sizes() if name == "two sizes" else CASES[name]()
    kw = dict(min_pixels=IC.ELLIPSOID_MIN_PIXELS) if name == "ellipsoids" else {}
    want_poses, want_status, want_stats = IC.reference_loop(case, **kw)
    poses, info, refiner = refine(case, **kw)
    assert np.array_equal(info["status"], want_status), (info["status"], want_status)
    assert info["status_names"][1] == "few_pixels" and refiner.last_renders == 9 * len(poses)
    assert np.array_equal(info["pixels_first"], want_stats[:, 0, 0]) and np.array_equal(info["pixels_last"], want_stats[:, -1, 0])
    np.testing.assert_allclose(info["rms_first"], want_stats[:, 0, 1], rtol=1e-9)
    kept = info["status"] != 0
    assert np.array_equal(poses[kept], case["poses"][kept])                # rejected: the input, bit for bit
    if name != "ellipsoids":
        rot, tr = IC.errors(case, poses)
        ref_rot, ref_tr = IC.errors(case, want_poses)
        inside = (ref_rot < IC.CONVERGED_DEG) & (ref_tr < IC.CONVERGED_MM) & ~kept
        assert inside.sum() == (~kept).sum() and (rot[inside] < IC.CONVERGED_DEG).all() and (tr[inside] < IC.CONVERGED_MM).all(), (rot, tr)
    else:
        for i in range(len(poses)):
            verts = case["meshes"][int(case["obj"][i])][0]
            assert IR.mean_vertex_distance(verts, poses[i], case["gt"][i]) < 0.25 * IR.mean_vertex_distance(verts, case["poses"][i], case["gt"][i])


def test_host_loop_does_not_depend_on_the_chunks():
    """300 estimates of one image are two render frames of 256 slots: one chunk under the default cap, two under a cap of one frame"""
    case = IC.many_jobs()
    _, ref_status, _ = IC.reference_loop(case, iterations=2)
    assert (ref_status == 0).sum() > 250                                        # the reference first: most of the 300 are refined
    whole, info_whole, one = refine(case, iterations=2)
    cut, info_cut, two = refine(case, iterations=2, workspace_cap=900000)      # a frame: 256 planes of 24 x 32 words and 256 tile records
    assert one.last_chunks == 1 and two.last_chunks == 2 and whole.tobytes() == cut.tobytes()
    for k in ("status", "step_status", "step_stats"):
        assert info_whole[k].tobytes() == info_cut[k].tobytes(), k
    assert (info_whole["status"] == 0).sum() > 250
    _, _, sizes = refine(IC.two_sizes(), iterations=1)
    assert sizes.last_chunks == 2                                               # one per image size


def test_keep_rule_by_hand():
    from casapose_amd.pose_estimation import depth_refine as D

    ok = np.zeros((3, 5), np.int32)
    stats = np.zeros((3, 5, 4))
    stats[0, :, :2] = (300.0, 2.0)
    stats[2, :, :2] = [(149.0, 1.0), (150.0, 1.0), (300.0, 2.5), (300.0, 2.0), (300.0, 1.0)]
    assert D.keep_rule(ok, stats, 32).tolist() == [D.LOST_PIXELS, D.REFINED, D.RMS_ROSE, D.REFINED, D.REFINED]
    stats[0, 0, 0], stats[2, 0, 0] = 40.0, 31.0
    assert D.keep_rule(ok, stats, 32)[0] == D.LOST_PIXELS and D.keep_rule(ok, stats, 31)[0] == D.REFINED
    ok[1, 4], ok[2, 4] = D.SINGULAR, D.FEW_PIXELS
    assert D.keep_rule(ok, stats, 32)[4] == D.SINGULAR and D.STATUS_NAMES[D.RMS_ROSE] == "rms_rose"


# ---- the script ----------------------------------------------------------------------------------------------------------------------------
def test_script_refuses_a_missing_depth_image_before_any_device_work(tmp_path, monkeypatch):
    import sys

    import test_masks_twin_host as TM
    from casapose_amd.utils.io_utils import write_poses
    from PIL import Image

    sys.path.insert(0, os.path.join(ROOT, "util_scripts"))
    try:
        import refine_poses
    finally:
        sys.path.pop(0)
    root = tmp_path / "bop"
    TM.write_bop_tree(root)                                   # models/, test/000002 with two images; no depth/
    os.makedirs(root / "test" / "000002" / "depth")
    Image.fromarray(np.full((TM.H, TM.W), 5000, np.uint16)).save(root / "test" / "000002" / "depth" / "000000.png")
    out_dir = str(tmp_path / "run") + "/"
    for im, instances in enumerate(TM.bop_poses()):
        poses = {o: P.astype(np.float32) for o, P in instances}
        write_poses(np.stack([poses[1], poses[5]])[:, None], np.stack([poses[1], poses[5]]), TM.NAMES, "000002_rgb_%06d" % im, out_dir)

    def no_device(*a, **k):
        raise AssertionError("a refiner was built before the depth images were checked")

    monkeypatch.setattr(refine_poses, "DeviceDepthRefiner", no_device)
    args = ["--result_file", out_dir + "bop_evaluation.csv", "--dataset_path", str(root), "--model_folder", "models", "--out", str(tmp_path / "refined.csv")]
    with pytest.raises(FileNotFoundError, match=r"depth.000001\.png"):
        refine_poses.main(args)
    with pytest.raises(FileNotFoundError, match=r"sensor.000000\.png"):
        refine_poses.main(args + ["--depth_folder", "sensor"])
    assert not os.path.exists(tmp_path / "refined.csv")
    line = "2,0,1,1.0,1 0 0 0 1 0 0 0 1,0.5 1.5 400.25,-1.0\n"
    pose = np.hstack([np.eye(3), [[0.1], [0.2], [0.30000000000000004]]])
    assert refine_poses.row_text(line, pose, 0.5) == "2,0,1,1.0,1.0 0.0 0.0 0.0 1.0 0.0 0.0 0.0 1.0,0.1 0.2 0.30000000000000004,-1.0\n"
    assert refine_poses.row_text(line.replace("-1.0\n", "0.25\n"), pose, 0.5).endswith(",0.75\n")
    timed = line.replace("-1.0\n", "0.25\n")
    assert refine_poses.row_text(line, None, 0.5) is line and refine_poses.row_text(timed, None, 0.0) is timed       # nothing to change
    assert refine_poses.row_text(timed, None, 0.5) == "2,0,1,1.0,1 0 0 0 1 0 0 0 1,0.5 1.5 400.25,0.75\n"           # rejected: its pose text, the time


def test_script_on_the_host_loop_gives_every_estimate_of_an_image_one_time(tmp_path, monkeypatch, capsys):
    """The script with its refiner switched to host=True: a kept estimate, a rejected one (two gates too deep), a "not found" row and an
    estimate of an object without a mesh, all in image 1 with a time of 0.25, and image 0 with a time of -1."""
    import json
    import sys

    import test_masks_twin_host as TM
    import vsd_cases as VC
    from casapose_amd.pose_estimation import depth_refine
    from casapose_amd.pose_estimation.bop_scores import read_bop_results
    from casapose_amd.pose_estimation.bop_vsd import DEFAULT_FAR, DEFAULT_NEAR
    from casapose_amd.utils.io_utils import write_poses
    from PIL import Image

    sys.path.insert(0, os.path.join(ROOT, "util_scripts"))
    try:
        import refine_poses
    finally:
        sys.path.pop(0)
    H, W, cam = TM.H, TM.W, TM.BOP_CAM
    root = tmp_path / "bop"
    meshes, poses = TM.write_bop_tree(root)
    scene_dir = root / "test" / "000002"
    os.makedirs(scene_dir / "depth")
    (scene_dir / "scene_camera.json").write_text(json.dumps({str(i): {"cam_K": VC.K_of(cam).reshape(-1).tolist(), "depth_scale": 0.1} for i in range(2)}))
    ids = [1, 5]
    ref = VR.Scene([meshes[o] for o in ids], DEFAULT_NEAR, DEFAULT_FAR)
    for im in range(2):
        d = VC.sensor_depth(ref, [(ids.index(o), 1, P) for o, P in poses[im]], cam, H, W, (0, 0, 3, 3, 380.0), (40, 40, 47, 46))
        Image.fromarray(np.rint(d.astype(np.float64) * 10.0).astype(np.uint16)).save(scene_dir / "depth" / ("%06d.png" % im))
    gt_of = [{o: P for o, P in poses[im]} for im in range(2)]
    rng = np.random.default_rng(31)
    near = lambda P: IC.perturbed(P, rng, (3.0, 8.0), (6.0, 6.0, 20.0)).astype(np.float32)   # noqa: E731
    deep = np.hstack([gt_of[1][1][:, :3], gt_of[1][1][:, 3:] + [[0.0], [0.0], [2.0 * 0.25 * 80.0]]]).astype(np.float32)
    est = [{1: np.zeros((3, 4), np.float32), 5: near(gt_of[0][5])}, {1: deep, 5: near(gt_of[1][5])}]
    out_dir = str(tmp_path / "run") + "/"
    for im in range(2):
        write_poses(np.stack([gt_of[im][o].astype(np.float32) for o in ids])[:, None], np.stack([est[im][o] for o in ids]), TM.NAMES, "000002_rgb_%06d" % im,
                    out_dir, time_needed=None if im == 0 else 0.25)
    in_file, out_file = out_dir + "bop_evaluation.csv", str(tmp_path / "refined.csv")
    with open(in_file, "a") as f:
        f.write("2,1,9,1.0,1.0 0.0 0.0 0.0 1.0 0.0 0.0 0.0 1.0,0.0 0.0 500.0,0.25\n")          # object 9 has no mesh

    class HostRefiner(depth_refine.DeviceDepthRefiner):
        def __init__(self, verts, faces, device):
            super().__init__(verts, faces, None)

        def refine(self, *a, **k):
            return super().refine(*a, host=True, **k)

    monkeypatch.setattr(refine_poses, "DeviceDepthRefiner", HostRefiner)
    got = refine_poses.main(["--result_file", in_file, "--dataset_path", str(root), "--model_folder", "models", "--out", out_file])
    printed = capsys.readouterr().out
    assert got["estimates"] == 4 and got["no_mesh"] == 1 and got["refined"] == 2 and sorted(got["status"]) == [0, 0, 1], got
    assert "5 rows, 4 estimates: 2 refined; kept unchanged: 1 few_pixels; 1 estimate(s) of objects without a mesh" in printed, printed
    lines_in, lines_out = open(in_file).read().splitlines(True), open(out_file).read().splitlines(True)
    assert len(lines_out) == 6 and lines_out[0] == lines_in[0] and lines_out[1] == lines_in[1]                      # the header; "not found"
    before, after = read_bop_results(in_file), read_bop_results(out_file)
    for k in ("scene_id", "im_id", "obj_id", "score"):
        assert np.array_equal(before[k], after[k])
    assert after["time"][0] == after["time"][1] == -1.0                                                             # -1 stays -1
    assert after["time"][2] == after["time"][3] == after["time"][4] > 0.25                                          # image 1: one time
    assert not np.array_equal(after["pose"][1], before["pose"][1]) and not np.array_equal(after["pose"][3], before["pose"][3])
    assert lines_out[3].split(",")[4:6] == lines_in[3].split(",")[4:6] and lines_out[5].split(",")[4:6] == lines_in[5].split(",")[4:6]


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from casapose_amd import _lib

    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    i, d, p, z = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    args = [p, p, i, i, i, p, p, i, p, p, i, d, d, i, i, i, p, p, p, p, z]
    assert table["cp_depth_icp_tile"] == (C.c_int, []) and table["cp_depth_icp_workspace_bytes"] == (z, [i, i, i])
    assert table["cp_depth_icp_step_f64"] == (C.c_int, args + [p]) and table["cp_depth_icp_step_host_f64"] == (C.c_int, args)
    assert _lib.POINTEES["cp_depth_icp_step_f64"] == ("uint32_t", "int32_t", None, None, None, "float", "double", None, "int32_t", "double", None, None,
                                                      None, None, None, None, "double", "double", "int32_t", "void", None, "void")
    assert _lib.host_twin("cp_depth_icp_step_f64") == "cp_depth_icp_step_host_f64" and _lib.ABI_VERSION == 302
    tile = hip_lib.cp_depth_icp_tile()
    assert tile >= 64 and tile % 64 == 0 and hasattr(hip_lib, "cp_depth_icp_step_host_f64")
    assert hip_lib.cp_depth_icp_workspace_bytes(3, 48, 64) == 3 * -(-46 * 62 // tile) * 29 * 8
    assert hip_lib.cp_depth_icp_workspace_bytes(1, 2, 2) == 29 * 8 and hip_lib.cp_depth_icp_workspace_bytes(0, 4, 4) == 0
    assert hip_lib.cp_depth_icp_workspace_bytes(1, 16385, 4) == 0
    text = open(os.path.join(ROOT, "include", "casapose_hip.h")).read()
    block = text[text.index("depth refinement: projective point-to-plane ICP"):text.index("int cp_depth_icp_tile(void);")]
    assert block.rstrip().endswith("Added in ABI 302 without changing any earlier entry point. */")


@pytest.mark.parametrize("symbol", ["cp_depth_icp_step_f64", "cp_depth_icp_step_host_f64"])
def test_entry_points_refuse_bad_arguments_by_name(hip_lib, symbol):
    """CP_REQUIRE runs before anything is launched or read: no GPU is needed to be refused"""
    a = np.zeros(256, np.float64)
    p = a.ctypes.data
    ok = [p, p, 1, 4, 4, p, p, 1, p, p, 1, 0.75, 1e-6, 32, 1, 1, p, p, p, p, 29 * 8]
    tail = (None,) if symbol.endswith("step_f64") else ()
    for at, bad, word in ((0, None, b"null"), (19, None, b"null"), (2, 0, b"nplanes"), (7, 0, b"images"), (10, 0, b"njobs"), (3, 16385, b"H and W"),
                          (4, 0, b"H and W"), (11, 0.0, b"jump"), (11, float("nan"), b"jump"), (12, -1e-9, b"damping"), (12, float("inf"), b"damping"),
                          (13, 0, b"min_pixels"), (14, 2, b"update"), (15, 0, b"split"), (15, 65, b"split"), (20, 29 * 8 - 1, b"workspace_bytes"),
                          (6, p + 4, b"8-byte"), (19, p + 4, b"8-byte"), (18, p + 2, b"4-byte")):
        args = list(ok)
        args[at] = bad
        assert getattr(hip_lib, symbol)(*args, *tail) == -1, word
        message = hip_lib.cp_last_error()
        assert word in message and symbol.encode() in message, (word, message)


def test_refiner_without_a_device_has_no_fall_back():
    from casapose_amd._lib import CasaposeHipError

    case = IC.unchanged()
    r = refiner_of(case)
    call = lambda **kw: r.refine(case["poses"], case["K"], case["obj"], case["img"], case["depths"], case["diameters"], **kw)   # noqa: E731
    with pytest.raises(CasaposeHipError, match="no host fall-back"):
        call()
    for kw, word in ((dict(iterations=0), "iterations"), (dict(gate=0.0), "gate"), (dict(jump=-1.0), "jump"), (dict(damping=-1.0), "damping"),
                     (dict(min_pixels=0), "min_pixels"), (dict(split=65), "split"), (dict(workspace_cap=1000), "workspace cap")):
        with pytest.raises(ValueError, match=word):
            call(host=True, **kw)
    with pytest.raises(ValueError, match="object_index"):
        r.refine(case["poses"], case["K"], case["obj"] + 2, case["img"], case["depths"], case["diameters"], host=True)
    with pytest.raises(ValueError, match="image_index"):
        r.refine(case["poses"], case["K"], case["obj"], case["img"] + 3, case["depths"], case["diameters"], host=True)
    with pytest.raises(ValueError, match="one array per object"):
        refiner_of(dict(meshes=[]))
