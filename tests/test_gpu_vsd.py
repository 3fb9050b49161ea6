"""cp_vsd_counts_i32 (csrc/vsd.hip), DeviceVsdScorer and util_scripts/bop_score.py --vsd on the GPU against tests/vsd_reference.py, fp64 NumPy
written from BOP's definitions over the depth planes of the renderer's host twin.

The gate (vsd_reference.check_counts): the results are integers.  On every pair without an undecided pixel -- one with a comparison within 1e-9 mm
or 1e-12 of its threshold, where the device's z * c and the reference's formula, a few fp64 ulps apart, may fall on different sides -- all 2 + ntau
counts are equal to the reference's; on the others each count lies within +- that pair's undecided pixels; at most 2 % of a test's pairs may have
any.  tests/test_bop_vsd_host.py holds the scenes to that cap on the CPU.  Errors and recalls follow from the integers exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bop_reference as B
import vsd_cases as VC
import vsd_reference as VR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (400.0, 410.0, 130.3, 128.9)


def scorer_for(case, device, **kw):
    from casapose_amd.pose_estimation.bop_vsd import DeviceVsdScorer

    return DeviceVsdScorer([m[0] for m in case["meshes"]], [m[1] for m in case["meshes"]], device, near=VC.NEAR, far=VC.FAR, **kw)


def counts_of(scorer, case, **kw):
    return scorer.counts(case["est"], case["gt"], case["K"], case["obj"], case["img"], case["depths"], case["diameters"], **kw)


def call(hip_lib, device, planes, records, depth, cams, pairs, diameters, taus=VR.TAUS, delta=VR.DELTA, split=1):
    """the entry point itself over uploaded arrays -> (status, counts int32 [npairs, 2 + ntau] pre-filled with rubbish)"""
    import torch

    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(device)   # noqa: E731
    d = [up(planes, np.uint32), up(records, np.int32), up(depth, np.float32), up(cams, np.float64), up(pairs, np.int32), up(diameters, np.float64),
         up(taus, np.float64)]
    counts = torch.full((len(pairs), 2 + len(taus)), -7, dtype=torch.int32, device=device)
    H, W = planes.shape[1:]
    rc = hip_lib.cp_vsd_counts_i32(d[0].data_ptr(), d[1].data_ptr(), len(planes), H, W, d[2].data_ptr(), d[3].data_ptr(), len(depth), d[4].data_ptr(),
                                   d[5].data_ptr(), len(pairs), float(delta), d[6].data_ptr(), len(taus), split, counts.data_ptr(),
                                   torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    return rc, counts.cpu().numpy()


# ---- 1. rendered scenes through the scorer --------------------------------------------------------------------------------------------------
def test_ellipsoids_at_two_image_sizes(device):
    case = VC.ellipsoids()
    scorer = scorer_for(case, device)
    got = counts_of(scorer, case)
    assert got.dtype == np.int32 and got.shape == (30, 12)
    loose = VR.check_counts(got, case["want"], case["undecided"], "ellipsoids")
    print("ellipsoids: %d pairs, %d with undecided pixels" % (len(got), loose))
    assert scorer.last_renders == case["renders"] and scorer.last_chunks == 2 and scorer.last_dropped == case["dropped"]
    from casapose_amd.pose_estimation.bop_vsd import vsd_errors

    if loose == 0:
        assert np.array_equal(vsd_errors(got), np.stack([VR.errors_of(w) for w in case["want"]]))


def test_hand_worked_quad(device):
    case = VC.quad()
    got = counts_of(scorer_for(case, device), case)
    assert got.tolist() == [[96, 96, 96, 96, 0, 0, 0, 0, 0, 0, 0, 0]]


def test_repeatable_and_independent_of_chunking_and_split(device):
    """three 48 x 64 images: two calls give the same bytes; a workspace cap of one image's planes gives three launches and the same bytes; so does
    every number of blocks per pair"""
    base = VC.ellipsoids()
    first = np.flatnonzero(base["img"] == 0)
    case = dict(meshes=base["meshes"], est=np.concatenate([base["est"][first]] * 3), gt=np.concatenate([base["gt"][first]] * 3), K=base["K"][0],
                obj=np.concatenate([base["obj"][first]] * 3), img=np.repeat([0, 1, 2], len(first)), depths=[base["depths"][0]] * 3,
                diameters=np.concatenate([base["diameters"][first]] * 3))
    scorer = scorer_for(case, device)
    one = counts_of(scorer, case)
    assert scorer.last_chunks == 1 and scorer.last_renders == 45
    VR.check_counts(one, np.concatenate([base["want"][first]] * 3), np.concatenate([base["undecided"][first]] * 3), "three images")
    assert counts_of(scorer, case).tobytes() == one.tobytes()
    three = counts_of(scorer, case, workspace_cap=15 * 48 * 64 * 4)
    assert scorer.last_chunks == 3 and three.tobytes() == one.tobytes()
    for split in (2, 3, 64):
        assert counts_of(scorer, case, split=split).tobytes() == one.tobytes(), split
    with pytest.raises(ValueError, match="workspace cap"):
        counts_of(scorer, case, workspace_cap=15 * 48 * 64 * 4 - 1)


def test_an_image_with_300_render_slots(device):
    case = VC.many_slots()
    scorer = scorer_for(case, device)
    got = counts_of(scorer, case)
    loose = VR.check_counts(got, case["want"], case["undecided"], "300 slots")
    print("300 slots: %d pairs, %d with undecided pixels" % (len(got), loose))
    assert scorer.last_renders == 300 and scorer.last_chunks == 1


# ---- 2. the entry point over hand-made planes ---------------------------------------------------------------------------------------------
def tile_boxes(T):
    """(H, W, boxes, pairs): every box twice, as planes p and p + n with different contents.  Boxes 0-8: T - 1, T and T + 1 pixels as one row and
    as one column, and two rows of ceil(n / 2); 9-11: across the top-left corner, the bottom-right corner, the left and right border; 12, 13:
    disjoint rectangles; 14, 15: empty"""
    H = W = T + 3
    sizes = (T - 1, T, T + 1)
    boxes = [(1, 2, n - 1, 0) for n in sizes] + [(2, 1, 0, n - 1) for n in sizes] + [(3, 5, (n + 1) // 2 - 1, 1) for n in sizes]
    boxes += [(-4, -3, 20, 9), (W - 7, H - 5, 30, 30), (-2, 40, W + 10, 3), (10, 10, 30, 20), (60, 50, 40, 33), (-1, -1, -1, -1), (-1, -1, -1, -1)]
    n = len(boxes)
    pairs = [(0, p, p + n, 0) for p in range(n)]
    pairs += [(0, 0, 3, 0), (0, 8, 5 + n, 0), (0, 9, 10, 0), (0, 12, 13, 0), (0, 13, 12 + n, 0), (0, 14, 12, 0), (0, 13, 15, 0), (0, 15, 14 + n, 0)]
    return H, W, boxes + boxes, pairs


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("ntau", [1, 10])
def test_union_boxes_around_the_tile(device, hip_lib, ntau, split):
    T = hip_lib.cp_vsd_tile()
    H, W, boxes, pairs = tile_boxes(T)
    planes, records, depth = VC.crafted(H, W, boxes, seed=3)
    taus = VR.TAUS[:ntau] if ntau > 1 else [0.3]
    diam = np.linspace(150.0, 400.0, len(pairs))
    want, und = VC.crafted_reference(planes, depth, [CAM], pairs, diam, taus=taus)
    rc, got = call(hip_lib, device, planes, records, depth, [CAM], pairs, diam, taus=taus, split=split)
    assert rc == 0, hip_lib.cp_last_error()
    assert want[:9, 0].min() > T // 8 and want[:14, 1].min() > 8 and (want[:14, 2] > 0).all()      # the cases hold what they mean to hold
    assert want[15].tolist() == [0] * (2 + ntau) and want[-1].tolist() == [0] * (2 + ntau) and want[19, 1] == 0 and want[19, 0] > 0
    VR.check_counts(got, want, und, "tile boxes, ntau %d, split %d" % (ntau, split))


def test_more_pairs_than_a_16_bit_grid_dimension(device, hip_lib):
    """70 000 pairs over four planes of an 8 x 8 image, among them pairs with an index out of range, which leave zeros"""
    planes, records, depth = VC.crafted(8, 8, [(0, 0, 7, 7), (2, 1, 4, 5), (-1, 3, 5, 9), (5, 5, 1, 1)], seed=9, images=2)
    rng = np.random.default_rng(1)
    pairs = np.stack([rng.integers(0, 2, 70000), rng.integers(0, 4, 70000), rng.integers(0, 4, 70000), np.zeros(70000, np.int64)], axis=1)
    pairs[1000] = (2, 0, 0, 0)
    pairs[2000] = (0, 4, 0, 0)
    pairs[3000] = (0, 0, -1, 0)
    pairs[69999] = (-1, 0, 0, 0)
    diam = np.full(70000, 250.0)
    want, und = VC.crafted_reference(planes, depth, [(50.0, 50.0, 3.6, 3.4)] * 2, pairs, diam)
    rc, got = call(hip_lib, device, planes, records, depth, [(50.0, 50.0, 3.6, 3.4)] * 2, pairs, diam)
    assert rc == 0, hip_lib.cp_last_error()
    assert (want[:, 0] > 0).sum() > 60000 and (want[[1000, 2000, 3000, 69999]] == 0).all() and want[69998].any()
    VR.check_counts(got, want, und, "70 000 pairs")


def test_refusals_by_name(device, hip_lib):
    planes, records, depth = VC.crafted(8, 8, [(0, 0, 7, 7)], seed=2)
    rc, got = call(hip_lib, device, planes, records, depth, [CAM], [(0, 0, 0, 0)], [100.0], taus=[0.01 * i for i in range(33)])
    assert rc == -1 and b"ntau" in hip_lib.cp_last_error() and (got == -7).all()          # nothing was written
    rc, got = call(hip_lib, device, planes, records, depth, [CAM], [(0, 0, 0, 0)], [100.0], taus=[0.01 * i for i in range(32)])
    assert rc == 0 and got[0, 0] == got[0, 1] == got[0, 2] > 0 and got[0, 3:].tolist() == [0] * 31      # e == g: cost 0 reaches tau 0 = 0.0 only
    rc, got = call(hip_lib, device, planes, records, depth, [CAM], [(0, 0, 0, 0)], [0.0])
    assert rc == 0 and got.tolist() == [[0] * 12]                                          # a diameter that is not > 0
    case = VC.quad()
    with pytest.raises(ValueError, match="ntau"):
        counts_of(scorer_for(case, device), case, taus=[0.01] * 33)


# ---- 3. the script, end to end --------------------------------------------------------------------------------------------------------------
def test_score_script_with_vsd_end_to_end(device, tmp_path):
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
    info = {str(o): {"diameter": 2.0 * max(a)} for o, a in TM.OBJECTS.items()}
    (scene_dir / "scene_camera.json").write_text(json.dumps({str(i): {"cam_K": K.reshape(-1).tolist(), "depth_scale": 0.1} for i in range(2)}))
    ids = [1, 5]
    ref = VR.Scene([meshes[o] for o in ids], DEFAULT_NEAR, DEFAULT_FAR)
    # sensor depth in tenths of a millimetre: the nearest ground truth over a background, an occluder over the right of image 0, a patch of zeros
    sensors = []
    for im in range(2):
        inst = [(ids.index(o), 1, P) for o, P in poses[im]]
        d = VC.sensor_depth(ref, inst, cam, H, W, (64, 30, 90, 70, 380.0) if im == 0 else (0, 0, 3, 3, 380.0), (40, 40, 47, 46))
        raw = np.rint(d.astype(np.float64) * 10.0).astype(np.uint16)
        Image.fromarray(raw).save(scene_dir / "depth" / ("%06d.png" % im))
        sensors.append(raw.astype(np.float32) * np.float32(0.1))
    # estimates: image 0 both objects a little off, image 1 object 5 far off in depth and object 1 not found
    def moved(P, dt, turn):
        return np.hstack([TM.RR.rotation((1, 1, 0), turn) @ P[:, :3], P[:, 3:] + np.asarray(dt, np.float64).reshape(3, 1)]).astype(np.float32)

    gt_of = [{o: P for o, P in poses[im]} for im in range(2)]
    est = [{1: moved(gt_of[0][1], (1.5, -1.0, 3.0), 0.02), 5: moved(gt_of[0][5], (-2.0, 1.0, 10.0), 0.05)},
           {1: np.zeros((3, 4), np.float32), 5: moved(gt_of[1][5], (3.0, 2.0, 37.0), 0.0)}]
    out_dir = str(tmp_path / "run") + "/"
    for im in range(2):
        write_poses(np.stack([gt_of[im][o].astype(np.float32) for o in ids])[:, None], np.stack([est[im][o] for o in ids]), TM.NAMES, "000002_rgb_%06d" % im, out_dir)
    # the file is the interface: it holds the shortest decimal of every fp32 number, which read as fp64 is not that fp32 number; the renders
    # take the fp64 poses as they are read
    in_file = read_bop_results(out_dir + "bop_evaluation.csv")["pose"]
    assert np.array_equal(in_file.astype(np.float32), np.stack([est[im][o] for im in range(2) for o in ids]))
    rows = [(2, im, o, 0.0 if not est[im][o].any() else 1.0, in_file[2 * im + k]) for im in range(2) for k, o in enumerate(ids)]
    read = {(im, o): in_file[2 * im + k] for im in range(2) for k, o in enumerate(ids)}

    # the reference, on the same numbers
    gts = {(2, im): [{"id": o, "R": P[:, :3], "t": P[:, 3]} for o, P in poses[im]] for im in range(2)}
    diam = {int(o): e["diameter"] for o, e in info.items()}
    want, pairs = B.score(rows, gts, {k: K for k in gts}, {o: meshes[o][0] for o in ids}, {o: B.symmetry_set({}) for o in ids}, diam, None, 640.0)
    assert want["targets"] == 4 and len(pairs) == 3
    for obj, e3, e2 in pairs:
        assert all(abs(e3 - t * diam[obj]) >= 0.01 * t * diam[obj] for t in B.MSSD_T) and all(abs(e2 - t) >= 0.01 * t for t in B.MSPD_T), (obj, e3, e2)
    groups = []
    for im in range(2):
        for o, P in poses[im]:
            if est[im][o].any():
                c, u = ref.counts(ids.index(o), read[(im, o)], P, cam, sensors[im], diam[o])
                assert u == 0, (im, o)
                groups.append((o, 1, VR.errors_of(c).reshape(1, 1, 10)))
            else:
                groups.append((o, 1, np.zeros((0, 1, 10))))
    vsd = VR.recall(groups)
    assert 0.0 < vsd["AR_VSD"] < 1.0 and len({tuple(r) for r in vsd["recall_vsd"]}) > 1

    command = [sys.executable, os.path.join(ROOT, "util_scripts", "bop_score.py"), "--result_file", out_dir + "bop_evaluation.csv", "--dataset_path",
               str(root), "--split", "test", "--model_folder", "models", "--image_width", "640"]
    out_json = str(tmp_path / "scores.json")
    r = subprocess.run(command + ["--out", out_json, "--vsd"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "AR_VSD" in r.stdout and " AR " in r.stdout and "AR_MSSD_MSPD" not in r.stdout and "VSD not computed" not in r.stdout
    with open(out_json) as f:
        got = json.load(f)
    for g, w, v in [(got, want, vsd)] + [(got["objects"][o], want["objects"][o], vsd["objects"][o]) for o in ("1", "5")]:
        assert g["AR_VSD"] == v["AR_VSD"] and g["recall_vsd"] == v["recall_vsd"] and g["targets"] == v["targets"] == w["targets"]
        assert g["AR_MSSD"] == w["AR_MSSD"] and g["AR_MSPD"] == w["AR_MSPD"]
        assert g["AR"] == (v["AR_VSD"] + w["AR_MSSD"] + w["AR_MSPD"]) / 3.0
    assert got["pairs"] == 3

    plain_json = str(tmp_path / "plain.json")
    p = subprocess.run(command + ["--out", plain_json], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    last = p.stdout.strip().splitlines()[-1]
    assert last == ("all objects: targets %6d  AR_MSSD %.4f  AR_MSPD %.4f  AR_MSSD_MSPD %.4f  (%d pairs, image width %d; VSD not computed)"
                    % (4, want["AR_MSSD"], want["AR_MSPD"], want["AR_MSSD_MSPD"], 3, 640))
    with open(plain_json) as f:
        plain = json.load(f)
    assert not {"AR", "AR_VSD", "recall_vsd", "vsd_taus", "vsd_thresholds"} & (set(plain) | set(plain["objects"]["1"]))
    assert plain == {k: v for k, v in got.items() if k not in ("AR", "AR_VSD", "recall_vsd", "vsd_taus", "vsd_thresholds", "objects")} | {
        "objects": {o: {k: v for k, v in e.items() if k not in ("AR", "AR_VSD", "recall_vsd")} for o, e in got["objects"].items()}}
