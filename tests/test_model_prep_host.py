"""Keypoints and models_info from the meshes on the CPU: `cp_model_prep_host_f32` (the host twin of `cp_model_prep_f32`: csrc/model_math.h run
serially) against a NumPy fp64 restatement of that header's rules, and what is built on it: ModelPrep, the two files, the converter's
keypoints / models_info = "generate" and the command lines.

The restatement is a chunked brute-force maximum over all vertex pairs and a plain farthest-point loop with np.argmax, whose first-maximum rule is
the lowest-index rule.  NumPy's fp64 products and sums are rounded one by one, like the header's (no FMA), so everything is compared bit for bit:
squared diameter, box, keypoints, indices, status."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_masks_twin_host as T
from casapose_amd._lib import CasaposeHipError
from casapose_amd.data_handler import bop_converter as BC
from casapose_amd.data_handler import model_prep as MP
from casapose_amd.data_handler.vectorfield_dataset import read_vertices

ROOT = T.ROOT
TILE = 256   # cp_model::TILE of csrc/model_math.h


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def d2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def reference(vertices, K):
    """one object's (diameter_sq, box, keypoints, indices, status) from float32 vertices [N, 3]"""
    v32 = np.asarray(vertices, np.float32)
    v = v32.astype(np.float64)
    best = 0.0
    for lo in range(0, len(v), 256):
        best = max(best, float(d2(v[lo:lo + 256, None, :], v[None, :, :]).max()))
    box = np.concatenate([v32.min(0), v32.max(0)])
    c = 0.5 * (box[:3].astype(np.float64) + box[3:].astype(np.float64))
    keypoints, indices, status = np.zeros((K, 3), np.float32), np.zeros(K - 1, np.int32), np.int32(MP.ST_OK)
    keypoints[0] = c.astype(np.float32)
    m = d2(v, c)
    for k in range(1, K):
        j = int(np.argmax(m))
        if not m[j] > 0:
            status = np.int32(MP.ST_TOO_FEW)
            break
        keypoints[k], indices[k - 1] = v32[j], j
        m = np.minimum(m, d2(v, v[j]))
    return dict(diameter_sq=np.float64(best), box=box, keypoints=keypoints, indices=indices, status=status)


# ---- the cases: {name: ({object: float32 vertices}, K)} -----------------------------------------------------------------------------------------
def cloud(n, seed):
    """normal points scaled by 50 and shifted by +1000 on every axis: a zero vertex taken for a point would move the box, the diameter and a pick"""
    return (np.random.default_rng(seed).normal(size=(n, 3)) * 50.0 + 1000.0).astype(np.float32)


def with_extremes(n, i, j, seed):
    """a cloud whose two farthest vertices are vertices i and j (2000 apart on a diagonal, the cloud itself spans a few hundred)"""
    v = cloud(n, seed)
    v[i], v[j] = (0.0 + 423.0, 1000.0, 1000.0), (2423.0, 1000.0, 1000.0)
    return v


def cube():
    return np.array([[1000.0 + (1 if i & 4 else -1), 1000.0 + (1 if i & 2 else -1), 1000.0 + (1 if i & 1 else -1)] for i in range(8)], np.float32)


def build_cases():
    cases = {}
    for n in (1, 2, 63, 64, 65, 257, 1000, 4099):
        cases["n%d" % n] = ({0: cloud(n, n)}, {1: 2, 2: 3}.get(n, 9))   # 1 and 2 vertices cannot give nine keypoints: see the refusals
    cases["three_objects"] = ({"a": cloud(65, 1), "b": cloud(4099, 2), "c": cloud(7, 3)}, 6)   # the largest not last
    cases["extremes_first_last"] = ({0: with_extremes(1000, 0, 999, 4)}, 9)
    cases["extremes_one_tile"] = ({0: with_extremes(1000, TILE + 3, 2 * TILE - 2, 5)}, 9)
    cases["extremes_adjacent_tiles"] = ({0: with_extremes(1000, 2 * TILE - 1, 2 * TILE, 6)}, 9)
    cases["cube"] = ({0: cube()}, 9)
    cases["cube_doubled"] = ({0: np.repeat(cube(), 2, axis=0)}, 9)
    for K in (2, 9, 16, 32):
        cases["k%d" % K] = ({0: cloud(300, 7)}, K)
    return cases


CASES = build_cases()


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """{array: [objects, ...]} of a case, computed once, shared, never modified"""
    meshes, K = CASES[name]
    per = [reference(meshes[o], K) for o in meshes]
    out = {k: np.stack([r[k] for r in per]) for k in per[0]}
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_same_bits(got, want, where):
    for key in ("status", "indices", "box", "keypoints", "diameter_sq"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (where, key, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (where, key, g, w)


@functools.lru_cache(maxsize=None)
def host_outputs(name):
    meshes, K = CASES[name]
    out = MP.ModelPrep(None).outputs(meshes, K, host=True)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_the_numpy_restatement(name):
    meshes, K = CASES[name]
    got, want = host_outputs(name), reference_of(name)
    assert_same_bits(got, want, name)
    assert (got["status"] == MP.ST_OK).all() or name == "n1"
    assert got["counts"].tolist() == [len(v) for v in meshes.values()]


def test_cases_hold_what_they_mean_to_hold():
    for name, (i, j) in (("extremes_first_last", (0, 999)), ("extremes_one_tile", (TILE + 3, 2 * TILE - 2)),
                         ("extremes_adjacent_tiles", (2 * TILE - 1, 2 * TILE))):
        want = reference_of(name)
        assert want["diameter_sq"][0] == 2000.0 ** 2 and {int(want["indices"][0, 0]), int(want["indices"][0, 1])} == {i, j}
    assert (TILE + 3) // TILE == (2 * TILE - 2) // TILE and (2 * TILE - 1) // TILE + 1 == (2 * TILE) // TILE
    one = reference_of("n1")
    assert one["diameter_sq"][0] == 0.0 and one["status"][0] == MP.ST_TOO_FEW and (one["keypoints"][0, 0] == CASES["n1"][0][0][0]).all()
    three = reference_of("three_objects")
    assert len(set(three["diameter_sq"].tolist())) == 3 and (three["box"][:, :3] > 700).all()


def test_cube_ties_go_to_the_lowest_index():
    """Every corner is sqrt(3) from the centre and at least 2 from every other corner: at every pick all remaining corners tie at 3 and the lowest
    index wins, so the picks are the corners in index order; four diagonals tie for the diameter, 12 = (2 sqrt(3))^2."""
    out = host_outputs("cube")
    assert out["indices"][0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and out["diameter_sq"][0] == 12.0
    assert np.array_equal(out["keypoints"][0, 1:], cube()) and out["keypoints"][0, 0].tolist() == [1000.0, 1000.0, 1000.0]
    doubled = host_outputs("cube_doubled")   # vertex 2 i and 2 i + 1 are corner i: the even copies win
    assert doubled["indices"][0].tolist() == [0, 2, 4, 6, 8, 10, 12, 14] and doubled["diameter_sq"][0] == 12.0
    assert np.array_equal(doubled["keypoints"], out["keypoints"])


def test_prepare_host_returns_the_documented_fields():
    meshes, K = CASES["three_objects"]
    results, want = MP.ModelPrep(None).prepare_host(meshes, K), reference_of("three_objects")
    assert list(results) == ["a", "b", "c"]
    for i, obj in enumerate(results):
        r = results[obj]
        assert r["keypoints"].dtype == np.float32 and r["keypoints"].shape == (K, 3) and r["keypoint_indices"].shape == (K - 1,)
        assert r["keypoints"].tobytes() == want["keypoints"][i].tobytes() and r["keypoint_indices"].tolist() == want["indices"][i].tolist()
        assert isinstance(r["diameter"], float) and r["diameter"] == float(np.sqrt(want["diameter_sq"][i]))
        assert r["min"].tobytes() == want["box"][i, :3].tobytes()
        assert np.array_equal(r["size"], want["box"][i, 3:].astype(np.float64) - want["box"][i, :3].astype(np.float64))
        assert np.array_equal(r["keypoints"][1:], meshes[obj][r["keypoint_indices"]])   # the picks are vertices, unchanged
    # the keypoints of an object do not depend on what else is in the call
    alone = MP.ModelPrep(None).prepare_host({"b": meshes["b"]}, K)["b"]
    assert alone["keypoints"].tobytes() == results["b"]["keypoints"].tobytes() and alone["diameter"] == results["b"]["diameter"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_object_and_the_reason():
    prep = MP.ModelPrep(None)
    same = np.full((40, 3), 1000.0, np.float32)
    out = prep.outputs({"flat": same}, 9, host=True)
    assert out["diameter_sq"][0] == 0.0 and out["status"][0] == MP.ST_TOO_FEW and (out["keypoints"][0, 1:] == 0).all() and (out["indices"] == 0).all()
    assert out["keypoints"][0, 0].tolist() == [1000.0, 1000.0, 1000.0] and out["box"][0].tolist() == [1000.0] * 6
    with pytest.raises(ValueError, match="flat.*too few distinct vertices"):
        prep.prepare_host({"ok": cloud(20, 1), "flat": same}, 9)
    five = np.concatenate([cloud(5, 2), cloud(5, 2)])   # ten vertices, five distinct: K - 1 = 6 picks cannot be made, 5 can
    assert len(prep.prepare_host({"five": five}, 6)["five"]["keypoint_indices"]) == 5
    out = prep.outputs({"five": five}, 7, host=True)
    assert out["status"][0] == MP.ST_TOO_FEW and (out["indices"][0, :5] < 5).all() and out["indices"][0, 5] == 0 and (out["keypoints"][0, 6] == 0).all()
    assert_same_bits(out, {k: v[None] for k, v in reference(five, 7).items()}, "five")
    with pytest.raises(ValueError, match="five.*too few distinct vertices"):
        prep.prepare_host({"five": five}, 7)
    for K in (1, 33):
        with pytest.raises(ValueError, match="no_points"):
            prep.prepare_host({"ok": cloud(20, 1)}, K)
    empty = prep.outputs({"ok": cloud(20, 1), "none": np.zeros((0, 3), np.float32), "after": cloud(9, 3)}, 4, host=True)
    assert empty["status"].tolist() == [MP.ST_OK, MP.ST_BAD_COUNT, MP.ST_OK] and (empty["box"][1] == 0).all() and empty["diameter_sq"][1] == 0.0
    assert_same_bits({k: v[2:] for k, v in empty.items()}, {k: v[None] for k, v in reference(cloud(9, 3), 4).items()}, "after an empty object")
    with pytest.raises(ValueError, match="none.*0 vertices"):
        prep.prepare_host({"none": np.zeros((0, 3), np.float32)}, 4)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        prep.prepare_host({"flat": np.zeros(9, np.float32)}, 4)
    with pytest.raises(CasaposeHipError, match="without a device"):
        prep.prepare({"ok": cloud(20, 1)}, 4)


def test_a_requested_device_never_falls_back_to_the_host(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(CasaposeHipError, match="needs a ROCm GPU"):
        MP.ModelPrep("cuda:0")
    with pytest.raises(CasaposeHipError, match="needs a ROCm GPU"):
        MP.model_prep_for("device")


def test_library_refuses_bad_arguments(hip_lib):
    v = cloud(20, 1)
    offsets, counts = np.zeros(1, np.int64), np.array([20], np.int32)
    diam, box, kps, idx, status = np.zeros(1), np.zeros(6, np.float32), np.zeros(27, np.float32), np.zeros(8, np.int32), np.zeros(1, np.int32)
    size = hip_lib.cp_model_prep_workspace_bytes(1, 20)
    assert size == 2 * 8 + 20 * 8
    ws = np.zeros(size // 8, np.int64)
    ok = [v.ctypes.data, 20, offsets.ctypes.data, counts.ctypes.data, 1, 9, diam.ctypes.data, box.ctypes.data, kps.ctypes.data, idx.ctypes.data,
          status.ctypes.data, ws.ctypes.data, size]
    assert hip_lib.cp_model_prep_host_f32(*ok) == 0 and status[0] == 0 and diam[0] > 0
    for at, bad, word in ((5, 1, b"no_points"), (5, 33, b"no_points"), (4, 0, b"objects"), (4, 1025, b"objects"), (1, -1, b"total"),
                          (12, size - 1, b"workspace"), (0, None, b"null"), (10, None, b"null"), (2, offsets.ctypes.data + 4, b"8-byte")):
        args = list(ok)
        args[at] = bad
        assert hip_lib.cp_model_prep_host_f32(*args) == -1 and word in hip_lib.cp_last_error(), word
        assert hip_lib.cp_model_prep_f32(*args, None) == -1 and word in hip_lib.cp_last_error(), word   # refused before any launch: no GPU needed
    assert hip_lib.cp_model_prep_workspace_bytes(0, 20) == 0 and hip_lib.cp_model_prep_workspace_bytes(1025, 20) == 0
    assert hip_lib.cp_model_prep_workspace_bytes(1, -1) == 0
    # a vertex range that leaves the array, and a count above 2^22, are a status: nothing of the object is read
    for off, n in ((15, 20), (-1, 5), (0, (1 << 22) + 1)):
        offsets[0], counts[0] = off, n
        assert hip_lib.cp_model_prep_host_f32(*ok) == 0 and status[0] == MP.ST_BAD_COUNT and diam[0] == 0.0 and (kps == 0).all()


# ---- the two files ---------------------------------------------------------------------------------------------------------------------------------
def test_keypoints_ply_round_trip(tmp_path):
    kp = np.concatenate([cloud(8, 9), np.array([[1e-7, -3.4028235e38, 0.1]], np.float32)])
    MP.write_keypoints_ply(str(tmp_path / "k.ply"), kp)
    lines = open(tmp_path / "k.ply").read().split("\n")
    assert lines[:7] == ["ply", "format ascii 1.0", "element vertex 9", "property float x", "property float y", "property float z", "end_header"]
    back = read_vertices(str(tmp_path / "k.ply"))
    assert back.shape == (9, 3) and back.astype(np.float32).tobytes() == kp.tobytes()
    # the layout of the reference's own keypoint files
    shipped = open(os.path.join(ROOT, "tests", "golden", "ref_data", "lm_models_eval", "obj_000001_keypoints.ply")).read().split("\n")
    assert [l.strip() for l in shipped[:8] if not l.startswith("comment")] == lines[:7]


def test_models_info_carries_other_fields_over(tmp_path):
    results = MP.ModelPrep(None).prepare_host({"obj_000001": cloud(50, 1), "obj_000005": cloud(60, 2)}, 9)
    sym = [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]]
    existing = {"1": {"diameter": 1.0, "min_x": -5.0, "symmetries_discrete": sym}, "7": {"diameter": 2.0, "symmetries_continuous": [{"axis": [0, 0, 1]}]}}
    wrote = MP.write_models_info(str(tmp_path / "models_info.json"), results, existing)
    info = json.load(open(tmp_path / "models_info.json"))
    assert info == wrote and list(info) == ["obj_000001", "obj_000005"]
    one = info["obj_000001"]
    assert list(one) == ["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "symmetries_discrete"]
    assert one["symmetries_discrete"] == sym and one["diameter"] == results["obj_000001"]["diameter"] and one["min_x"] == float(results["obj_000001"]["min"][0])
    assert one["size_z"] == float(results["obj_000001"]["size"][2]) and "symmetries_discrete" not in info["obj_000005"]
    again = MP.write_models_info(str(tmp_path / "again.json"), results, info)   # found under the stem as well
    assert again == info and MP.write_models_info(str(tmp_path / "none.json"), results)["obj_000001"].keys() == {"diameter", "min_x", "min_y", "min_z",
                                                                                                               "size_x", "size_y", "size_z"}


# ---- the converter ---------------------------------------------------------------------------------------------------------------------------------
def write_bare_tree(root):
    """test_masks_twin_host's BOP tree without keypoint files and without models_info.json: what a BOP archive other than LM's holds"""
    meshes, poses = T.write_bop_tree(root)
    for obj in T.OBJECTS:
        os.remove(root / "models" / ("obj_%06d_keypoints.ply" % obj))
    os.remove(root / "models" / "models_info.json")
    return meshes, poses


def generate_settings(**kw):
    return T.settings_for(**dict(dict(keypoints="generate", models_info="generate"), **kw))


def check_generated_tree(out, meshes, renderer="host"):
    """the converted tree against ModelPrep's own results of the meshes: the files, and what the reader makes of them"""
    prep = MP.model_prep_for(renderer)
    want = prep.run({"obj_%06d" % o: meshes[o][0] for o in sorted(meshes)}, 9, renderer)
    info = json.load(open(out / "models" / "models_info.json"))
    assert list(info) == T.NAMES
    for name in T.NAMES:
        kp = read_vertices(str(out / "models" / name / (name + "_keypoints.ply")))
        assert kp.astype(np.float32).tobytes() == want[name]["keypoints"].tobytes()
        assert info[name]["diameter"] == want[name]["diameter"] and info[name]["size_y"] == float(want[name]["size"][1])
        assert os.path.isfile(out / "models" / name / (name + ".ply"))
    b = T.read_back(out)
    poses = T.bop_poses()
    K = np.array([[T.BOP_CAM[0], 0, T.BOP_CAM[2]], [0, T.BOP_CAM[1], T.BOP_CAM[3]], [0, 0, 1]])
    for i in range(2):
        for obj, P in poses[i]:
            name = "obj_%06d" % obj
            o = T.NAMES.index(name)
            assert np.array_equal(b["keypoints3d"][i, o, 0].numpy(), want[name]["keypoints"])
            assert float(b["diameters"][i, o, 0, 0]) == np.float32(want[name]["diameter"])
            uv, _ = BC.project(want[name]["keypoints"].astype(np.float64), K, P)
            assert np.allclose(b["target_vert"][i, o, 0].numpy(), uv[:, ::-1], atol=1e-3)   # the generated keypoints feed the frame JSONs
    return want


def test_converter_generates_what_a_bare_bop_tree_lacks(tmp_path):
    meshes, _ = write_bare_tree(tmp_path / "bop")
    before = sorted(os.listdir(tmp_path / "bop" / "models"))
    with pytest.raises(FileNotFoundError, match="models_info.json"):   # the defaults still fail as before: no models_info.json
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o1"), T.settings_for(), image_folder="test")
    json.dump({"1": {"diameter": 80.0}, "5": {"diameter": 90.0}}, open(tmp_path / "bop" / "models" / "models_info.json", "w"))
    with pytest.raises(IndexError):   # and with it, at the keypoint files paired by position
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o2"), T.settings_for(), image_folder="test")
    with pytest.raises(FileNotFoundError, match="obj_000001_keypoints.ply"):   # models_info alone generated: the keypoint file is asked for by name
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o3"), generate_settings(keypoints="file"), image_folder="test")
    with pytest.raises(ValueError, match="keypoints"):
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o4"), generate_settings(keypoints="guess"), image_folder="test")
    os.remove(tmp_path / "bop" / "models" / "models_info.json")
    BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "out"), generate_settings(), model_folder="models", model_folder_out="models",
                     image_folder="test")
    assert sorted(os.listdir(tmp_path / "bop" / "models")) == before   # nothing is written into the input dataset
    want = check_generated_tree(tmp_path / "out", meshes)
    assert all(r["diameter"] > 60 for r in want.values())
    # keypoints from files, models_info generated: the existing entry's other fields are carried over
    for obj, axes in T.OBJECTS.items():
        T.write_ply(tmp_path / "bop" / "models" / ("obj_%06d_keypoints.ply" % obj), T.keypoints_of(axes))
    json.dump({"1": {"diameter": 1.0, "symmetries_discrete": [[1.0] * 16]}}, open(tmp_path / "bop" / "models" / "models_info.json", "w"))
    BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "mixed"), generate_settings(keypoints="file"), image_folder="test")
    info = json.load(open(tmp_path / "mixed" / "models" / "models_info.json"))
    assert info["obj_000001"]["symmetries_discrete"] == [[1.0] * 16] and info["obj_000001"]["diameter"] == want["obj_000001"]["diameter"]
    kp = read_vertices(str(tmp_path / "mixed" / "models" / "obj_000005" / "obj_000005_keypoints.ply"))
    assert np.allclose(kp, T.keypoints_of(T.OBJECTS[5]))


def test_command_lines(tmp_path):
    meshes, _ = write_bare_tree(tmp_path / "bop")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "util_scripts", "dataset_converter.py"), "--dataset_path", str(tmp_path / "bop"),
                        "--dataset_path_out", str(tmp_path / "out"), "--image_folder", "test", "--width", str(T.W), "--height", str(T.H), "--mask", "render",
                        "--gt_info", "render", "--renderer", "host", "--copy_meshes", "--keypoints", "generate", "--models_info", "generate",
                        "--no_points", "9"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = check_generated_tree(tmp_path / "out", meshes)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "util_scripts", "make_keypoints.py"), "--model_folder", str(tmp_path / "bop" / "models"),
                        "--out", str(tmp_path / "kp"), "--no_points", "5", "--renderer", "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.load(open(tmp_path / "kp" / "models_info.json"))
    for name in T.NAMES:
        kp = read_vertices(str(tmp_path / "kp" / name / (name + "_keypoints.ply"))).astype(np.float32)
        assert kp.tobytes() == want[name]["keypoints"][:5].tobytes()   # farthest-point samples are a prefix of a longer run's
        assert info[name]["diameter"] == want[name]["diameter"] and os.path.isfile(tmp_path / "kp" / name / (name + ".ply"))
