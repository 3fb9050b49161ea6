"""The host side of BOP's VSD (casapose_amd/pose_estimation/bop_vsd.py, util_scripts/bop_score.py --vsd) without a GPU: the error from the
integers, matching and recall, the depth reader, `score` with and without a VSD scorer, the script's refusal of a missing depth image, the new
entry points' declarations -- and the reference of the GPU tests on its own: tests/vsd_reference.py against a case worked by hand, and the share of
pairs with undecided pixels in every scene tests/test_gpu_vsd.py scores."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vsd_cases as VC
import vsd_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_bop19s():
    from casapose_amd.pose_estimation import bop_scores as S
    from casapose_amd.pose_estimation import bop_vsd as V

    assert V.VSD_DELTA == 15.0
    assert V.VSD_TAUS == tuple(0.05 * i for i in range(1, 11)) == S.MSSD_THRESHOLDS == V.VSD_THRESHOLDS
    assert V.DEFAULT_NEAR > 0 and V.DEFAULT_FAR > V.DEFAULT_NEAR


def test_vsd_errors_from_hand_made_counts():
    from casapose_amd.pose_estimation.bop_vsd import vsd_errors

    counts = np.array([[100, 80, 80, 40, 0],       # (80 + 20) / 100, (40 + 20) / 100, 20 / 100
                       [0, 0, 0, 0, 0],            # an empty union
                       [50, 0, 0, 0, 0],           # disjoint: 1
                       [7, 7, 0, 0, 0],            # identical: 0
                       [3, 1, 1, 1, 0]], np.int32)
    e = vsd_errors(counts)
    assert e.dtype == np.float64 and e.shape == (5, 3)
    assert e.tolist() == [[1.0, 0.6, 0.2], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 2 / 3]]
    assert vsd_errors(np.zeros((0, 12), np.int32)).shape == (0, 10)
    big = vsd_errors(np.array([[2 ** 28, 2 ** 28, 2 ** 28]], np.int32))     # no int32 overflow in count + union - intersection
    assert big.tolist() == [[1.0]]
    with pytest.raises(ValueError):
        vsd_errors(np.zeros((3, 2), np.int32))


def test_match_and_recall_vsd_worked_by_hand():
    """Two objects, two taus.  Object 1: one image with two targets, two estimates, two instances; object 2: one image, one target, no estimate,
    and one image with one target and one estimate.
      object 1, tau 0: e = [[0.12, 0.90], [0.30, 0.07]]: estimate 0 takes instance 0 when 0.12 < theta (theta >= 0.15), estimate 1 takes instance 1
                       when 0.07 < theta (theta >= 0.10): matches per theta = 0, 1, 2, 2, 2, 2, 2, 2, 2, 2 -> recalls / 2
      object 1, tau 1: e = [[0.45, 1.0], [0.45, 0.50]]: estimate 0 takes instance 0 at theta = 0.50 (0.45 < 0.5); estimate 1's best free
                       instance is 1 with 0.50, never below theta: matches = 0 x 9, 1
      object 2: e = 0.26 at tau 0 (theta >= 0.30: five thetas), 0.0 at tau 1 (all ten), over two targets"""
    from casapose_amd.pose_estimation.bop_vsd import match_and_recall_vsd

    g1 = np.array([[[0.12, 0.45], [0.90, 1.0]], [[0.30, 0.45], [0.07, 0.50]]])
    out = match_and_recall_vsd([(1, 2, g1), (2, 1, np.zeros((0, 1, 2))), (2, 1, np.array([[[0.26, 0.0]]]))])
    o1, o2 = out["objects"]["1"], out["objects"]["2"]
    assert o1["targets"] == 2 and o2["targets"] == 2 and out["targets"] == 4
    assert o1["recall_vsd"] == [[0.0, 0.5] + [1.0] * 8, [0.0] * 9 + [0.5]]
    assert o2["recall_vsd"] == [[0.0] * 5 + [0.5] * 5, [0.5] * 10]
    assert o1["AR_VSD"] == (0.5 + 8.0 + 0.5) / 20.0 and o2["AR_VSD"] == (2.5 + 5.0) / 20.0
    assert out["recall_vsd"] == [[0.0, 0.25, 0.5, 0.5, 0.5] + [0.75] * 5, [0.25] * 9 + [0.5]]
    assert out["AR_VSD"] == sum(sum(r) for r in out["recall_vsd"]) / 20.0
    assert out["vsd_thresholds"] == [0.05 * i for i in range(1, 11)]
    empty = match_and_recall_vsd([])
    assert empty["targets"] == 0 and empty["AR_VSD"] == 0.0 and empty["objects"] == {}


def test_read_depth_round_trip(tmp_path):
    from PIL import Image

    from casapose_amd.pose_estimation.bop_vsd import read_depth

    raw = np.array([[0, 1, 9999], [65535, 12345, 4000]], np.uint16)
    Image.fromarray(raw).save(tmp_path / "000000.png")
    with Image.open(tmp_path / "000000.png") as im:
        assert im.mode in ("I;16", "I;16B", "I")
    d = read_depth(str(tmp_path / "000000.png"), 0.1)
    assert d.dtype == np.float32 and d.shape == (2, 3)
    assert np.array_equal(d, raw.astype(np.float32) * np.float32(0.1)) and d[0, 0] == 0.0 and abs(float(d[1, 1]) - 1234.5) < 1e-3
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match="one channel"):
        read_depth(str(tmp_path / "rgb.png"), 1.0)


# ---- score with and without VSD ------------------------------------------------------------------------------------------------------------
class StubScorer:
    """errors in millimetres / pixels taken from the estimate's t_x, so that a test writes them into the poses"""

    def errors(self, est, gt, K, object_index):
        e = np.asarray(est, np.float64).reshape(-1, 12)[:, 3]
        return e.astype(np.float32), e.astype(np.float32)


class StubVsd:
    taus = (0.05, 0.5)

    def __init__(self):
        self.calls = []

    def errors(self, est, gt, K, object_index, image_keys, diameters):
        self.calls.append((np.asarray(est).copy(), np.asarray(gt).copy(), np.asarray(object_index).copy(), list(image_keys), list(diameters)))
        e = np.asarray(est, np.float64).reshape(-1, 12)[:, 7]           # the VSD error at tau 0 is the estimate's t_y; at tau 1, half of it
        return np.stack([e, 0.5 * e], axis=1)


def score_inputs():
    def inst(obj):
        return {"id": obj, "R": np.eye(3), "t": np.array([0.0, 0.0, 900.0])}

    def pose(tx, ty):
        return np.hstack([np.eye(3), [[tx], [ty], [900.0]]])

    gts = {(1, 0): [inst(1), inst(2)], (1, 1): [inst(1)]}
    cams = {k: np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]]) for k in gts}
    # (scene, im, obj, score, t_x = MSSD / MSPD error, t_y = VSD error)
    rows = [(1, 0, 1, 1.0, 4.0, 0.12), (1, 0, 2, 1.0, 30.0, 0.31), (1, 1, 1, 1.0, 90.0, 0.62)]
    results = {"scene_id": np.array([r[0] for r in rows]), "im_id": np.array([r[1] for r in rows]), "obj_id": np.array([r[2] for r in rows]),
               "score": np.array([r[3] for r in rows]), "time": np.full(len(rows), -1.0), "pose": np.stack([pose(r[4], r[5]) for r in rows])}
    return results, gts, cams


TODAYS_KEYS = {"targets", "AR_MSSD", "AR_MSPD", "AR_MSSD_MSPD", "recall_mssd", "recall_mspd", "image_width", "mssd_thresholds", "mspd_thresholds",
               "objects", "pairs"}
TODAYS_OBJECT_KEYS = {"targets", "AR_MSSD", "AR_MSPD", "AR_MSSD_MSPD", "recall_mssd", "recall_mspd"}


def test_score_without_vsd_returns_todays_keys():
    from casapose_amd.pose_estimation.bop_scores import score

    results, gts, cams = score_inputs()
    out = score(results, gts, cams, StubScorer(), [1, 2], {1: 100.0, 2: 200.0})
    assert set(out) == TODAYS_KEYS and all(set(o) == TODAYS_OBJECT_KEYS for o in out["objects"].values())
    assert out == score(results, gts, cams, StubScorer(), [1, 2], {1: 100.0, 2: 200.0}, None, 640.0, vsd=None)
    assert out["pairs"] == 3 and out["targets"] == 3 and out["objects"]["1"]["recall_mssd"] == [0.5] * 10     # 4 mm < 5; 90 mm > 50


def test_score_with_vsd_hands_over_the_same_pairs_and_adds_three_keys():
    from casapose_amd.pose_estimation.bop_scores import score

    results, gts, cams = score_inputs()
    plain = score(results, gts, cams, StubScorer(), [1, 2], {1: 100.0, 2: 200.0})
    vsd = StubVsd()
    out = score(results, gts, cams, StubScorer(), [1, 2], {1: 100.0, 2: 200.0}, vsd=vsd)
    assert set(out) == TODAYS_KEYS | {"AR_VSD", "recall_vsd", "AR", "vsd_taus", "vsd_thresholds"}
    assert all(set(o) == TODAYS_OBJECT_KEYS | {"AR_VSD", "recall_vsd", "AR"} for o in out["objects"].values())
    for key in TODAYS_KEYS - {"objects"}:
        assert out[key] == plain[key], key
    (est, gt, obj, keys, diam), = vsd.calls
    assert est[:, 0, 3].tolist() == [4.0, 30.0, 90.0] and obj.tolist() == [0, 1, 0]        # the order of the MSSD / MSPD pairs
    assert keys == [(1, 0), (1, 0), (1, 1)] and diam == [100.0, 200.0, 100.0] and gt.shape == (3, 3, 4)
    # object 1: errors 0.12 and 0.62 at tau 0 -> one of two targets from theta = 0.15 on; 0.06 and 0.31 at tau 1 -> one from 0.10, two from 0.35
    o1, o2 = out["objects"]["1"], out["objects"]["2"]
    assert o1["recall_vsd"] == [[0.0, 0.0] + [0.5] * 8, [0.0] + [0.5] * 5 + [1.0] * 4]
    assert o2["recall_vsd"] == [[0.0] * 6 + [1.0] * 4, [0.0] * 3 + [1.0] * 7]              # 0.31 at tau 0, 0.155 at tau 1
    assert o1["AR_VSD"] == (4.0 + 6.5) / 20.0 and o2["AR_VSD"] == 11.0 / 20.0
    for o in (out, o1, o2):
        assert o["AR"] == (o["AR_VSD"] + o["AR_MSSD"] + o["AR_MSPD"]) / 3.0
    assert out["vsd_taus"] == [0.05, 0.5] and len(out["recall_vsd"]) == 2 and len(out["recall_vsd"][0]) == 10


def test_images_with_pairs_names_only_what_score_reads():
    from casapose_amd.pose_estimation.bop_vsd import images_with_pairs

    results, gts, cams = score_inputs()
    assert images_with_pairs(results, gts) == [(1, 0), (1, 1)]
    results["score"][2] = 0.0                                # "no estimate": image (1, 1) has no pair left
    assert images_with_pairs(results, gts) == [(1, 0)]
    assert images_with_pairs(results, gts, [{"scene_id": 1, "im_id": 1, "obj_id": 1, "inst_count": 1}]) == []


# ---- the script ----------------------------------------------------------------------------------------------------------------------------
def test_script_refuses_a_missing_depth_image_before_any_device_work(tmp_path, monkeypatch):
    import test_masks_twin_host as TM
    from casapose_amd.pose_estimation import bop_scores, bop_vsd
    from casapose_amd.utils.io_utils import write_poses

    sys.path.insert(0, os.path.join(ROOT, "util_scripts"))
    try:
        import bop_score
    finally:
        sys.path.pop(0)
    root = tmp_path / "bop"
    TM.write_bop_tree(root)                                   # models/, test/000002 with two images; no depth/
    os.makedirs(root / "test" / "000002" / "depth")
    from PIL import Image

    Image.fromarray(np.full((TM.H, TM.W), 5000, np.uint16)).save(root / "test" / "000002" / "depth" / "000000.png")
    out_dir = str(tmp_path / "run") + "/"
    for im, instances in enumerate(TM.bop_poses()):
        poses = {o: P.astype(np.float32) for o, P in instances}
        write_poses(np.stack([poses[1], poses[5]])[:, None], np.stack([poses[1], poses[5]]), TM.NAMES, "000002_rgb_%06d" % im, out_dir)

    def no_device(*a, **k):
        raise AssertionError("a device scorer was built before the depth images were checked")

    monkeypatch.setattr(bop_score, "DeviceBopScorer", no_device)
    monkeypatch.setattr(bop_score, "DeviceVsdScorer", no_device)
    args = ["--result_file", out_dir + "bop_evaluation.csv", "--dataset_path", str(root), "--split", "test", "--model_folder", "models", "--vsd"]
    with pytest.raises(FileNotFoundError, match=r"depth.000001\.png"):
        bop_score.main(args)
    with pytest.raises(FileNotFoundError, match=r"sensor.000000\.png"):
        bop_score.main(args + ["--depth_folder", "sensor"])
    assert bop_scores.score.__defaults__[-1] is None and bop_vsd.depth_path("s", "000002", "depth", 7) == os.path.join("s", "000002", "depth", "000007.png")


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from casapose_amd import _lib

    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    i, d, p = C.c_int, C.c_double, C.c_void_p
    assert table["cp_vsd_tile"] == (C.c_int, [])
    assert table["cp_vsd_counts_i32"] == (C.c_int, [p, p, i, i, i, p, p, i, p, p, i, d, p, i, i, p, p])
    assert _lib.POINTEES["cp_vsd_counts_i32"] == ("uint32_t", "int32_t", None, None, None, "float", "double", None, "int32_t", "double", None, None,
                                                  "double", None, None, "int32_t", "void")
    assert hasattr(hip_lib, "cp_vsd_counts_i32") and hip_lib.cp_vsd_tile() >= 64 and hip_lib.cp_vsd_tile() % 64 == 0
    assert not any("vsd" in k or "vsd" in v for k, v in _lib.TWINS.items()) and len(_lib.TWINS) == 5 and _lib.ABI_VERSION == 302
    text = open(os.path.join(ROOT, "include", "casapose_hip.h")).read()
    block = text[text.index("BOP's Visible Surface Discrepancy"):text.index("int cp_vsd_tile(void);")]
    assert block.rstrip().endswith("Added in ABI 302 without changing any earlier entry point. */")


def test_entry_point_refuses_bad_arguments_by_name(hip_lib):
    """CP_REQUIRE runs before anything is launched: no GPU is needed to be refused"""
    a = np.zeros(64, np.float64)
    p = a.ctypes.data
    ok = [p, p, 1, 4, 4, p, p, 1, p, p, 1, 15.0, p, 10, 1, p]       # ... and a null stream
    for at, bad, word in ((13, 33, b"ntau"), (13, 0, b"ntau"), (0, None, b"null"), (2, 0, b"nplanes"), (3, 16385, b"H and W"), (10, 0, b"npairs"),
                          (11, -1.0, b"delta"), (11, float("nan"), b"delta"), (14, 0, b"split"), (14, 65, b"split"), (6, p + 4, b"8-byte"),
                          (15, p + 2, b"4-byte")):
        args = list(ok)
        args[at] = bad
        assert hip_lib.cp_vsd_counts_i32(*args, None) == -1 and word in hip_lib.cp_last_error(), word


def test_scorer_without_a_device_has_no_fall_back():
    import test_masks_twin_host as TM
    from casapose_amd._lib import CasaposeHipError
    from casapose_amd.pose_estimation.bop_vsd import DeviceVsdScorer

    v, f = TM.ellipsoid(1, (10, 10, 10))
    scorer = DeviceVsdScorer([v], [f], None)
    with pytest.raises(CasaposeHipError, match="no host fall-back"):
        scorer.counts(np.eye(4)[None, :3], np.eye(4)[None, :3], np.eye(3), [0], [0], [np.zeros((4, 4), np.float32)], [20.0])
    with pytest.raises(ValueError, match="one array per object"):
        DeviceVsdScorer([v], [], None)


# ---- the reference on its own ---------------------------------------------------------------------------------------------------------------
def test_reference_on_the_hand_worked_quad():
    q = VC.quad()
    scene = VR.Scene(q["meshes"], VC.NEAR, VC.FAR)
    cam = (2000.0, 2000.0, 9.5, 7.5)
    hit, z = VR.plane_depth(scene.plane(0, q["gt"][0], cam, 16, 20))
    assert hit.sum() == VC.QUAD_N == 96 and hit[4:12, 4:16].all() and np.all(z[hit] == 1000.0)
    counts, undecided = scene.counts(0, q["est"][0], q["gt"][0], cam, q["depths"][0], 8.0)
    assert counts.tolist() == [96, 96, 96, 96, 0, 0, 0, 0, 0, 0, 0, 0] and undecided == 0
    assert VR.errors_of(counts).tolist() == [1.0, 1.0] + [0.0] * 8
    # the sensor 100 mm in front of both: nothing is visible; no sensor depth: everything is
    assert scene.counts(0, q["est"][0], q["gt"][0], cam, np.full((16, 20), 900.0, np.float32), 8.0)[0].tolist() == [0] * 12
    assert scene.counts(0, q["est"][0], q["gt"][0], cam, np.zeros((16, 20), np.float32), 8.0)[0].tolist() == [96] * 4 + [0] * 8
    # a comparison inside the margin is reported: delta equal to the distance difference at the principal point's neighbours
    d = VR.distance_image(np.full((16, 20), 1001.0), cam) - VR.distance_image(np.full((16, 20), 1000.0), cam)
    assert scene.counts(0, q["est"][0], q["gt"][0], cam, q["depths"][0], 8.0, delta=float(d[7, 9]))[1] >= 1


@pytest.mark.parametrize("case", ["ellipsoids", "many_slots"])
def test_reference_alone_stays_inside_the_undecided_cap(case):
    """what the GPU tests' gate needs of their scenes, checked where no GPU is: at most 2 % of the pairs have an undecided pixel, and the scenes
    hold what they mean to hold"""
    c = getattr(VC, case)()
    want, und = c["want"], c["undecided"]
    assert (und > 0).sum() <= 0.02 * len(und), (case, int((und > 0).sum()), len(und))
    e = np.stack([VR.errors_of(w) for w in want])
    if case == "ellipsoids":
        assert len(want) == 30 and c["renders"] == 30
        first = want[:15].reshape(3, 5, 12)                       # 48 x 64: [object][estimate]
        assert (first[:, 0, 0] == first[:, 0, 1]).all() and (first[:, 0, 2:] == 0).all() and (first[:, 0, 0] > 40).all()      # exact: error 0
        assert (first[:, 1, 1] > 0).all() and (first[:, 1, 2] >= 0.9 * first[:, 1, 1]).all() and (first[:, 1, 11] == 0).all()   # deeper: a step
        assert (first[:, 2, 1] > 0).all() and (first[:, 2, 0] > first[:, 2, 1]).all()                                         # sideways
        assert (first[:, 3:, 1] == 0).all() and (first[:, 3:, 0] == first[:, :1, 0]).all()                                    # off / behind: gt only
        assert 0 < want[25, 0] < first[2, 0, 0] / 4                                  # 37 x 50: the border cuts most of the third object off
        visible = [int(VR.plane_depth(VR.Scene(c["meshes"], VC.NEAR, VC.FAR).plane(1, c["gt"][5], (100.0, 101.0, 31.7, 23.4), 48, 64))[0].sum())]
        assert first[1, 0, 0] < visible[0]                                           # the second object is partly occluded
    else:
        assert len(want) == 299 and (want[:, 0] > 0).all() and len(np.unique(e[:, 0])) > 20 and 0 < (want[:, 1] == 0).sum() + 1
        assert (e.min(axis=1) < 0.3).any() and (e.max(axis=1) == 1.0).any()
