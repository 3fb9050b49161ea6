"""CPU checks of the BOP scorer (casapose_amd/pose_estimation/bop_scores.py, csrc/bop_errors.hip): the symmetry sets of models_info entries,
targets, matching and recall on answers worked out by hand, the result file's round trip, and the argument refusals of cp_bop_errors_f32.  No
kernel is launched here; the kernels are checked in tests/test_gpu_bop_scores.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_INFO = os.path.join(ROOT, "tests", "golden", "ref_data", "lm_models_eval", "models_info.json")


@pytest.fixture(scope="module")
def lib():
    from casapose_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def lm_info():
    with open(LM_INFO) as f:
        return json.load(f)


# ---- symmetry sets ----------------------------------------------------------------------------------------------------------------------
def test_symmetry_transforms_of_the_lm_models(lm_info):
    from casapose_amd.pose_estimation.bop_scores import symmetry_transforms

    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    s1 = symmetry_transforms(lm_info["obj_000001"])
    assert s1.dtype == np.float64 and s1.shape == (1, 3, 4) and np.array_equal(s1[0], ident)
    s10 = symmetry_transforms(lm_info["obj_000010"])
    assert s10.shape == (2, 3, 4) and np.array_equal(s10[0], ident)
    assert np.array_equal(s10[1], np.array(lm_info["obj_000010"]["symmetries_discrete"][0]).reshape(4, 4)[:3])
    s3 = symmetry_transforms(lm_info["obj_000003"])
    assert s3.shape == (315, 3, 4) and np.array_equal(s3[0], ident)
    for k, m in enumerate(s3):
        R = m[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
        th = 2.0 * math.pi * k / 315
        want = np.array([[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]])
        assert np.abs(R - want).max() <= 1e-15 and np.all(m[:, 3] == 0)
    assert symmetry_transforms({}).shape == (1, 3, 4)


def test_symmetry_transforms_discrete_times_continuous_with_an_offset():
    from casapose_amd.pose_estimation.bop_scores import symmetry_transforms

    flip = [1, 0, 0, 4.0, 0, -1, 0, 0, 0, 0, -1, 10.0, 0, 0, 0, 1]                # 180 degrees about x, with a translation
    offset = np.array([3.0, -2.0, 5.0])
    entry = {"symmetries_discrete": [flip], "symmetries_continuous": [{"axis": [0, 0, 2.0], "offset": offset.tolist()}]}
    S = symmetry_transforms(entry)
    assert S.shape == (630, 3, 4)
    # the first 315 are the continuous set itself (d = identity): each maps the offset point to itself; k = 1 is a turn by 2 pi / 315 about z
    for m in S[:315]:
        assert np.abs(m[:, :3] @ offset + m[:, 3] - offset).max() <= 1e-12
    th = 2.0 * math.pi / 315
    assert np.abs(S[1, :2, :2] - [[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]).max() <= 1e-15
    assert np.array_equal(S[0], np.hstack([np.eye(3), np.zeros((3, 1))]))
    # d-major: element 315 + k is c_k applied after the flip
    D = np.array(flip, np.float64).reshape(4, 4)
    assert np.array_equal(S[315], D[:3])
    for k in (1, 100, 314):
        c = np.eye(4)
        c[:3] = S[k]
        assert np.abs((c @ D)[:3] - S[315 + k]).max() <= 1e-14
    # a coarser step: n = ceil(pi / 0.5) = 7
    assert symmetry_transforms(entry, max_sym_disc_step=0.5).shape == (14, 3, 4)
    # the independent restatement the GPU tests use builds the same set
    import bop_reference as B

    assert np.abs(B.symmetry_set(entry) - S).max() <= 1e-12


# ---- matching and recall, by hand -------------------------------------------------------------------------------------------------------
def _col(*rows):
    return np.array(rows, np.float64)


def test_one_target_correct_from_the_third_threshold():
    """diameter 100: e_MSSD = 12 mm is below 0.15 * 100 and every larger threshold, above 5 and 10: 8 of 10 -> AR_MSSD = 0.8.  e_MSPD = 22 px is
    below 25 .. 50: 6 of 10."""
    from casapose_amd.pose_estimation.bop_scores import match_and_recall

    out = match_and_recall([(7, 1, _col([12.0]), _col([22.0]))], {7: 100.0}, 640.0)
    assert out["targets"] == 1 and out["recall_mssd"] == [0.0, 0.0] + [1.0] * 8 and out["recall_mspd"] == [0.0] * 4 + [1.0] * 6
    assert out["AR_MSSD"] == 0.8 and out["AR_MSPD"] == 0.6 and abs(out["AR_MSSD_MSPD"] - 0.7) < 1e-15
    assert out["objects"]["7"]["AR_MSSD"] == 0.8 and "AR" not in out
    # twice the image width doubles the pixel thresholds: 22 px is below 10 * 2 = 20? no; below 15 * 2 = 30: 8 of 10
    assert match_and_recall([(7, 1, _col([12.0]), _col([22.0]))], {7: 100.0}, 1280.0)["AR_MSPD"] == 0.8


def test_two_instances_one_estimate():
    """The estimate is 3 mm from instance 1 and 40 mm from instance 0 (diameter 100): it takes instance 1 from theta = 0.05 on; the other
    instance stays unmatched, so recall is 1 / 2 everywhere."""
    from casapose_amd.pose_estimation.bop_scores import greedy_matches, match_and_recall

    out = match_and_recall([(2, 2, _col([40.0, 3.0]), _col([90.0, 2.0]))], {2: 100.0})
    assert out["targets"] == 2 and out["recall_mssd"] == [0.5] * 10 and out["recall_mspd"] == [0.5] * 10 and out["AR_MSSD_MSPD"] == 0.5
    assert greedy_matches(_col([40.0, 3.0]), 5.0) == 1 and greedy_matches(_col([40.0, 3.0]), 3.0) == 0     # strictly below


def test_the_higher_score_takes_the_nearer_instance():
    """Two estimates (rows, by descending score) and two instances.  Row 0 is 4 mm from instance 0 and 6 from instance 1; row 1 is 2 mm from
    instance 0 and 31 from instance 1.  Row 0 takes instance 0 (its smallest), so row 1 is left with instance 1 at 31 mm: at theta * 100 <= 30
    one match, above it two.  (Matching row 1 first would give two matches already at 10.)"""
    from casapose_amd.pose_estimation.bop_scores import greedy_matches, match_and_recall

    e = _col([4.0, 6.0], [2.0, 31.0])
    # at 3 mm row 0 takes nothing (4 is not below 3) and blocks nothing, so row 1 takes instance 0
    assert [greedy_matches(e, t) for t in (2.0, 3.0, 5.0, 10.0, 31.0, 35.0)] == [0, 1, 1, 1, 1, 2]
    out = match_and_recall([(1, 2, e, e)], {1: 100.0})
    assert out["recall_mssd"] == [0.5] * 6 + [1.0] * 4 and out["AR_MSSD"] == 0.7
    assert out["recall_mspd"] == [0.5] * 6 + [1.0] * 4      # pixel thresholds 5 .. 50 happen to cut at the same places
    # an estimate whose best free instance is above the threshold takes nothing and blocks nothing
    assert greedy_matches(_col([50.0, 60.0], [1.0, 70.0]), 10.0) == 1


class _TableScorer:
    """Stands in for DeviceBopScorer: the error of a pair is |t_est - t_gt| (MSSD) and twice that (MSPD)."""

    def __init__(self):
        self.calls = []

    def errors(self, est, gt, K, object_index):
        d = np.linalg.norm(np.asarray(est)[:, :, 3] - np.asarray(gt)[:, :, 3], axis=1)
        self.calls.append((np.asarray(est).copy(), np.asarray(object_index).copy()))
        return d.astype(np.float32), (2.0 * d).astype(np.float32)


def _pose(t):
    return np.hstack([np.eye(3), np.asarray(t, np.float64).reshape(3, 1)])


def _results(rows):
    return {"scene_id": np.array([r[0] for r in rows]), "im_id": np.array([r[1] for r in rows]), "obj_id": np.array([r[2] for r in rows]),
            "score": np.array([r[3] for r in rows], np.float64), "time": np.full(len(rows), -1.0),
            "pose": np.array([r[4] for r in rows], np.float64).reshape(len(rows), 3, 4)}


def _gt(obj, t, visib=None):
    g = {"id": obj, "R": np.eye(3), "t": list(t)}
    if visib is not None:
        g["visib_fract"] = visib
    return g


def test_score_with_a_miss_row_targets_and_visibility():
    from casapose_amd.pose_estimation.bop_scores import score, select_targets

    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    gts = {(1, 0): [_gt(5, (0, 0, 1000), 0.9), _gt(5, (200, 0, 1000), 0.05), _gt(6, (0, 100, 900), 0.5)],
           (1, 1): [_gt(5, (0, 0, 800), 1.0)]}
    cams = {k: K for k in gts}
    rows = [(1, 0, 5, 1.0, _pose((0, 4, 1000))),          # 4 mm from the visible instance of object 5
            (1, 0, 6, 0.0, np.zeros((3, 4))),             # a miss row for object 6
            (1, 1, 5, 1.0, _pose((0, 0, 812))),           # 12 mm
            (1, 1, 9, 1.0, _pose((0, 0, 812)))]           # an object without targets: ignored
    diam = {5: 100.0, 6: 100.0}
    # the visib_fract rule: the 5 % instance is no target and no candidate
    want = select_targets(gts)
    assert want == {(1, 0, 5): (1, [0]), (1, 0, 6): (1, [2]), (1, 1, 5): (1, [0])}
    sc = _TableScorer()
    out = score(_results(rows), gts, cams, sc, [5, 6], diam)
    assert len(sc.calls) == 1 and list(sc.calls[0][1]) == [0, 0] and out["pairs"] == 2            # the miss row makes no pair
    assert out["targets"] == 3
    assert out["objects"]["5"]["targets"] == 2 and out["objects"]["6"]["targets"] == 1
    # object 5: 4 mm is correct at every theta, 12 mm from theta = 0.15: recall (1, 1, 2, 2, ...) / 2
    assert out["objects"]["5"]["recall_mssd"] == [0.5, 0.5] + [1.0] * 8 and out["objects"]["5"]["AR_MSSD"] == 0.9
    # MSPD = 8 and 24 px: 8 px from theta = 10, 24 px from theta = 25
    assert out["objects"]["5"]["recall_mspd"] == [0.0, 0.5, 0.5, 0.5] + [1.0] * 6
    assert out["objects"]["6"]["AR_MSSD"] == 0.0 and out["objects"]["6"]["AR_MSPD"] == 0.0
    assert out["recall_mssd"] == [1 / 3, 1 / 3] + [2 / 3] * 8
    assert abs(out["AR_MSSD"] - 0.6) < 1e-15 and out["AR_MSSD_MSPD"] == 0.5 * (out["AR_MSSD"] + out["AR_MSPD"])

    # without scene_gt_info every instance is a target: object 5 has two in image 0, one estimate -> the far instance is never found
    bare = {k: [{a: b for a, b in g.items() if a != "visib_fract"} for g in v] for k, v in gts.items()}
    assert select_targets(bare)[(1, 0, 5)] == (2, [0, 1])
    out = score(_results(rows), bare, cams, _TableScorer(), [5, 6], diam)
    assert out["targets"] == 4 and out["objects"]["5"]["recall_mssd"] == [1 / 3, 1 / 3] + [2 / 3] * 8

    # a targets file that leaves out image 1 and object 6, and asks for one instance of object 5 in image 0: the candidates are both instances
    targets = [{"scene_id": 1, "im_id": 0, "obj_id": 5, "inst_count": 1}]
    assert select_targets(gts, targets) == {(1, 0, 5): (1, [0, 1])}
    out = score(_results(rows), gts, cams, _TableScorer(), [5, 6], diam, targets=targets)
    assert out["targets"] == 1 and out["AR_MSSD"] == 1.0 and list(out["objects"]) == ["5"] and out["pairs"] == 2
    with pytest.raises(KeyError, match="no evaluation mesh"):
        score(_results(rows), gts, cams, _TableScorer(), [6], diam)


def test_estimates_are_ranked_by_score_with_ties_in_file_order():
    from casapose_amd.pose_estimation.bop_scores import score

    K = np.eye(3)
    gts = {(2, 3): [_gt(1, (0, 0, 500))]}
    rows = [(2, 3, 1, 0.5, _pose((0, 0, 540))), (2, 3, 1, 0.9, _pose((0, 0, 520))), (2, 3, 1, 0.9, _pose((0, 0, 503)))]
    sc = _TableScorer()
    out = score(_results(rows), gts, {(2, 3): K}, sc, [1], {1: 100.0})
    # one instance: one estimate is kept, the first of the two with score 0.9 (20 mm), not the nearer one after it
    assert out["pairs"] == 1 and sc.calls[0][0][0, 2, 3] == 520.0
    assert out["recall_mssd"] == [0.0] * 4 + [1.0] * 6           # 20 mm < theta * 100 from theta = 0.25 on
    # scores() output is plain Python: io_utils.to_json writes it and json reads it back
    from casapose_amd.utils.io_utils import to_json

    assert json.loads(to_json(out))["recall_mssd"] == out["recall_mssd"]


# ---- the result file --------------------------------------------------------------------------------------------------------------------
def test_read_bop_results_round_trips_write_poses(tmp_path):
    from casapose_amd.pose_estimation.bop_scores import is_estimate, read_bop_results
    from casapose_amd.utils.io_utils import write_poses

    rng = np.random.default_rng(4)
    gt = rng.normal(0, 1, (3, 1, 3, 4)).astype(np.float32)
    gt[2] = 0                                                       # object 12 is not in the image: no row
    est = rng.normal(0, 1, (3, 3, 4)).astype(np.float32)
    est[1] = 0                                                      # object 7 was missed
    out = str(tmp_path) + "/"
    write_poses(gt, est, ["obj_000005", "obj_000007", "obj_000012"], "000048_rgb_000123", out, time_needed=0.25)
    write_poses(gt, est, ["obj_000005", "obj_000007", "obj_000012"], "000048_rgb_000124", out)
    res = read_bop_results(out + "bop_evaluation.csv")
    assert list(res["scene_id"]) == [48] * 4 and list(res["im_id"]) == [123, 123, 124, 124] and list(res["obj_id"]) == [5, 7, 5, 7]
    assert list(res["score"]) == [1.0, 0.0, 1.0, 0.0] and list(res["time"]) == [0.25, 0.25, -1.0, -1.0]
    assert res["pose"].shape == (4, 3, 4) and res["pose"].dtype == np.float64
    assert np.array_equal(res["pose"][0].astype(np.float32), est[0]) and np.all(res["pose"][1] == 0)      # str(float32) round-trips
    assert list(is_estimate(res["score"], res["pose"])) == [True, False, True, False]
    assert list(is_estimate([1.0, 0.0], np.stack([np.zeros((3, 4)), est[0]]))) == [False, False]          # either sign of a miss


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_bop_errors_symbols_and_workspace(lib):
    from casapose_amd import _lib

    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for n in ("cp_bop_errors_workspace_bytes", "cp_bop_errors_tile", "cp_bop_errors_sym_group", "cp_bop_errors_f32"):
        assert hasattr(lib, n) and n in bound, n
    assert len(bound["cp_bop_errors_f32"][1]) == 14 and bound["cp_bop_errors_workspace_bytes"][0] is C.c_size_t
    assert "bop_errors.hip" in open(os.path.join(ROOT, "casapose_amd", "csrc", "Makefile")).read()
    assert lib.cp_bop_errors_tile() >= 64 and lib.cp_bop_errors_tile() % 64 == 0 and lib.cp_bop_errors_sym_group() >= 2
    # one (MSSD, MSPD) pair of fp32 maxima per (pair, symmetry)
    assert lib.cp_bop_errors_workspace_bytes(3, 5) == 3 * 5 * 2 * 4 and lib.cp_bop_errors_workspace_bytes(70000, 630) == 70000 * 630 * 8
    assert lib.cp_bop_errors_workspace_bytes(0, 5) == 0 and lib.cp_bop_errors_workspace_bytes(3, 0) == 0
    assert lib.cp_version() == _lib.ABI_VERSION == 302             # additions only
    assert not any("bop" in host for host in _lib.TWINS.values())  # the host copy is bop_math.h in the self-test, not an export


def test_bop_errors_refuses_bad_arguments_before_any_launch(lib):
    """Never-dereferenced stand-in pointers: every call below is refused by its argument checks."""
    from casapose_amd import _lib

    p = lambda a: C.c_void_p(a)  # noqa: E731
    good = dict(points=p(4096), counts=p(8192), objects=2, vmax=100, syms=p(12288), sym_counts=p(16384), smax=3, pairs=p(20480), index=p(24576),
                npairs=5, workspace=p(28672), errors=p(32768), per=None)
    bad = [dict(points=None), dict(counts=None), dict(syms=None), dict(sym_counts=None), dict(pairs=None), dict(index=None), dict(workspace=None),
           dict(errors=None), dict(objects=0), dict(vmax=0), dict(vmax=(1 << 24) + 1), dict(smax=0), dict(smax=-3), dict(smax=(1 << 16) + 1),
           dict(npairs=0), dict(npairs=-1), dict(npairs=1 << 24), dict(npairs=1 << 20, smax=630), dict(workspace=p(28676))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.cp_bop_errors_f32(a["points"], a["counts"], a["objects"], a["vmax"], a["syms"], a["sym_counts"], a["smax"], a["pairs"], a["index"],
                                   a["npairs"], a["workspace"], a["errors"], a["per"], None)
        assert rc == -1, change                                     # CP_ERR_INVALID
        assert lib.cp_last_error().startswith(b"cp_bop_errors_f32:"), change
    with pytest.raises(_lib.CasaposeHipError, match="must be positive"):
        _lib.check(lib.cp_bop_errors_f32(p(4096), p(8192), 2, 100, p(12288), p(16384), 3, p(20480), p(24576), 0, p(28672), p(32768), None, None),
                   "cp_bop_errors_f32")


def test_pairs_are_packed_in_the_pose_eval_record():
    from casapose_amd.pose_estimation.bop_scores import pack_bop_pairs

    est = np.arange(24, dtype=np.float64).reshape(2, 3, 4) + 0.5
    gt = -np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    K = np.array([[572.4, 0.1, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])
    rec, idx = pack_bop_pairs(est, gt, K, [1, 0], 2)
    assert rec.dtype == np.float32 and rec.shape == (2, 36) and idx.dtype == np.int32 and list(idx) == [1, 0]
    assert np.array_equal(rec[1, :12], (np.arange(12, 24) + 0.5).astype(np.float32)) and np.array_equal(rec[1, 12:24], -np.arange(12, 24, dtype=np.float32))
    assert np.array_equal(rec[0, 24:33], K.astype(np.float32).reshape(9)) and np.all(rec[:, 33:] == 0)
    rec2, _ = pack_bop_pairs(est.reshape(2, 12), gt, np.stack([K, 2 * K]), [0, 0], 1)
    assert np.array_equal(rec2[1, 24:33], (2 * K).astype(np.float32).reshape(9))
    with pytest.raises(ValueError, match="object_index"):
        pack_bop_pairs(est, gt, K, [0, 2], 2)
