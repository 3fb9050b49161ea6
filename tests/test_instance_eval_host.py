"""pose_estimation/instance_evaluation.py on the host: the greedy rule on hand-made cost matrices, match_instances_host against evaluate_poses
at R = I = 1, summarise on a hand-counted case, the CSV writers, and the stand-alone self-test of csrc/match_math.h.  No GPU."""
import csv
import os
import subprocess

import numpy as np
import pytest

from casapose_amd.pose_estimation import instance_evaluation as IE
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation import pose_evaluation as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def match(cost, live=None, count=None):
    cost = np.asarray(cost, np.float64)
    live = [True] * cost.shape[0] if live is None else live
    em, gm, n = IE.greedy_match(cost, live, cost.shape[1] if count is None else count)
    return em.tolist(), gm.tolist(), n


def test_ties_go_to_the_smaller_instance_then_the_smaller_estimate():
    assert match([[3, 3], [3, 3], [3, 3]]) == ([0, 1, -1], [0, 1], 2)
    assert match([[9, 1], [1, 9]]) == ([1, 0], [1, 0], 2)           # (e1, g0) and (e0, g1) tie: g 0 is served first
    assert match([[4], [4]]) == ([0, -1], [0], 1)                   # two identical estimates: slot 0 matches, slot 1 is the false positive


def test_empty_slots_and_no_ground_truth():
    assert match([[0, 0], [5, 7], [6, 1]], live=[False, True, True]) == ([-2, 0, 1], [1, 2], 2)
    assert match([[1, 2], [3, 4]], count=0) == ([-1, -1], [-1, -1], 0)
    assert match([[1, 2]], live=[False]) == ([-2], [-1, -1], 0)
    assert match([[5, 0], [4, 0]], count=1) == ([-1, 0], [1, -1], 1)   # column 1 is no instance


def test_more_estimates_than_instances_and_fewer():
    assert match([[5, 6], [1, 9], [7, 2], [8, 8]]) == ([-1, 0, 1, -1], [1, 2], 2)
    assert match([[5, 1, 7, 8], [6, 9, 2, 8]]) == ([1, 2], [-1, 0, 1, -1], 2)


def test_a_cost_that_is_not_finite_is_never_matched():
    assert match([[NAN, INF], [NAN, 2], [INF, NAN]]) == ([-1, 1, -1], [-1, 1], 1)
    assert match([[INF]]) == ([-1], [-1], 0)


def test_the_rule_is_greedy_not_optimal_and_the_documents_say_so():
    """(e0, g0) = 1 is taken first and leaves (e1, g1) = 100; the optimum pairs (e0, g1), (e1, g0) at 2 + 2: under a threshold of 3 greedy finds
    one instance, the optimum two."""
    em, gm, n = match([[1, 2], [2, 100]])
    assert (em, gm, n) == ([0, 1], [0, 1], 2)
    cost = np.array([[1.0, 2.0], [2.0, 100.0]])
    assert sum(cost[e, g] < 3 for e, g in enumerate(em)) == 1 and sum(cost[e, g] < 3 for e, g in enumerate([1, 0])) == 2
    for name in ("DESIGN.md", os.path.join("casapose_amd", "csrc", "match_math.h"), os.path.join("casapose_amd", "pose_estimation", "instance_evaluation.py")):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "greedy" in text.lower() and "0.2 diameters" in text, name


def rot(rv):
    return P.rodrigues(np.asarray(rv, np.float64))


def scene(seed=3, b=3, oc=3):
    """one estimate and one instance per (image, object): near, far and zero estimates; counts (40, 25, 12), the second mesh symmetric"""
    rng = np.random.default_rng(seed)
    counts = np.array([40, 25, 12])
    mesh = np.zeros((oc, 40, 3), np.float32)
    for o in range(oc):
        mesh[o, :counts[o]] = rng.uniform(-40, 40, (counts[o], 3))
    gt = np.zeros((b, oc, 1, 3, 4), np.float32)
    est = np.zeros((b, oc, 1, 3, 4), np.float32)
    for n in range(b):
        for o in range(oc):
            R, t = rot(rng.normal(0, 1, 3)), np.array([rng.uniform(-100, 100), rng.uniform(-80, 80), rng.uniform(600, 1000)])
            gt[n, o, 0] = np.concatenate([R, t[:, None]], 1)
            shift = (0.5, 3.0, 30.0)[(n + o) % 3]
            est[n, o, 0] = np.concatenate([rot([0.01 * shift, 0, 0]) @ R, (t + shift)[:, None]], 1)
    est[1, 2] = 0.0                                # an empty slot
    diam = np.array([80.0, 90.0, 100.0], np.float32)
    return mesh, counts, gt, est, diam


def test_one_estimate_and_one_instance_is_evaluate_poses(monkeypatch):
    mesh, counts, gt, est, diam = scene()
    b, oc = gt.shape[:2]
    flags = [0, 1, 0]
    err, rec, em, tally = IE.match_instances_host(est, gt, np.ones((b, oc), np.int32), mesh, counts, K, diam, symmetric=flags, allowed_error_2d=5.0)
    monkeypatch.setattr(E, "SYMMETRIC_VERTEX_COUNTS", (25,))
    pts, cnt = E._eval_points(None, mesh, counts.reshape(oc, 1), 1, oc, 1)
    valid = np.ones((1, oc))
    seen = set()
    for n in range(b):
        e2, e3, v2, v3, miss, _, fp = E.evaluate_poses(est[n:n + 1, :, 0], gt[n:n + 1], None, pts, cnt, K[None], np.tile(diam[None, :, None], (1, 1, 1)), valid, 5.0)
        for o in range(oc):
            if miss[o]:
                assert em[n, o, 0] == IE.EMPTY and rec[n, o, 0].tolist() == [-1, 0, 0, 0, 0] and np.all(np.isinf(err[n, o]))
                assert tally[n, o].tolist() == [1, 0, 0, 0, 0]
                continue
            # evaluate_poses returns float32 roundings of the same fp64 values
            assert np.float32(err[n, o, 0, 0, 0]) == e2[o] and np.float32(err[n, o, 0, 0, 1]) == e3[o]
            assert rec[n, o, 0, 0] == 0 and rec[n, o, 0, 3] == v3[o] and rec[n, o, 0, 4] == v2[o] and em[n, o, 0] == 0
            assert tally[n, o].tolist() == [1, 1, 1, int(v3[o]), int(v2[o])]
            seen.add((int(v3[o]), int(v2[o])))
    assert (1, 1) in seen and (0, 0) in seen, "the scene has to hold estimates on both sides of the thresholds"


def test_absent_instances_and_diameters_of_a_batch():
    """a batch's diameters [b, oc, I] pad absent instances with -1; rows g >= count stay (-1, 0, 0, 0, 0) and their errors +inf"""
    mesh, counts, gt1, est1, diam = scene(b=2)
    gt = np.concatenate([gt1, np.zeros_like(gt1)], axis=2)
    est = np.concatenate([est1, est1], axis=2)                      # two identical estimates per group
    dbatch = np.full((2, 3, 2), -1.0, np.float32)
    dbatch[:, :, 0] = diam
    err, rec, em, tally = IE.match_instances_host(est, gt, np.ones((2, 3), np.int32), mesh, counts, K, dbatch, symmetric=[0, 1, 0])
    assert np.all(np.isinf(err[:, :, :, 1])) and np.all(rec[:, :, 1] == [-1, 0, 0, 0, 0])
    assert em[0, 0].tolist() == [0, -1] and em[1, 2].tolist() == [-2, -2] and tally[0, 0, :3].tolist() == [1, 2, 1]
    assert np.array_equal(IE.object_diameters(dbatch, 3), diam.astype(np.float64))


def test_summarise_on_a_hand_counted_case(tmp_path):
    # two images, two objects, I = 2.  object 0: image 0 has 2 instances, both matched (one inside both thresholds, one outside both), 3 estimates;
    # image 1 has 1 instance, not found, 0 estimates.  object 1: image 0 has none but 1 estimate; image 1 has 1, matched, valid in 2-D only
    tally = np.array([[[2, 3, 2, 1, 1], [0, 1, 0, 0, 0]], [[1, 0, 0, 0, 0], [1, 1, 1, 0, 1]]], np.int32)
    rec = np.zeros((2, 2, 2, 5), np.float32)
    rec[..., 0] = -1
    rec[0, 0, 0] = (2, 1.0, 4.0, 1, 1)
    rec[0, 0, 1] = (0, 9.0, 30.0, 0, 0)
    rec[1, 1, 0] = (0, 3.0, 14.0, 0, 1)
    s = IE.summarise(tally, rec)
    a, b = s["objects"]
    assert (a["gt"], a["est"], a["matched"], a["tp_add"], a["tp_2d"]) == (3, 3, 2, 1, 1)
    assert a["recall_add"] == pytest.approx(1 / 3) and a["precision_add"] == pytest.approx(1 / 3) and a["recall_2d"] == pytest.approx(1 / 3)
    assert a["mean_err_3d"] == 17.0 and a["median_err_3d"] == 17.0 and a["mean_err_2d"] == 5.0
    assert (b["gt"], b["est"], b["matched"], b["tp_add"], b["tp_2d"]) == (1, 2, 1, 0, 1)
    assert b["recall_add"] == 0.0 and b["recall_2d"] == 1.0 and b["precision_2d"] == 0.5 and b["median_err_3d"] == 14.0
    t = s["all"]
    assert (t["gt"], t["est"], t["matched"], t["tp_add"], t["tp_2d"]) == (4, 5, 3, 1, 2)
    assert t["recall_add"] == 0.25 and t["recall_2d"] == 0.5 and t["precision_add"] == 0.2 and t["precision_2d"] == 0.4
    assert t["mean_err_3d"] == 16.0 and t["median_err_3d"] == 14.0 and t["median_err_2d"] == 3.0
    # the same figures from the per-image pieces, stacked
    assert IE.summarise(np.stack([tally[:1], tally[1:]]), np.stack([rec[:1], rec[1:]])) == s
    none = IE.summarise(np.zeros((1, 1, 5), np.int32), np.full((1, 1, 2, 5), -1.0))["all"]
    assert none["recall_add"] == 0.0 and none["precision_add"] == 0.0 and np.isnan(none["mean_err_3d"])

    IE.write_instance_evaluation(str(tmp_path / "e.csv"), ["obj_a", "obj_b"], s)
    rows = list(csv.reader(open(tmp_path / "e.csv")))
    assert rows[0] == ["object"] + list(IE.SUMMARY_COLUMNS) and [r[0] for r in rows[1:]] == ["obj_a", "obj_b", "all"]
    assert rows[3][1:4] == ["4", "5", "3"] and float(rows[3][4]) == 0.25 and float(rows[1][8]) == 17.0
    n = IE.write_instance_matches(str(tmp_path / "m.csv"), ["obj_a", "obj_b"], tally, rec, images=["im0", "im1"])
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert n == 4 == len(rows) - 1 and rows[0] == ["image", "object", "instance", "slot", "err_2d", "err_3d", "valid_3d", "valid_2d"]
    assert rows[1] == ["im0", "obj_a", "0", "2", "1", "4", "1", "1"] and rows[3] == ["im1", "obj_a", "0", "-1", "0", "0", "0", "0"]
    assert rows[4][:4] == ["im1", "obj_b", "0", "0"]


def test_crop_cameras_moves_the_principal_point():
    offsets = np.array([[176, 240, 0, 0, 0, 0, 0, 1, 640, 480], [10, 20, 0, 0, 0, 0, 0, 1, 640, 480]], np.float32)
    cams = IE.crop_cameras(K, offsets)
    assert np.allclose(cams[0], [[K[0, 0], 0, K[0, 2] - 240], [0, K[1, 1], K[1, 2] - 176], [0, 0, 1]], atol=1e-9)
    assert np.allclose(cams[1][:2, 2], [K[0, 2] - 20, K[1, 2] - 10], atol=1e-9)


def test_symmetry_flags_of_a_mesh_folder(tmp_path):
    import json

    assert IE.symmetric_from_models_info(str(tmp_path), ["obj_000001", "obj_000002"], [7862, 100]).tolist() == [1, 0]      # no file: the count rule
    json.dump({"1": {"diameter": 1.0}, "2": {"diameter": 1.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}},
              open(tmp_path / "models_info.json", "w"))
    assert IE.symmetric_from_models_info(str(tmp_path), ["obj_000001", "obj_000002", "obj_000003"], [7862, 100, 3417]).tolist() == [0, 1, 1]


def test_selftest_passes():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "casapose_amd", "csrc"), "match-selftest"], capture_output=True, text=True)
    assert r.returncode == 0 and "match_selftest: ok" in r.stdout, r.stdout + r.stderr
