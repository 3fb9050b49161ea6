"""cp_bop_errors_f32 (csrc/bop_errors.hip), DeviceBopScorer and util_scripts/bop_score.py on the GPU against tests/bop_reference.py, an fp64
NumPy restatement fed the same fp32-rounded inputs as the device.

Gates (those of tests/test_gpu_pose_eval.py, derived from the arithmetic, with one more rounding for the composed ground-truth pose times symmetry).
S0 = the largest |camera-frame coordinate| of a case; every case keeps z >= S0 / 2 (asserted):
  3-D: |dev - ref| <= 4e-6 * S0.  A transformed coordinate is three fp32 FMAs, <= 3 * 2^-24 * S0 per point, and the composed matrix adds one
       rounding of each entry; a distance takes two points and three coordinates: about 7e-7 * S0, so the gate leaves about 5x.
  2-D: |dev - ref| <= 2e-6 * (f + max(W, H)): the same argument through the projection.
A maximum or minimum of values that are each within a gate of their references is within that gate of the reference's maximum or minimum.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bop_reference as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K32 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
GATE_2D = 2e-6 * (float(K32[1, 1]) + 640.0)
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def gate_3d(s):
    return 4e-6 * s


def rodrigues(rv):
    from casapose_amd.pose_estimation import pnp as P

    return P.rodrigues(np.asarray(rv, np.float64))


def rot_z(th):
    return np.array([[math.cos(th), -math.sin(th), 0.0], [math.sin(th), math.cos(th), 0.0], [0.0, 0.0, 1.0]])


def pose32(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32)


def ring(n, radius=80.0, wave=0.0):
    a = 2.0 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a), wave * np.sin(3.0 * a)], axis=1).astype(np.float32)


def z_rotations(count):
    """`count` transforms: the identity and the turns by 2 pi k / count about the axis z through (3, -2, 5)"""
    if count == 315:
        return B.symmetry_set({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [3.0, -2.0, 5.0]}]})
    c = np.array([3.0, -2.0, 5.0])
    out = [IDENT]
    for k in range(1, count):
        R = rot_z(2.0 * np.pi * k / count)
        out.append(np.hstack([R, (c - R @ c).reshape(3, 1)]))
    return np.stack(out)


def reference(mesh, est, gt, K, syms32):
    """fp64 on the fp32-rounded inputs -> (mssd [S], mspd [S], S0, smallest z)"""
    return B.per_symmetry_errors(mesh.astype(np.float64), est.astype(np.float64), gt.astype(np.float64), K.astype(np.float64),
                                 syms32.astype(np.float64))


def check(where, dev3, dev2, ref3, ref2, s0, zmin):
    assert zmin >= s0 / 2, where
    d3, d2 = np.abs(np.asarray(dev3, np.float64) - ref3).max(), np.abs(np.asarray(dev2, np.float64) - ref2).max()
    print("%s max |mssd - ref| = %.3g (gate %.3g), max |mspd - ref| = %.3g (gate %.3g)" % (where, d3, gate_3d(s0), d2, GATE_2D))
    assert np.all(np.isfinite(dev3)) and np.all(np.isfinite(dev2)), where
    assert d3 <= gate_3d(s0), where
    assert d2 <= GATE_2D, where


# ---- 1. ring meshes: the per-(pair, symmetry) maxima --------------------------------------------------------------------------------------
RING_SIZES = ["1", "63", "64", "65", "255", "256", "257", "T-1", "T", "T+1", "2*T+1"]     # T = cp_bop_errors_tile()
SYM_COUNTS = ["1", "2", "315", "G-1", "G+1"]                                              # G = cp_bop_errors_sym_group()


@pytest.mark.parametrize("symmetries", SYM_COUNTS)
@pytest.mark.parametrize("size", RING_SIZES)
def test_ring_meshes(device, hip_lib, size, symmetries):
    from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer

    T, G = hip_lib.cp_bop_errors_tile(), hip_lib.cp_bop_errors_sym_group()
    n, sc = eval(size, {"T": T}), eval(symmetries, {"G": G})
    mesh = ring(n, 80.0, wave=10.0)
    syms = z_rotations(sc)
    syms32 = syms.astype(np.float32)
    padded = np.full((1, n + 5, 3), np.nan, np.float32)            # rows n .. vmax-1 must never be read
    padded[0, :n] = mesh
    Rg, tg = rodrigues([0.4, -0.7, 0.3]), [30.0, -20.0, 900.0]
    Rh, th = rodrigues([-0.2, 0.5, 1.1]), [-45.0, 25.0, 1100.0]
    gt = np.stack([pose32(Rg, tg), pose32(Rh, th), pose32(Rg, tg)])
    est = np.stack([pose32(Rg @ rot_z(1.2345), np.array(tg) + [0.5, -0.25, 2.0]),
                    pose32(Rh @ rodrigues([0.02, -0.01, 0.4]), np.array(th) + [-1.0, 0.75, 3.0]), np.zeros((3, 4), np.float32)])
    scorer = DeviceBopScorer(padded, [n], [syms], device)
    assert scorer.smax == sc
    mssd, mspd = scorer.errors(est, gt, K32, [0, 0, 0], per_symmetry=True)
    per3, per2 = scorer.last_per_symmetry
    assert per3.shape == per2.shape == (3, sc) and mssd.dtype == mspd.dtype == np.float32
    for p in (0, 1):
        r3, r2, s0, zmin = reference(mesh, est[p], gt[p], K32, syms32)
        check("ring n=%d S=%d pair %d:" % (n, sc, p), per3[p], per2[p], r3, r2, s0, zmin)
        assert abs(float(mssd[p]) - r3.min()) <= gate_3d(s0) and abs(float(mspd[p]) - r2.min()) <= GATE_2D
        assert mssd[p] == per3[p].min() and mspd[p] == per2[p].min()
    assert np.isposinf(mssd[2]) and np.isposinf(mspd[2]) and np.all(np.isposinf(per3[2])) and np.all(np.isposinf(per2[2]))


# ---- 2. the minimum is taken ------------------------------------------------------------------------------------------------------------
def test_exact_discrete_symmetry_gives_zero_at_its_index(device):
    from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer

    rng = np.random.default_rng(5)
    half = rng.uniform(-60, 60, (150, 3)).astype(np.float32)
    mesh = np.concatenate([half, half * np.array([-1, -1, 1], np.float32)])       # (x, y, z) and (-x, -y, z): exact in fp32
    s1 = np.hstack([np.diag([-1.0, -1.0, 1.0]), np.zeros((3, 1))])
    gt = pose32(rodrigues([0.3, 0.2, -0.5]), [12.0, -7.0, 820.0])
    est = gt * np.array([-1, -1, 1, 1], np.float32)                               # gt * S1, exactly
    syms = np.stack([IDENT, s1])
    r3, r2, s0, zmin = reference(mesh, est, gt, K32, syms.astype(np.float32))
    assert r3[0] > 100.0 > 1000 * gate_3d(s0) and r2[0] > 50.0 > 1000 * GATE_2D and r3[1] == 0.0 and r2[1] == 0.0
    scorer = DeviceBopScorer(mesh[None], [len(mesh)], [syms], device)
    mssd, mspd = scorer.errors(est[None], gt[None], K32, [0], per_symmetry=True)
    per3, per2 = scorer.last_per_symmetry
    check("exact 180 degrees:", per3[0], per2[0], r3, r2, s0, zmin)
    assert mssd[0] <= gate_3d(s0) and mspd[0] <= GATE_2D
    assert int(np.argmin(per3[0])) == 1 and int(np.argmin(per2[0])) == 1 and mssd[0] == per3[0, 1] and mspd[0] == per2[0, 1]
    # without the symmetry the same estimate is far off
    plain = DeviceBopScorer(mesh[None], [len(mesh)], [IDENT[None]], device)
    m3, m2 = plain.errors(est[None], gt[None], K32, [0])
    assert abs(float(m3[0]) - r3[0]) <= gate_3d(s0) and abs(float(m2[0]) - r2[0]) <= GATE_2D


# ---- 3. continuous symmetry -------------------------------------------------------------------------------------------------------------
def test_continuous_symmetry_leaves_at_most_half_a_step(device):
    from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer, symmetry_transforms

    r = 80.0
    mesh = ring(720, r)
    assert np.linalg.norm(mesh[:, :2].astype(np.float64), axis=1).max() <= r * (1 + 1e-7)
    syms = symmetry_transforms({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    assert syms.shape == (315, 3, 4)
    Rg, tg = rodrigues([0.4, -0.7, 0.3]), [30.0, -20.0, 900.0]
    gt, est = pose32(Rg, tg), pose32(Rg @ rot_z(1.2345), tg)
    r3, r2, s0, zmin = reference(mesh, est, gt, K32, syms.astype(np.float32))
    bound = r * math.pi / 315                     # the residual turn is at most half a step, pi / 315, and a chord is shorter than its arc
    assert 0.0 < r3.min() <= bound and r3[0] > 50.0
    scorer = DeviceBopScorer(mesh[None], [720], [syms], device)
    mssd, mspd = scorer.errors(est[None], gt[None], K32, [0], per_symmetry=True)
    per3, per2 = scorer.last_per_symmetry
    check("continuous:", per3[0], per2[0], r3, r2, s0, zmin)
    print("continuous: e_MSSD %.6g (reference %.6g, bound %.6g)" % (mssd[0], r3.min(), bound))
    assert 0.0 < mssd[0] <= bound + gate_3d(s0) and abs(float(mssd[0]) - r3.min()) <= gate_3d(s0) and abs(float(mspd[0]) - r2.min()) <= GATE_2D


# ---- 4. padding -------------------------------------------------------------------------------------------------------------------------
def test_padded_vertices_and_symmetries_take_no_part(device):
    """Two objects, 5 and 300 vertices in one vmax = 300 array, 1 and 3 symmetries in smax = 3.  Both meshes sit 200 mm off the model origin and
    the estimate is the ground truth turned about the mesh's centre, so the zero-padded vertex (the origin) would be the farthest-moved point.
    The padded symmetry rows of object 0 are overwritten on the device with the transform that brings the error to zero: reading one would
    lower the minimum."""
    import torch

    from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer

    rng = np.random.default_rng(9)
    c = np.array([200.0, 0.0, 0.0])
    counts = [5, 300]
    mesh = np.zeros((2, 300, 3), np.float32)
    for o, n in enumerate(counts):
        mesh[o, :n] = rng.uniform(-30, 30, (n, 3)) + c
    about = lambda R: np.hstack([R, (c - R @ c).reshape(3, 1)])   # noqa: E731  (x -> R (x - c) + c)
    syms = [IDENT[None], np.stack([IDENT, about(rot_z(2 * np.pi / 3)), about(rot_z(4 * np.pi / 3))])]
    delta = about(rodrigues([0.02, 0.05, 0.1]))
    G = np.eye(4)
    Rg, tg = rodrigues([0.3, -0.4, 0.2]), np.array([-150.0, 20.0, 950.0])
    G[:3, :3], G[:3, 3] = Rg, tg
    D = np.eye(4)
    D[:3] = delta
    gt, est = G[:3].astype(np.float32), (G @ D)[:3].astype(np.float32)
    scorer = DeviceBopScorer(mesh, counts, syms, device)
    assert scorer.smax == 3 and list(scorer.sym_counts_host) == [1, 3]
    scorer.syms[0, 1:] = torch.from_numpy(delta.astype(np.float32).reshape(12)).to(device)
    mssd, mspd = scorer.errors(np.stack([est, est]), np.stack([gt, gt]), K32, [0, 1], per_symmetry=True)
    per3, per2 = scorer.last_per_symmetry
    for o in (0, 1):
        r3, r2, s0, zmin = reference(mesh[o, :counts[o]], est, gt, K32, syms[o].astype(np.float32))
        n = len(r3)
        check("padding, object %d:" % o, per3[o, :n], per2[o, :n], r3, r2, s0, zmin)
        assert np.all(np.isposinf(per3[o, n:])) and np.all(np.isposinf(per2[o, n:]))
        assert abs(float(mssd[o]) - r3.min()) <= gate_3d(s0) and abs(float(mspd[o]) - r2.min()) <= GATE_2D
        # the padded vertex and the padded symmetry would each show: the origin moves far more, the extra transform brings the error to ~0
        with_origin, _, _, _ = reference(np.vstack([mesh[o, :counts[o]], np.zeros((1, 3), np.float32)]), est, gt, K32, syms[o].astype(np.float32))
        assert with_origin.min() > r3.min() + 5.0 > 1000 * gate_3d(s0)
    zero, _, _, _ = reference(mesh[0, :5], est, gt, K32, delta[None].astype(np.float32))
    assert zero[0] < 1e-3 and float(mssd[0]) > 1.0


# ---- 5. other device cases --------------------------------------------------------------------------------------------------------------
def test_zero_pose_is_never_correct_and_calls_repeat_bit_for_bit(device):
    from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer, greedy_matches

    mesh = ring(300, 80.0, wave=10.0)
    syms = z_rotations(17)
    gt = pose32(rodrigues([0.4, -0.7, 0.3]), [30.0, -20.0, 900.0])
    est = np.stack([pose32(rodrigues([0.4, -0.7, 0.3]) @ rot_z(0.3), [31.0, -20.0, 902.0]), np.zeros((3, 4), np.float32)])
    scorer = DeviceBopScorer(mesh[None], [300], [syms], device)
    a3, a2 = scorer.errors(est, np.stack([gt, gt]), K32, [0, 0], per_symmetry=True)
    pa = [x.copy() for x in scorer.last_per_symmetry]
    assert np.isfinite(a3[0]) and np.isfinite(a2[0]) and np.isposinf(a3[1]) and np.isposinf(a2[1])
    assert greedy_matches(np.array([[a3[1]]]), 1e30) == 0 and greedy_matches(np.array([[a3[0]]]), 1e30) == 1
    b3, b2 = scorer.errors(est, np.stack([gt, gt]), K32, [0, 0], per_symmetry=True)
    assert a3.tobytes() == b3.tobytes() and a2.tobytes() == b2.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pa, scorer.last_per_symmetry))


def test_more_pairs_than_a_grid_dimension(device):
    """70 000 pairs of a one-vertex mesh in one errors() call: nothing to compute, but the pair index passes 65535."""
    from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer

    n = 70000
    mesh = np.array([[[10.0, -5.0, 3.0]]], np.float32)
    gt = np.tile(pose32(rodrigues([0.4, -0.7, 0.3]), [30.0, -20.0, 900.0]), (n, 1, 1))
    est = gt.copy()
    i = np.arange(n)
    est[:, 0, 3] += (0.001 * i).astype(np.float32)                 # pair i is i micrometres-times-1000 to the right
    est[:, 2, 3] += ((i % 7) - 3).astype(np.float32)
    scorer = DeviceBopScorer(mesh, [1], [IDENT[None]], device)
    mssd, mspd = scorer.errors(est, gt, K32, np.zeros(n, np.int64))
    assert mssd.shape == mspd.shape == (n,) and np.all(np.isfinite(mssd)) and np.all(np.isfinite(mspd))
    for p in (0, 65535, n - 1):
        r3, r2, s0, zmin = reference(mesh[0], est[p], gt[p], K32, IDENT[None].astype(np.float32))
        check("pair %d of %d:" % (p, n), mssd[p:p + 1], mspd[p:p + 1], r3, r2, s0, zmin)
    assert mssd[65535] > 65.0 and mssd[n - 1] > 69.0             # each pair got its own record


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
def _write_ply(path, vertices):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(vertices))
        for v in vertices:
            f.write("%r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))


def test_score_script_end_to_end(device, tmp_path):
    from casapose_amd.utils.io_utils import write_poses

    root = tmp_path / "bop" / "toy"
    models, scene = root / "models_eval", root / "test" / "000001"
    os.makedirs(models)
    os.makedirs(scene)
    # object 1: 400 vertices with an exact 180 degree symmetry about z; object 2: a ring of 500 about z
    rng = np.random.default_rng(31)
    half = rng.uniform(-50, 50, (200, 3)).astype(np.float32)
    meshes = {1: np.concatenate([half, half * np.array([-1, -1, 1], np.float32)]), 2: ring(500, 70.0, wave=15.0)}
    flip = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    info = {"1": {"diameter": 150.0, "symmetries_discrete": [flip]},
            "2": {"diameter": 145.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    for o, v in meshes.items():
        _write_ply(str(models / ("obj_%06d.ply" % o)), v)
    (models / "models_info.json").write_text(json.dumps(info))
    K = K32.astype(np.float64)

    def inst(obj, rv, t, visib):
        return {"obj_id": obj, "R": rodrigues(rv), "t": np.asarray(t, np.float64), "visib": visib}

    # image 0: both objects; image 1: two instances of object 1 and one of object 2; image 2: object 1 nearly hidden, object 2
    frames = {0: [inst(1, [0.3, 0.2, -0.5], [12, -7, 820], 0.9), inst(2, [0.4, -0.7, 0.3], [-80, 40, 900], 0.8)],
              1: [inst(1, [-0.2, 0.5, 0.1], [100, 10, 1000], 1.0), inst(1, [0.1, 0.1, 0.9], [-120, -30, 950], 0.6), inst(2, [0.0, 0.6, 0.2], [0, 90, 870], 0.7)],
              2: [inst(1, [0.5, 0.0, 0.0], [30, 30, 780], 0.05), inst(2, [-0.3, 0.3, 0.3], [60, -50, 990], 1.0)]}
    (scene / "scene_gt.json").write_text(json.dumps({str(im): [{"cam_R_m2c": g["R"].reshape(-1).tolist(), "cam_t_m2c": g["t"].tolist(), "obj_id": g["obj_id"]}
                                                               for g in gl] for im, gl in frames.items()}))
    (scene / "scene_camera.json").write_text(json.dumps({str(im): {"cam_K": K.reshape(-1).tolist(), "depth_scale": 1.0} for im in frames}))
    (scene / "scene_gt_info.json").write_text(json.dumps({str(im): [{"bbox_obj": [0, 0, 10, 10], "bbox_visib": [0, 0, 10, 10], "px_count_all": 100,
                                                                    "px_count_valid": 100, "px_count_visib": int(100 * g["visib"]),
                                                                    "visib_fract": g["visib"]} for g in gl] for im, gl in frames.items()}))

    # estimates: the ground truth times a symmetry of the object, turned and shifted by an amount chosen per image
    def estimate(g, sym_turn, rv, dt):
        return pose32(g["R"] @ rot_z(sym_turn) @ rodrigues(rv), g["t"] + np.asarray(dt, np.float64))

    zero = np.zeros((3, 4), np.float32)
    est = {0: {1: estimate(frames[0][0], math.pi, [0.0, 0.0, 0.0], [1.0, -0.5, 2.0]), 2: estimate(frames[0][1], 2.1, [0.03, 0.0, 0.0], [4.0, 3.0, 14.0])},
           1: {1: estimate(frames[1][1], 0.0, [0.0, 0.1, 0.0], [6.0, -2.0, 22.0]), 2: zero},                # object 1: one estimate, two instances
           2: {1: estimate(frames[2][0], 0.0, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]), 2: estimate(frames[2][1], 0.7, [0.0, 0.05, 0.0], [-9.0, 5.0, 38.0])}}
    out_dir = str(tmp_path / "run") + "/"
    names = ["obj_000001", "obj_000002"]
    rows = []
    for im in frames:
        gt_first = np.stack([next(pose32(g["R"], g["t"]) for g in frames[im] if g["obj_id"] == o) for o in (1, 2)])[:, None]
        write_poses(gt_first, np.stack([est[im][1], est[im][2]]), names, "000001_rgb_%06d" % im, out_dir)
        rows += [(1, im, o, 0.0 if not est[im][o].any() else 1.0, est[im][o].astype(np.float64)) for o in (1, 2)]

    # the reference, on the same numbers
    gts = {(1, im): [{"id": g["obj_id"], "R": g["R"], "t": g["t"], "visib_fract": g["visib"]} for g in gl] for im, gl in frames.items()}
    syms = {int(o): B.symmetry_set(e) for o, e in info.items()}
    want, pairs = B.score(rows, gts, {k: K for k in gts}, meshes, syms, {1: 150.0, 2: 145.0}, None, 640.0)
    assert want["targets"] == 6 and want["objects"]["1"]["targets"] == 3 and len(pairs) == 5
    for obj, e3, e2 in pairs:          # every error is at least 1 % away from every threshold
        d = {1: 150.0, 2: 145.0}[obj]
        assert all(abs(e3 - t * d) >= 0.01 * t * d for t in B.MSSD_T) and all(abs(e2 - t) >= 0.01 * t for t in B.MSPD_T), (obj, e3, e2)
    assert 0.0 < want["AR_MSSD"] < 1.0 and 0.0 < want["AR_MSPD"] < 1.0 and len(set(want["recall_mssd"])) > 1

    out_json = str(tmp_path / "scores.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "util_scripts", "bop_score.py"), "--result_file", out_dir + "bop_evaluation.csv",
                        "--dataset_path", str(root), "--split", "test", "--model_folder", "models_eval", "--image_width", "640", "--out", out_json],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "AR_MSSD_MSPD" in r.stdout and "obj      1:" in r.stdout and "all objects:" in r.stdout
    with open(out_json) as f:
        got = json.load(f)
    assert got["pairs"] == len(pairs) and "AR" not in got
    for key in ("targets", "recall_mssd", "recall_mspd", "AR_MSSD", "AR_MSPD", "AR_MSSD_MSPD"):
        assert got[key] == want[key], key
        for o in ("1", "2"):
            assert got["objects"][o][key] == want["objects"][o][key], (o, key)
    assert sorted(got["objects"]) == ["1", "2"]
