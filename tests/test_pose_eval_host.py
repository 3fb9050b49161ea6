"""CPU checks of the device pose evaluation (csrc/pose_eval.hip, pose_estimation/device_evaluation.py): the three C-ABI symbols, the argument
refusals of cp_pose_eval_f32, the packed pair record, and that the `evaluator` keyword changes nothing when it is not given.  No kernel is
launched here; the kernels are checked in tests/test_gpu_pose_eval.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cp_pose_eval_workspace_bytes", "cp_pose_eval_est_tile", "cp_pose_eval_f32")


@pytest.fixture(scope="module")
def lib():
    from casapose_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_pose_eval_symbols_are_declared_exported_and_bound(lib):
    from casapose_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "casapose_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), "%s is not declared in include/casapose_hip.h" % n
        assert hasattr(lib, n), "%s is not exported" % n
        assert n in bound, "%s is not bound in casapose_amd/_lib.py" % n
    assert len(bound["cp_pose_eval_f32"][1]) == 13 and bound["cp_pose_eval_workspace_bytes"][0] is C.c_size_t
    assert "pose_eval.hip" in open(os.path.join(ROOT, "casapose_amd", "csrc", "Makefile")).read()
    tile = lib.cp_pose_eval_est_tile()
    assert tile >= 64 and tile % 8 == 0
    # one fp64 (2-D, 3-D) pair of partial sums per 256-point chunk of every (image, object) pair
    assert lib.cp_pose_eval_workspace_bytes(2, 3, 257) == 2 * 3 * 2 * 2 * 8
    assert lib.cp_pose_eval_workspace_bytes(1, 8, 38325) == 8 * 150 * 2 * 8
    assert lib.cp_pose_eval_workspace_bytes(0, 3, 9) == 0 and lib.cp_pose_eval_workspace_bytes(1, 1, 0) == 0
    assert lib.cp_version() == _lib.ABI_VERSION      # additions only


def test_pose_eval_refuses_bad_arguments_before_any_launch(lib):
    """Never-dereferenced stand-in pointers: every call below is refused by its argument checks."""
    from casapose_amd import _lib

    p = lambda a: C.c_void_p(a)  # noqa: E731
    good = dict(points=p(4096), counts=p(8192), symmetric=p(12288), objects=3, vmax=100, pairs=p(16384), batch=2, allowed=5.0, workspace=p(20480),
                records=p(24576), e2=None, e3=None)
    bad = [dict(points=None), dict(counts=None), dict(symmetric=None), dict(pairs=None), dict(workspace=None), dict(records=None),
           dict(objects=0), dict(objects=-2), dict(batch=0), dict(batch=-1), dict(vmax=0), dict(vmax=-7), dict(batch=1 << 14, objects=8),
           dict(vmax=(1 << 24) + 1), dict(workspace=p(20484))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.cp_pose_eval_f32(a["points"], a["counts"], a["symmetric"], a["objects"], a["vmax"], a["pairs"], a["batch"], a["allowed"],
                                  a["workspace"], a["records"], a["e2"], a["e3"], None)
        assert rc == -1, change                                     # CP_ERR_INVALID
        assert lib.cp_last_error().startswith(b"cp_pose_eval_f32:"), change
    with pytest.raises(_lib.CasaposeHipError, match="objects, batch and vmax must be positive"):
        _lib.check(lib.cp_pose_eval_f32(p(4096), p(8192), p(12288), 3, 100, p(16384), 0, 5.0, p(20480), p(24576), None, None, None), "cp_pose_eval_f32")


def test_packed_pair_record_layout():
    """[b*oc][36]: estimated pose (12, row-major 3x4), ground-truth pose of instance 0 (12), K (9), diameter, valid, pad."""
    from casapose_amd.pose_estimation.device_evaluation import PAIR_FLOATS, pack_pairs

    b, oc, ic = 2, 3, 2
    est = (np.arange(b * oc * 12, dtype=np.float64).reshape(b, oc, 3, 4) + 0.25) * 1.5
    gt = -(np.arange(b * oc * ic * 12, dtype=np.float64).reshape(b, oc, ic, 3, 4) + 0.5)
    cams = np.stack([np.array([[572.4, 0.1, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]]) + n for n in range(b)])
    diam = 100.0 + np.arange(b * oc * ic, dtype=np.float64).reshape(b, oc, ic)
    valid = np.array([[1, 0, 1], [0, 1, 1]])
    rec = pack_pairs(est, gt, cams, diam, valid)
    assert rec.dtype == np.float32 and rec.shape == (b * oc, PAIR_FLOATS) and PAIR_FLOATS == 36
    # pair 4 = image 1, object 1, written out by hand
    e0, g0 = (12 * 4 + 0.25) * 1.5, -(12 * (4 * ic) + 0.5)
    want = [e0 + 1.5 * i for i in range(12)] + [g0 - i for i in range(12)] + [573.4, 1.1, 326.3, 1.0, 574.6, 243.0, 1.0, 1.0, 2.0] + [108.0, 1.0, 0.0]
    assert np.array_equal(rec[4], np.array(want, np.float32))
    assert list(rec[:, 34]) == [1, 0, 1, 0, 1, 1] and np.all(rec[:, 35] == 0)
    # one camera matrix for the whole batch, poses already flat, and packing into a caller's buffer
    buf = np.full((b * oc + 1, PAIR_FLOATS), np.nan, np.float32)
    out = pack_pairs(est.reshape(b, oc, 12), gt[:, :, :1], cams[0], diam[:, :, 0], valid.astype(np.float32), out=buf[:b * oc])
    assert out.base is buf or out is buf[:b * oc] or np.shares_memory(out, buf)
    assert np.array_equal(buf[:, 24:33][: b * oc], np.tile(cams[0].astype(np.float32).reshape(1, 9), (b * oc, 1)))
    assert np.array_equal(buf[:b * oc, :24], rec[:, :24]) and np.array_equal(buf[:b * oc, 33], rec[:, 33]) and np.all(np.isnan(buf[-1]))


def _scene(b=2, oc=3, v=40):
    from casapose_amd.pose_estimation import pnp as P

    rng = np.random.default_rng(12)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    mesh = rng.uniform(-50, 50, (oc, v, 3))
    kp3 = np.tile(rng.uniform(-50, 50, (1, oc, 1, 9, 3)), (b, 1, 1, 1, 1))
    gt = np.zeros((b, oc, 1, 3, 4))
    for n in range(b):
        for o in range(oc):
            gt[n, o, 0, :, :3] = P.rodrigues(rng.normal(0, 0.5, 3))
            gt[n, o, 0, :, 3] = [rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(700, 900)]
    est = gt[:, :, 0].copy()
    est[..., 3] += [0.5, -0.25, 2.0]
    est[0, 1] = 0                                     # a missing object
    seg = np.zeros((b, 16, 16, oc + 1), np.float32)
    for o in range(oc):
        seg[:, 4 * o:4 * o + 4, :, o + 1] = 1.0       # 64 pixels each
    seg[1, 8:12, :, 3] = 0.0                          # object 2 is not in image 1: its non-zero pose is a false positive
    counts = np.array([[v], [v - 7], [v - 1]], np.int32)
    return dict(points=np.zeros((b, oc, 9, 2)), poses=est, gt=gt, seg=seg, kp3=kp3, cams=np.tile(K, (b, 1, 1)), diam=np.full((b, oc, 1), 110.0),
                mesh=mesh, counts=counts)


def test_without_an_evaluator_nothing_changes(monkeypatch):
    """evaluator=None (and no keyword at all) is today's host path: _eval_points + evaluate_poses."""
    from casapose_amd.pose_estimation import pose_evaluation as E

    s = _scene()
    args = (s["points"], s["poses"], s["gt"], s["seg"], s["kp3"], s["cams"], s["diam"])
    kw = dict(evaluation_points=s["mesh"], object_points_3d_count=s["counts"], min_num=20)
    plain, poses, pts = E.evaluate_pose_estimates(*args, **kw)
    none, _, _ = E.evaluate_pose_estimates(*args, evaluator=None, **kw)
    b, oc = 2, 3
    tiled, cnt = E._eval_points(s["kp3"], s["mesh"], s["counts"], b, oc, 1)
    avail = E._objects_available(s["seg"], 20)
    e2, e3, v2, v3, miss, vcount, fp = E.evaluate_poses(s["poses"], s["gt"], s["points"], tiled, cnt, s["cams"], s["diam"], avail, 5.0)
    want = [v2, v3, vcount, np.zeros_like(v2), e2, e3, miss, fp]
    assert len(plain) == len(none) == 8 and poses is s["poses"] and pts is s["points"]
    for a, b_, c in zip(plain, none, want):
        assert a.dtype == c.dtype and np.array_equal(a, b_) and np.array_equal(a, c)
    assert list(plain[6]) == [0, 1, 0] and list(plain[7]) == [0, 0, 1] and list(plain[2]) == [2, 2, 1]   # the scene has a miss and a false positive


def test_with_an_evaluator_the_host_statistics_are_not_computed(monkeypatch):
    """With an evaluator neither the mesh tiling (_eval_points) nor the host evaluate_poses runs; the evaluator gets the reshaped poses,
    the availability flags and the 5 px bound, and its seven arrays are returned in evaluate_pose_estimates' order."""
    from casapose_amd.pose_estimation import pose_evaluation as E

    s = _scene()
    seen = {}

    class Recorder:
        def evaluate(self, poses, poses_gt, camera_matrixes, diameters, valid_points_filter, allowed_error_2d=5.0):
            seen.update(poses=poses, gt=poses_gt, cams=camera_matrixes, diam=diameters, valid=valid_points_filter, allowed=allowed_error_2d)
            return tuple(np.full(3, float(i), np.float32) for i in range(7))

    def refuse(*a, **k):
        raise AssertionError("the host path ran although an evaluator was given")

    monkeypatch.setattr(E, "_eval_points", refuse)
    monkeypatch.setattr(E, "evaluate_poses", refuse)
    stats, _, _ = E.evaluate_pose_estimates(s["points"], s["poses"].reshape(2, 3, 12), s["gt"], s["seg"], s["kp3"], s["cams"], s["diam"], min_num=20,
                                            evaluator=Recorder())
    assert [float(a[0]) for a in stats] == [2.0, 3.0, 5.0, 0.0, 0.0, 1.0, 4.0, 6.0]     # (e2, e3, v2, v3, miss, count, fp) -> the eight columns
    assert seen["poses"].shape == (2, 3, 3, 4) and seen["allowed"] == 5.0
    assert np.array_equal(seen["valid"], [[1, 1, 1], [1, 1, 0]]) and np.array_equal(seen["gt"], s["gt"])
    import inspect

    from casapose_amd import training

    for fn in (E.evaluate_pose_estimates, E.estimate_and_evaluate_poses, training.test_step):
        assert inspect.signature(fn).parameters["evaluator"].default is None


def test_environment_switch_selects_nothing_unless_set_and_meshes_are_given(monkeypatch):
    """CASAPOSE_DEVICE_EVAL: unset or 0 -> the host path; set without evaluation meshes (the 9-keypoint validation of the training driver)
    -> the host path too.  No device is touched in either case."""
    from casapose_amd.pose_estimation.device_evaluation import evaluator_from_environment

    mesh, counts = np.zeros((2, 5, 3), np.float32), np.full((2, 1), 5, np.int32)
    monkeypatch.delenv("CASAPOSE_DEVICE_EVAL", raising=False)
    assert evaluator_from_environment(mesh, counts, "cuda:0") is None
    monkeypatch.setenv("CASAPOSE_DEVICE_EVAL", "0")
    assert evaluator_from_environment(mesh, counts, "cuda:0") is None
    monkeypatch.setenv("CASAPOSE_DEVICE_EVAL", "1")
    assert evaluator_from_environment(None, None, "cuda:0") is None and evaluator_from_environment(mesh, None, "cuda:0") is None
