"""casapose_amd.twin.call on the CPU: one argument list reaches a kernel or its host twin, and what the header's pointee types can tell apart
is refused in Python before the library is entered.  No kernel is launched here: every device call below is refused first."""
import numpy as np
import pytest
import torch

from casapose_amd import _lib, twin
from casapose_amd.data_handler.device_scenes import DeviceScenes
from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
from casapose_amd.pose_estimation.device_pnp import hypothesis_table

H, W, OC = 8, 12, 1


@pytest.fixture(scope="module")
def scene():
    """one record of an 8 x 12 image with one object, and output arrays for it"""
    scenes = DeviceScenes(SyntheticSceneDataset(OC, (H, W), seed=0), "cuda:0")   # the host half touches no GPU
    records = np.ascontiguousarray(scenes.host_half(range(1))["records"].numpy())
    return records, lambda: twin.alloc(dict(img=((1, H, W, 3), np.float32), label=((1, H, W), np.uint8), target_seg=((1, H, W, OC + 1), np.float32),
                                            counts=((1, OC), np.int32)))


def scene_args(records, out):
    return (records, 1, OC, H, W, 1, out["img"], out["label"], out["target_seg"], out["counts"])


def test_host_call_equals_the_raw_twin(scene):
    records, outputs = scene
    lib, raw, got = _lib.load(), outputs(), outputs()
    assert lib.cp_render_scenes_host_f32(records.ctypes.data, 1, OC, H, W, 1, *(raw[k].ctypes.data for k in ("img", "label", "target_seg", "counts"))) == 0
    twin.call("cp_render_scenes_f32", *scene_args(records, got), host=True)
    assert raw["counts"][0, 0] == (raw["label"] == 1).sum() > 0 and np.ptp(raw["img"]) > 0   # the call rendered something
    for k in raw:
        assert np.array_equal(raw[k], got[k]), k
    # CPU tensors are host arrays too
    again = {k: torch.from_numpy(np.zeros_like(v)) for k, v in raw.items()}
    twin.call("cp_render_scenes_f32", *scene_args(torch.from_numpy(records), again), host=True)
    for k in raw:
        assert np.array_equal(raw[k], again[k].numpy()), k


def test_refusals_name_the_symbol_and_the_argument(scene):
    records, outputs = scene
    out = {k: np.zeros_like(v) for k, v in outputs().items()}
    wide = np.zeros((1, H, W, 6), np.float32)
    refused = [
        # (argument position, its replacement, keywords, text)
        (6, wide[..., ::2], dict(host=True), "cp_render_scenes_host_f32, argument 6 (float*): the array is not contiguous"),
        (6, out["img"].astype(np.float64), dict(host=True), "cp_render_scenes_host_f32, argument 6 (float*): the array holds float64"),
        (0, records.astype(np.float32), dict(host=True), "cp_render_scenes_host_f32, argument 0 (double*): the array holds float32"),
        (0, records, dict(stream=0), "cp_render_scenes_f32, argument 0 (double*): a NumPy array for a device entry point"),
        (0, torch.from_numpy(records), dict(stream=0), "cp_render_scenes_f32, argument 0 (double*): a CPU tensor for a device entry point"),
        (7, [0] * (H * W), dict(host=True), "cp_render_scenes_host_f32, argument 7 (uint8_t*): a tensor, a NumPy array or None is expected (got list)"),
        (0, records, dict(host=True, stream=0), "cp_render_scenes_host_f32: a host twin takes no stream"),
        (0, records, dict(), "cp_render_scenes_f32: a device call needs a stream"),
    ]
    for position, value, kw, text in refused:
        args = list(scene_args(records, out))
        args[position] = value
        with pytest.raises(_lib.CasaposeHipError) as e:
            twin.call("cp_render_scenes_f32", *args, **kw)
        assert str(e.value) == text
    with pytest.raises(_lib.CasaposeHipError, match="cp_pose_eval_f32 has no host twin"):
        twin.call("cp_pose_eval_f32", *([None] * 12), host=True)
    with pytest.raises(_lib.CasaposeHipError, match="cp_render_scenes_f32 takes 10 arguments before the stream"):
        twin.call("cp_render_scenes_f32", *scene_args(records, out)[:-1], host=True)
    with pytest.raises(_lib.CasaposeHipError, match="cp_conv_pack_weights_host is no entry point"):
        twin.call("cp_conv_pack_weights_host", None, host=True)
    assert not any(v.any() for v in out.values())   # nothing above entered the library


def pnp_args(table):
    """one (image, object) pair of five points in front of the LINEMOD camera"""
    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float32)
    x3 = np.array([[0, 0, 0], [50, 0, 0], [0, 50, 0], [0, 0, 50], [-40, 30, 20]], np.float32).reshape(1, 1, 5, 3)
    cam = x3[0, 0] + np.array([20.0, -10.0, 800.0], np.float32)
    xy = (cam @ K.T)[:, :2] / (cam @ K.T)[:, 2:]
    out = twin.alloc(dict(poses=((1, 1, 3, 4), np.float32), info=((1, 1, 4), np.int32), cost=((1, 1, 2), np.float32)))
    return (np.ascontiguousarray(xy.reshape(1, 1, 5, 2), np.float32), x3, K, 0, None, np.ones((1, 1), np.int32), table, 1, 1, 5, len(table), 12.0,
            out["poses"], out["info"], out["cost"]), out


def test_a_rejection_inside_the_library_names_the_called_symbol():
    args, out = pnp_args(hypothesis_table(5))
    twin.call("cp_pnp_f64", *args, host=True)
    assert out["info"][0, 0, 0] == 0 and abs(out["poses"][0, 0, 2, 3] - 800.0) < 1e-2
    bad = hypothesis_table(9).copy()
    bad[3, 4] = 9
    args, _ = pnp_args(bad)
    args = args[:9] + (9,) + args[10:]   # n = 9: the table may name points 0..8
    with pytest.raises(_lib.CasaposeHipError, match="cp_pnp_host_f64 failed.*hypothesis 3 names point 9 of 9"):
        twin.call("cp_pnp_f64", *args, host=True)


def test_a_void_workspace_takes_any_element_type():
    """cp_model_prep_f32's `void* workspace`: the same four-vertex object through uint8, uint32 and float64 workspaces"""
    verts = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 1], [0, 0, 0]], np.float32)
    size = int(_lib.load().cp_model_prep_workspace_bytes(1, 4))
    results = []
    for dtype in (np.uint8, np.uint32, np.float64):
        out = twin.alloc(dict(diameter_sq=((1,), np.float64), box=((1, 6), np.float32), keypoints=((1, 3, 3), np.float32), indices=((1, 2), np.int32),
                              status=((1,), np.int32)), zero=True)
        workspace = np.empty(size // np.dtype(dtype).itemsize + 1, dtype)
        twin.call("cp_model_prep_f32", verts, 4, np.zeros(1, np.int64), np.full(1, 4, np.int32), 1, 3, out["diameter_sq"], out["box"], out["keypoints"],
                  out["indices"], out["status"], workspace, size, host=True)
        assert out["status"][0] == 0 and out["diameter_sq"][0] == 25.0
        results.append(out)
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]) and np.array_equal(results[0][k], results[2][k]), k
    with pytest.raises(_lib.CasaposeHipError, match=r"cp_model_prep_host_f32, argument 2 \(long long\*\): the array holds int32"):
        twin.call("cp_model_prep_f32", verts, 4, np.zeros(1, np.int32), np.full(1, 4, np.int32), 1, 3, out["diameter_sq"], out["box"], out["keypoints"],
                  out["indices"], out["status"], workspace, size, host=True)


def test_array_and_alloc_place_data_where_the_call_runs():
    a = twin.array([[1, 2], [3, 4]], np.float32)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous
    t = twin.array(torch.arange(6).reshape(2, 3).t(), np.int32)
    assert isinstance(t, np.ndarray) and t.dtype == np.int32 and t.flags.c_contiguous and t.tolist() == [[0, 3], [1, 4], [2, 5]]
    out = twin.alloc(dict(a=((2, 3), np.float64), b=((0,), np.uint8)), zero=True)
    assert out["a"].dtype == np.float64 and out["a"].shape == (2, 3) and not out["a"].any() and out["b"].shape == (0,)
    cpu = twin.alloc(dict(a=((2, 3), np.int32)), torch.device("cpu"), zero=True)
    assert isinstance(cpu["a"], torch.Tensor) and cpu["a"].dtype == torch.int32 and tuple(cpu["a"].shape) == (2, 3)
