"""cp_pose_verify_host_i32 -- the host twin of the pose verification's kernel, the same header the device kernels compile -- against the NumPy
restatement (tests/verify_reference.py) on the hand case, on seeded planes and on planes rendered by cp_render_masks_host_u8 from the scenes of
tests/contour_cases.py.  No GPU is needed.  The helpers also serve tests/test_gpu_pose_verify.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import verify_cases as VC
import verify_reference as VR
from test_verify_reference import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_FILL = -7          # what the counts hold before the call: every word of them is written


def run(case, device=None, split=1, fill=0xA5, **change):
    """cp_pose_verify_i32 on `device`, or its host twin (device None), over a case of tests/verify_cases.py; the workspace pre-filled with the
    byte `fill`, the counts with COUNT_FILL -> counts int32 [njobs, 8] as a NumPy array"""
    from casapose_amd import _lib, twin

    lib = _lib.load()
    c = dict(case, **change)
    nplanes, H, W = c["planes"].shape
    images, ld = len(c["labels"]), c["field"].shape[-1]
    jobs = np.asarray(c["jobs"], np.int32).reshape(-1, 4)
    n = len(jobs)
    size = int(lib.cp_pose_verify_workspace_bytes(images))
    assert size == images * 256 * 4
    stream = None
    if device is not None:
        import torch

        stream = torch.cuda.current_stream(device).cuda_stream
    arg = dict(planes=twin.array(c["planes"], np.uint32, device), records=twin.array(c["records"], np.int32, device),
               inst_counts=twin.array(c["inst_counts"], np.int32, device), labels=twin.array(c["labels"], np.uint8, device),
               field=twin.array(c["field"], np.float32, device), kp2d=twin.array(np.asarray(c["kp2d"], np.float64).reshape(n, c["kp"], 2), np.float64, device),
               jobs=twin.array(jobs, np.int32, device), counts=twin.array(np.full((n, 8), COUNT_FILL, np.int32), np.int32, device),
               work=twin.array(np.full(size, fill, np.uint8), np.uint8, device))
    twin.call("cp_pose_verify_i32", arg["planes"], arg["records"], nplanes, H, W, arg["inst_counts"], len(c["inst_counts"]), int(c["imax"]), arg["labels"],
              arg["field"], images, ld, int(c["dir_off"]), int(c["kp"]), arg["kp2d"], arg["jobs"], n, float(c["sample_offset"]), float(c["cos_min"]), int(split),
              arg["counts"], arg["work"], size, host=device is None, stream=stream)
    return arg["counts"] if device is None else arg["counts"].cpu().numpy()


def host_counts(name):
    if name not in _host:
        _host[name] = run(VC.CASES[name]())
        _host[name].setflags(write=False)
    return _host[name]


_host = {}


@pytest.mark.parametrize("name", list(VC.CASES))
def test_twin_equals_reference_exactly(name):
    case = VC.CASES[name]()
    got, want = host_counts(name), reference(case)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (name, np.argwhere(got != want)[:6].tolist())
    if name == "hand":
        assert got.tolist() == [list(VC.HAND_A), list(VC.HAND_B)]
    else:      # the case exercises what it is there for
        assert got[:, VR.HIDDEN].any() and got[:, VR.ON_OTHER].any() and got[:, VR.ON_BACKGROUND].any()
        assert (got[:, VR.INLIERS] > 0).any() and (got[:, VR.INLIERS] < got[:, VR.PAIRS]).any()
        assert (got[:, VR.PAIRS] < case["kp"] * got[:, VR.ON_LABEL]).any()           # a direction or a keypoint made no pair
    if name == "production":
        bad = np.flatnonzero(case["jobs"][:, 1] == 8)
        assert len(bad) == 1 and not got[bad].any() and (got[case["jobs"][:, 2] == 255, VR.ON_LABEL] > 0).any()
        twice = np.flatnonzero(case["jobs"][:, 1] == 1)
        assert len(twice) == 2 and got[twice[0], VR.RENDERED] == got[twice[1], VR.RENDERED] > 0


def test_tile_and_box_sizes():
    from casapose_amd import _lib

    T = _lib.load().cp_pose_verify_tile()
    assert T == VC.TILE and T % 64 == 0
    r = VC.tiles()["records"]
    assert [(int(w) + 1) * (int(h) + 1) for w, h in r[:3, 4:6]] == [T - 1, T, T + 1] and VC.tiles()["planes"].shape[2] % 64 != 0


@pytest.mark.parametrize("split", [3, 64])
def test_split_and_workspace_contents_change_nothing(split):
    for name in ("tiles", "production"):
        assert run(VC.CASES[name](), split=split, fill=0x3C).tobytes() == host_counts(name).tobytes()


def test_refused_jobs_leave_zeros():
    case = VC.hand()
    big = 2 ** 31 - 1
    jobs = [(0, 0, 1, 0), (1, 0, 1, 0), (-1, 0, 1, 0), (0, 2, 1, 0), (0, -1, 1, 0), (0, big, 1, 0), (big, big, big, big), (0, 0, 0, 0), (0, 0, 256, 0),
            (0, 0, -3, 0), (0, 1, 2, 5)]
    kp2d = np.concatenate([np.tile(case["kp2d"][:1], (len(jobs) - 1, 1, 1)), case["kp2d"][1:]])
    got = run(case, jobs=np.array(jobs, np.int32), kp2d=kp2d)
    assert got[0].tolist() == list(VC.HAND_A) and got[-1].tolist() == list(VC.HAND_B) and not got[1:-1].any()
    # three planes' worth of records and planes, two frames' worth named: plane 2 lies in frame 1, beyond the one inst_count
    planes = np.concatenate([case["planes"], case["planes"][:1]])
    records = np.concatenate([case["records"], case["records"][:1]])
    got = run(case, planes=planes, records=records, jobs=np.array([(0, 2, 1, 0), (0, 0, 1, 0)], np.int32), kp2d=case["kp2d"][[0, 0]])
    assert not got[0].any() and got[1].tolist() == list(VC.HAND_A)


def raw_args(case):
    """the host twin's argument list over a case, as ctypes values, and the arrays that keep the pointers alive"""
    from casapose_amd import _lib

    lib = _lib.load()
    nplanes, H, W = case["planes"].shape
    n, images = len(case["jobs"]), len(case["labels"])
    keep = [np.ascontiguousarray(case[k]) for k in ("planes", "records", "inst_counts", "labels", "field", "kp2d", "jobs")]
    keep += [np.zeros((n, 8), np.int32), np.zeros(images * 256, np.int32)]
    ptr = [a.ctypes.data for a in keep]
    args = [ptr[0], ptr[1], nplanes, H, W, ptr[2], len(case["inst_counts"]), case["imax"], ptr[3], ptr[4], images, case["field"].shape[-1], case["dir_off"],
            case["kp"], ptr[5], ptr[6], n, case["sample_offset"], case["cos_min"], 1, ptr[7], ptr[8], images * 256 * 4]
    return lib, args, keep


REFUSALS = [(0, None, "null pointer"), (21, None, "null pointer"), (13, 0, "kp must lie in [1, 32]"), (13, 33, "kp must lie in [1, 32]"),
            (2, 0, "must be positive"), (6, 0, "must be positive"), (10, 0, "must be positive"), (16, 0, "must be positive"),
            (7, 0, "instances_max must lie in [1, 256]"), (7, 257, "instances_max must lie in [1, 256]"), (3, 16385, "H and W must lie in"),
            (4, 0, "H and W must lie in"), (2, 2 ** 31 - 1, "is too large"), (10, 2 ** 22 + 1, "images must be at most"),
            (11, 2, "dir_off + 2 kp <= ld"), (11, 4097, "dir_off + 2 kp <= ld"), (12, -1, "dir_off + 2 kp <= ld"), (12, 3, "dir_off + 2 kp <= ld"),
            (17, -0.01, "sample_offset must lie in [0, 1]"), (17, 1.5, "sample_offset must lie in [0, 1]"), (18, -0.1, "cos_min must lie in [0, 1]"),
            (18, 1.01, "cos_min must lie in [0, 1]"), (18, float("nan"), "cos_min must lie in [0, 1]"), (19, 0, "split must lie in [1, 64]"),
            (19, 65, "split must lie in [1, 64]"), (16, 2 ** 31 - 1, "above 2^31 - 1 blocks"), (22, 1023, "below cp_pose_verify_workspace_bytes"),
            (1, "odd", "4-byte aligned"), (14, "odd", "kp2d must be 8-byte aligned")]


@pytest.mark.parametrize("at,value,word", REFUSALS)
def test_refusals_by_name(at, value, word):
    lib, args, keep = raw_args(VC.hand())
    args[at] = args[at] + 1 if value == "odd" else value
    if (at, value) == (16, 2 ** 31 - 1):
        args[19] = 2
    for fn, stream in ((lib.cp_pose_verify_host_i32, ()), (lib.cp_pose_verify_i32, (None,))):      # the device entry refuses before any launch
        assert fn(*args, *stream) == -1
        text = lib.cp_last_error().decode()
        assert word in text and text.startswith("cp_pose_verify_host_i32" if not stream else "cp_pose_verify_i32:"), text


def test_pair_counts_must_fit():
    lib, args, keep = raw_args(VC.hand())
    args[3], args[4], args[13], args[11] = 16384, 16384, 8, 20      # refused before anything is read
    assert lib.cp_pose_verify_host_i32(*args) == -1 and "the pair counts would not fit" in lib.cp_last_error().decode()
    assert lib.cp_pose_verify_workspace_bytes(0) == 0 and lib.cp_pose_verify_workspace_bytes(2 ** 22 + 1) == 0


def test_twin_table_and_header():
    from casapose_amd import _lib

    assert _lib.TWIN_READERS == {"cp_pose_verify_i32": "cp_pose_verify_host_i32"} and _lib.ABI_VERSION == 302
    assert _lib.host_twin("cp_pose_verify_i32") == "cp_pose_verify_host_i32"
    assert "cp_pose_verify_i32" not in _lib.TWINS and "cp_pose_verify_i32" not in _lib.TWIN_STEPS and "cp_pose_verify_i32" not in _lib.TWIN_VARIANTS
    assert _lib.host_twin("cp_vsd_counts_i32") is None
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    p, i, d, z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    assert table["cp_pose_verify_tile"] == (C.c_int, []) and table["cp_pose_verify_workspace_bytes"] == (C.c_size_t, [i])
    assert table["cp_pose_verify_host_i32"] == (C.c_int, [p, p, i, i, i, p, i, i, p, p, i, i, i, i, p, p, i, d, d, i, p, p, z])
    assert table["cp_pose_verify_i32"][1] == table["cp_pose_verify_host_i32"][1] + [p]
    assert _lib.POINTEES["cp_pose_verify_i32"][:10] == ("uint32_t", "int32_t", None, None, None, "int32_t", None, None, "uint8_t", "float")
    text = open(_lib.HEADER_PATH).read()
    block = text[text.index("pose verification: a rendered estimate"):text.index("int cp_pose_verify_tile(void);")]
    assert "Added in ABI 302 without changing any earlier entry point" in block and "cp_pose_verify_host_i32 runs the same code serially" in block


def test_selftest_passes():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "casapose_amd", "csrc"), "verify-selftest"], capture_output=True, text=True)
    assert r.returncode == 0 and "verify_selftest: ok" in r.stdout, r.stdout + r.stderr


# ---- planes rendered by the renderer's host twin --------------------------------------------------------------------------------------------
def rendered_case(H, W):
    """the block scene of tests/contour_cases.py at its ground truth: block, occluder and cut object in one frame, verified against the very
    label map the renderer made of them, with directions towards keypoint 0 of the block everywhere"""
    import contour_cases as CC
    from casapose_amd import _lib

    if (H, W) in _rendered:
        return _rendered[H, W]
    occ, cut = CC.placements(W)
    frame = dict(cam=CC.CAM, instances=[(0, CC.BLOCK, CC.IC.BLOCK_GT), (1, CC.OCCLUDER, occ), (2, CC.CUT, cut)])
    r = CC.scene().renderer
    p = r.pack([frame])
    size = int(_lib.load().cp_render_masks_workspace_bytes(1, 3, H, W))
    planes = np.empty(size // 4, np.uint32)
    labels, records = r._render((r.verts, r.vert_counts, r.faces, r.face_counts), p, 1, H, W, CC.NEAR, CC.FAR, CC.SAMPLE_OFFSET, planes, size, None, None)
    rng = np.random.default_rng(8)
    kp2d = np.stack([rng.uniform(0, H, (3, 2)), rng.uniform(0, W, (3, 2))], axis=-1)
    yy, xx = np.mgrid[0:H, 0:W]
    field = rng.normal(0, 1, (1, H, W, 6)).astype(np.float32)
    field[0, :, :, 1:3] = (kp2d[0, 0] - np.stack([yy + 0.5, xx + 0.5], axis=-1)).astype(np.float32)
    _rendered[H, W] = VC.frozen(dict(planes=planes.reshape(3, H, W), records=records.reshape(3, 11), inst_counts=p["inst_counts"], imax=3, labels=labels,
                                     field=field, dir_off=1, kp=2, kp2d=kp2d, jobs=np.array([(0, 0, 1, 0), (0, 1, 2, 0), (0, 2, 3, 0)], np.int32),
                                     sample_offset=0.5, cos_min=0.99))
    return _rendered[H, W]


_rendered = {}


@pytest.mark.parametrize("size", [(48, 64), (37, 50)])
def test_twin_equals_reference_on_rendered_planes(size):
    case = rendered_case(*size)
    got, want = run(case), reference(case)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:6].tolist()
    # the truth against its own render: every visible pixel lies on its label, the occluder hides a part of the block, and every direction of
    # keypoint 0 points at it
    assert not got[:, VR.ON_BACKGROUND].any() and not got[:, VR.ON_OTHER].any() and (got[:, VR.ON_LABEL] == got[:, VR.LABEL_PIXELS]).all()
    assert got[0, VR.HIDDEN] > 0 and got[1, VR.HIDDEN] == 0 and (got[:, VR.RENDERED] - got[:, VR.HIDDEN] == got[:, VR.ON_LABEL]).all()
    assert got[0, VR.INLIERS] >= got[0, VR.ON_LABEL] - 1 and got[0, VR.INLIERS] < got[0, VR.PAIRS] == 2 * got[0, VR.ON_LABEL]
