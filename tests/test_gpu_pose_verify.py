"""cp_pose_verify_i32 (csrc/pose_verify.hip) and DevicePoseVerifier on the GPU against the host twin, which tests/test_verify_twin_host.py holds
to the NumPy restatement on the CPU: the results are integers, so the gate is equality of bytes.  The cases are tests/verify_cases.py's (the
5 x 7 hand case; boxes of tile - 1, tile and tile + 1 pixels at a width that is no multiple of 64; the production record ld 36 / dir_off 9 /
kp 9 over three images with shuffled jobs, a plane named twice, an out-of-range job and label 255; the generic ld 20 / dir_off 3 / kp 1; a frame
of 256 planes at 8 x 8; a record no 16-byte load can take), each with a workspace full of garbage."""
import numpy as np
import pytest

import contour_cases as CC
import verify_cases as VC
import verify_reference as VR
import verify_scenes as VS
from test_verify_twin_host import host_counts, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(VC.CASES))
def test_device_equals_host_twin(device, name):
    got, want = run(VC.CASES[name](), device=device, fill=0xA5), host_counts(name)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (name, np.argwhere(got != want)[:6].tolist())
    if name == "hand":
        assert got.tolist() == [list(VC.HAND_A), list(VC.HAND_B)]


@pytest.mark.parametrize("name", ["tiles", "production", "256 planes"])
def test_split_changes_nothing(device, name):
    want = host_counts(name)
    for split, fill in ((1, 0x00), (3, 0xFF), (64, 0x5A)):
        got = run(VC.CASES[name](), device=device, split=split, fill=fill)
        assert got.tobytes() == want.tobytes(), (name, split, np.argwhere(got != want)[:6].tolist())


def test_refused_jobs_leave_zeros(device):
    case = VC.hand()
    big = 2 ** 31 - 1
    jobs = np.array([(0, 0, 1, 0), (1, 0, 1, 0), (-1, 0, 1, 0), (0, 2, 1, 0), (0, -1, 1, 0), (big, big, big, big), (0, 0, 0, 0), (0, 0, 256, 0), (0, 1, 2, 0)], np.int32)
    kp2d = np.concatenate([np.tile(case["kp2d"][:1], (len(jobs) - 1, 1, 1)), case["kp2d"][1:]])
    got = run(case, device=device, jobs=jobs, kp2d=kp2d)
    assert got.tobytes() == run(case, jobs=jobs, kp2d=kp2d).tobytes()
    assert got[0].tolist() == list(VC.HAND_A) and got[-1].tolist() == list(VC.HAND_B) and not got[1:-1].any()


def test_unaligned_field_takes_the_scalar_loads(device):
    """the production record from a field that starts 4 bytes past a 16-byte boundary: the same counts"""
    import torch

    from casapose_amd import _lib, twin

    case = VC.production()
    lib = _lib.load()
    nplanes, H, W = case["planes"].shape
    images, ld, n = len(case["labels"]), 36, len(case["jobs"])
    up = lambda a, t: twin.array(a, t, device)    # noqa: E731
    pad = torch.zeros(case["field"].size + 1, dtype=torch.float32, device=device)
    field = pad[1:]
    field.copy_(up(case["field"], np.float32).reshape(-1))
    assert field.data_ptr() % 16 == 4
    size = int(lib.cp_pose_verify_workspace_bytes(images))
    counts, work = up(np.full((n, 8), -7, np.int32), np.int32), up(np.full(size, 0xEE, np.uint8), np.uint8)
    twin.call("cp_pose_verify_i32", up(case["planes"], np.uint32), up(case["records"], np.int32), nplanes, H, W, up(case["inst_counts"], np.int32),
              len(case["inst_counts"]), case["imax"], up(case["labels"], np.uint8), field, images, ld, case["dir_off"], case["kp"], up(case["kp2d"], np.float64),
              up(case["jobs"], np.int32), n, case["sample_offset"], case["cos_min"], 2, counts, work, size, stream=torch.cuda.current_stream(device).cuda_stream)
    assert counts.cpu().numpy().tobytes() == host_counts("production").tobytes()


@pytest.mark.parametrize("size", VS.SIZES)
def test_verify_end_to_end_in_chunks(device, size):
    """DevicePoseVerifier.verify on the device and with host=True over each of the two block scenes (two images: the true poses, and the block
    shifted beside the other two), under a cap that forces two chunks: equal counts, and equal to the one-chunk run; the true poses outscore
    the shifted block"""
    import torch

    from casapose_amd import _lib
    from casapose_amd.pose_estimation.pose_verify import DevicePoseVerifier

    m = CC.meshes()
    v = DevicePoseVerifier([a for a, _ in m], [f for _, f in m], device, near=CC.NEAR, far=CC.FAR)
    H, W = size
    s, t = VS.scene(H, W), VS.scene(H, W)["truth"]
    labels, field = np.concatenate([s["labels"]] * 2), np.concatenate([s["field"]] * 2)
    poses = np.stack([p for _, _, p in t] + [VS.shifted(0, t[0][2]), t[1][2], t[2][2]])
    obj, lab, img = [o for o, _, _ in t] * 2, [l for _, l, _ in t] * 2, [0, 0, 0, 1, 1, 1]
    K, kps = CC.IC.VC.K_of(VS.CAM), VS.keypoints3d()
    d_labels, d_field = torch.from_numpy(labels).to(device), torch.from_numpy(field).to(device)
    host = v.verify(poses, K, obj, img, labels, lab, field, kps, VS.DIR_OFF, host=True)
    one = v.verify(poses, K, obj, img, d_labels, lab, d_field, kps, VS.DIR_OFF)
    assert v.last_chunks == 1 and v.last_renders == 6
    cap = int(_lib.load().cp_render_masks_workspace_bytes(1, 3, H, W))
    two = v.verify(poses, K, obj, img, d_labels, lab, d_field, kps, VS.DIR_OFF, workspace_cap=cap, split=5)
    assert v.last_chunks == 2
    assert one["counts"].tobytes() == host["counts"].tobytes() and two["counts"].tobytes() == host["counts"].tobytes()
    assert one["score"].tolist() == host["score"].tolist() and (one["score"][:3] > 0.95).all() and one["score"][3] < 0.3
    assert one["counts"][0, VR.HIDDEN] > 0
    with pytest.raises(ValueError, match="device tensors, or NumPy arrays with host=True"):
        v.verify(poses, K, obj, img, labels, lab, field, kps, VS.DIR_OFF)
