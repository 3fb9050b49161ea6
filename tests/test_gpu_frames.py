"""The inference-frame path on the GPU: cp_frames_to_input_f32 (csrc/frames.hip) bit for bit against NumPy's float32 formula of the
reference's load_images, the ImageOnlyDataset iterator, and util_scripts/test_minimal.py end to end against the same chain called directly."""
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "config_8.ini")
NAMES = "obj_000001,obj_000005,obj_000006,obj_000008,obj_000009,obj_000010,obj_000011,obj_000012".split(",")


def reference_input(frames_u8, n0=0.5, n1=0.5):
    """((img / 255) - normal[0]) / normal[1] in float32 (image_only_dataset.py:45), channels expanded as :40-43 do"""
    x = frames_u8[..., :3] if frames_u8.shape[-1] == 4 else np.repeat(frames_u8, 3, axis=-1) if frames_u8.shape[-1] == 1 else frames_u8
    return (x.astype(np.float32) / np.float32(255) - np.float32(n0)) / np.float32(n1)


def run_kernel(lib, src_bytes, batch, h, w, c, pitch, stride, n0, n1, device, out_offset=0):
    from casapose_amd import _lib

    src = torch.from_numpy(src_bytes).to(device)
    out = torch.full((batch * h * w * 3 + out_offset,), float("nan"), dtype=torch.float32, device=device)
    _lib.check(lib.cp_frames_to_input_f32(src.data_ptr(), batch, h, w, c, pitch, stride, n0, n1, out.data_ptr() + 4 * out_offset,
                                          torch.cuda.current_stream(device).cuda_stream), "cp_frames_to_input_f32")
    torch.cuda.synchronize(device)
    return out[out_offset:].cpu().numpy().reshape(batch, h, w, 3)


# (batch, h, w, extra row bytes, extra image bytes, normal, output offset in floats): dense and padded layouts on the float4 path, odd sizes,
# unaligned pitches and an unaligned output on the scalar path
LAYOUTS = [(3, 37, 53, 0, 0, (0.5, 0.5), 0), (2, 48, 64, 0, 0, (0.5, 0.5), 0), (3, 37, 53, 7, 11, (0.485, 0.229), 0),
           (2, 16, 64, 16, 32, (0.5, 0.5), 0), (1, 9, 12, 4, 0, (0.3, 0.7), 0), (2, 24, 40, 0, 0, (0.5, 0.5), 1), (1, 1, 1, 0, 0, (0.0, 1.0), 0)]


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%dx%dx%d_pad%d_%d_n%g_%g_off%d" % (l[0], l[1], l[2], l[3], l[4], l[5][0], l[5][1], l[6]))
def test_kernel_is_bit_identical_to_numpy(hip_lib, device, channels, layout):
    batch, h, w, pad_row, pad_img, (n0, n1), out_off = layout
    pitch = w * channels + pad_row
    stride = h * pitch + pad_img
    rng = np.random.default_rng([channels, batch, h, w, pad_row])
    raw = rng.integers(0, 256, batch * stride, dtype=np.uint8)
    if raw.size >= 256:
        raw[:256] = np.arange(256)                              # every byte value at least once
    frames = np.stack([np.lib.stride_tricks.as_strided(raw[b * stride:], (h, w, channels), (pitch, channels, 1)) for b in range(batch)])
    got = run_kernel(hip_lib, raw, batch, h, w, channels, pitch, stride, n0, n1, device, out_off)
    want = reference_input(frames, n0, n1)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


def test_kernel_refuses_invalid_arguments(hip_lib, device):
    src = torch.zeros(4096, dtype=torch.uint8, device=device)
    out = torch.zeros(4096, dtype=torch.float32, device=device)
    s, o = src.data_ptr(), out.data_ptr()
    ok = (s, 2, 4, 5, 3, 15, 60, 0.5, 0.5, o, None)
    assert hip_lib.cp_frames_to_input_f32(*ok) == 0
    torch.cuda.synchronize(device)
    for k, v in [(4, 2), (4, 5), (4, 0), (1, 0), (2, 0), (3, -2), (5, 14), (6, 59), (0, None), (9, None)]:
        args = list(ok)
        args[k] = v
        assert hip_lib.cp_frames_to_input_f32(*args) == -1, (k, v)
        assert b"cp_frames_to_input_f32" in hip_lib.cp_last_error()


def test_dataset_iterator_equals_the_kernel_on_the_decoded_files(hip_lib, device, tmp_path):
    from casapose_amd.data_handler.image_only_dataset import ImageOnlyDataset

    rng = np.random.default_rng(3)
    for k, (mode, shape) in enumerate([("RGB", (37, 53, 3)), ("L", (37, 53)), ("RGBA", (37, 53, 4))]):
        d = tmp_path / mode
        d.mkdir()
        imgs = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(5)]
        for i, a in enumerate(imgs):
            Image.fromarray(a, mode).save(str(d / ("%06d.png" % i)))
        Image.fromarray(imgs[0], mode).save(str(d / "000000.seg.png"))
        normal = [0.5, 0.5] if k != 1 else [0.25, 0.75]
        ds = ImageOnlyDataset(str(d), normal=normal)
        it, n = ds.generate_dataset(2, device=device)
        assert n == 2.0
        batches = list(it)
        assert len(batches) == 2
        c = 1 if mode == "L" else len(mode)
        for b, got in enumerate(batches):
            assert got.device.type == "cuda" and got.dtype == torch.float32 and tuple(got.shape) == (2, 37, 53, 3)
            frames = np.stack([np.asarray(Image.open(str(d / ("%06d.png" % (2 * b + j))))).reshape(37, 53, c) for j in range(2)])
            direct = run_kernel(hip_lib, frames.reshape(-1).copy(), 2, 37, 53, c, 53 * c, 37 * 53 * c, normal[0], normal[1], device)
            g = got.cpu().numpy()
            assert g.tobytes() == direct.tobytes()
            assert g.view(np.uint32).tobytes() == reference_input(frames, *normal).view(np.uint32).tobytes()


def test_test_minimal_end_to_end_matches_the_direct_chain(device, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "util_scripts"))
    import test_minimal

    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset, write_ndds_scene
    from casapose_amd.pose_estimation.pose_evaluation import poses_pnp
    from casapose_amd.pose_estimation.voting_layers_2d import CoordLSVotingWeighted
    from casapose_amd.pose_models.tfkeras import Classifiers

    data, models, out = str(tmp_path / "data"), str(tmp_path / "models"), str(tmp_path / "run")
    write_ndds_scene(data, models, SyntheticSceneDataset(8, (480, 640), length=12, seed=5), 12, NAMES)
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=9, input_shape=(480, 640, 3), weights=None, device=device, seed=21)
    os.makedirs(out + "/frozen_model")
    net.save_weights(out + "/frozen_model/result_w.h5")
    argv = ["-c", CFG, "--outf", out, "--manualseed", "7", "--datatest", data, "--datameshes", models, "--load_h5_weights", "1",
            "--object", ",".join(NAMES), "--write_poses", "1"]
    res = test_minimal.main(argv)
    printed = capsys.readouterr().out

    rows = list(csv.reader(open(out + "/speed_eval.csv")))
    assert open(out + "/speed_eval.csv").readline() == "batchid,speed \n"
    assert [int(r[0]) for r in rows[1:]] == list(range(1, 13))
    speeds = np.array([float(r[1]) for r in rows[1:]])
    assert np.all(np.isfinite(speeds)) and np.all(speeds > 0) and len(res["speed"]) == 12
    avg = re.search(r"^average speed: (\S+)$", printed, flags=re.M)
    assert avg and abs(float(avg.group(1)) - np.mean(res["speed"][10:])) < 1e-12
    assert os.path.exists(out + "/header_eval.txt") and os.path.isdir(out + "/control_output")
    est = list(csv.reader(open(out + "/poses_est.csv")))
    assert est[0] == ["name", "object"] + ["r%d%d" % (i, j) for i in range(1, 4) for j in range(1, 4)] + ["t1", "t2", "t3"]
    assert len(est) == 1 + 12 * 8 and est[1][:2] == ["000000", NAMES[0]]

    # the same chain called directly on inputs normalised by NumPy from the same PNGs, with the same seeded draws
    ref = VectorfieldDataset(root=data, path_meshes=models, no_points=9, objectsofinterest=NAMES, noise=0.00001, contrast=0.00001, brightness=0.00001,
                             random_translation=(0, 0), random_rotation=0, random_crop=False)
    first = next(ref.generate_dataset(1, 1, 0, (480, 640), 1.0, 1, 8, shuffle=False)[0])
    direct = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=9, input_shape=(480, 640, 3), weights=None, device=device, seed=3)
    direct.load_weights(out + "/frozen_model/result_w.h5")
    voter = CoordLSVotingWeighted(name="coords_ls_voting", num_classes=9, num_points=9, filter_estimates=True)
    rng = np.random.default_rng(7)
    found = 0
    assert sorted(res["poses"]) == ["%06d" % i for i in range(12)]
    for i in range(12):
        img = reference_input(np.asarray(Image.open(os.path.join(data, "000000", "%06d.png" % i)).convert("RGB")))[None]
        o = direct([img], training=False)
        seg, dirs, conf = torch.split(o, [9, 18, 9], dim=3)
        want = poses_pnp(voter([seg, dirs, conf]), seg, first["keypoints3d"], first["cam_mat"], 8, min_num=200, rng=rng)[0, :, 0]
        got = res["poses"]["%06d" % i]
        assert got.shape == (8, 3, 4)
        assert np.abs(got - want).max() <= 1e-5, "image %d" % i
        found += int(np.any(want != 0, axis=(1, 2)).sum())
        for o_ in range(8):
            row = est[1 + 8 * i + o_]
            assert row[:2] == ["%06d" % i, NAMES[o_]]
            assert np.allclose([float(v) for v in row[2:]], np.concatenate([got[o_, :, :3].reshape(-1), got[o_, :, 3]]), rtol=1e-7, atol=1e-7)
    assert found > 0, "no object was found in any frame: the comparison would be vacuous"


def test_test_minimal_refusals(device, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "util_scripts"))
    import test_minimal

    base = ["-c", CFG, "--outf", str(tmp_path / "run"), "--datatest", str(tmp_path)]
    with pytest.raises(SystemExit, match="estimate_confidence"):
        test_minimal.main(base + ["--estimate_confidence", "0"])
    with pytest.raises(SystemExit, match="pvnet"):
        test_minimal.main(base + ["--modelname", "pvnet", "--estimate_confidence", "0", "--estimate_coords", "0"])
