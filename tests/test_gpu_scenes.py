"""The device scene renderer on the GPU: `cp_render_scenes_f32` (csrc/scenes.hip) against its host twin on the records of
tests/test_scenes_twin_host.py, and `DeviceScenes` / `SyntheticSceneDataset.batch(..., device=)` / `generate_dataset(..., device=)` on top of it.

Kernel and twin run the same header (csrc/scene_math.h) on the same records, the geometry in fp64 without FMA contraction on both sides:
  label, target_seg, counts   equal.
  noise-free img              within 2.4e-7: fp64 values in [-1, 1] rounded once to fp32 (ulp 1.2e-7), 2 ulps for the last bit of the device's and
                              the host's sqrt / sin / cos.
  noisy img                   within 1e-6: the same Philox words, Box-Muller in fp32 on both sides; a normal is at most 5.8 and enters with
                              2 x 0.02, so a relative difference of a few fp32 ulps between the two logf / cosf / sinf stays below 1e-7.
Measured on the MI355X: label / target_seg / counts equal at every shape, noise-free img equal (0), noisy img within 5.96e-8 (half an fp32 ulp at 1).

Besides the shapes of the host test: 49 x 93 with 2 objects (a width that is no multiple of 4: the element-wise stores, five blocks, the last
one partial; b = 3 puts images at offsets that are no multiple of 4), and one call whose img holds more than 2^31 elements."""
import numpy as np
import pytest
import torch

import test_scenes_twin_host as T
from casapose_amd.data_handler.device_scenes import DeviceScenes
from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

pytestmark = pytest.mark.gpu

SHAPES = tuple(s[:3] for s in T.SHAPES) + ((49, 93, 2),)
NOISY_TOL = 1e-6


def on_device(s, device, records, noise):
    """cp_render_scenes_f32 on host records -> NumPy arrays like DeviceScenes.twin's"""
    scenes = DeviceScenes(s.ds, device)
    out, done = scenes.launch_records(torch.from_numpy(np.ascontiguousarray(records)), noise)
    done.synchronize()
    return {k: out[k].cpu().numpy() for k in ("img", "label", "target_seg", "counts")}, out["counts_host"].numpy().copy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kernel_matches_its_host_twin(device, shape):
    s = T.scene(*shape, *((1,) if shape[0] == 480 else ()))
    for noise, twin, tol in ((False, s.twin, T.IMG_TOL), (True, s.twin_noisy, NOISY_TOL)):
        got, counts_host = on_device(s, device, s.records, noise)
        again, _ = on_device(s, device, s.records, noise)
        for k in ("label", "target_seg", "counts"):
            assert np.array_equal(got[k], twin[k]), (k, noise)
        assert np.array_equal(counts_host, twin["counts"])
        err = np.abs(got["img"].astype(np.float64) - twin["img"].astype(np.float64)).max()
        print("%s noise %d: max |kernel - twin| = %.3g" % (shape, noise, err))
        assert err <= tol
        for k in got:   # two calls give identical bits
            assert np.array_equal(got[k], again[k]), k
    assert (s.twin["label"] > 0).sum() >= 100 and (s.twin["label"] == 0).sum() >= 100   # the batch has hit and miss pixels
    assert np.abs(s.twin_noisy["img"] - s.twin["img"]).max() > 0.01


def test_image_does_not_depend_on_how_it_is_rendered(device):
    """image 6 of the stream: alone, as member 2 of a batch of 4, and by shard (1, 2) of a global batch of 4"""
    ds = SyntheticSceneDataset(3, (40, 72), seed=5)
    alone = ds.batch(6, 1, device=device)
    four = ds.batch(1, 4, device=device)
    shard = ds.batch(1, 4, shard=(1, 2), device=device)
    assert shard["img"].shape[0] == 2
    for k in alone:
        a = alone[k].cpu().numpy()
        assert np.array_equal(a[0], four[k].cpu().numpy()[2]) and np.array_equal(a[0], shard[k].cpu().numpy()[0]), k
    assert np.abs(alone["img"].cpu().numpy()[0] - four["img"].cpu().numpy()[1]).max() > 0.1   # (another image is another picture)


def test_noise_statistics(device):
    s = T.scene(96, 128, 8)
    big = s.scenes.host_half(range(6))["records"].numpy()
    clean, _ = on_device(s, device, big, False)
    noisy, _ = on_device(s, device, big, True)
    assert np.array_equal(clean["label"], noisy["label"])
    T.assert_noise(T.noise_statistics(noisy["img"], clean["img"], clean["label"]))


def test_generate_dataset_on_the_device(device):
    oc, H, W, bs = 3, 64, 64, 2
    ds = SyntheticSceneDataset(oc, (H, W), length=8, seed=9)
    it, n = ds.generate_dataset(bs, device=device, prefetch=2)
    assert n == 4
    first = next(it)
    want = ds.batch(0, bs)
    assert list(first) == list(want)
    for k, v in want.items():
        assert first[k].shape == v.shape and first[k].dtype == v.dtype, k
        assert (first[k].device.type == "cuda") == (k in ("img", "target_seg", "filtered_seg")), k
        if k not in ("img", "target_seg", "filtered_seg", "pixel_gt_count"):
            assert np.array_equal(first[k].numpy(), v.numpy()), k
    kept = {k: first[k].cpu().numpy().copy() for k in first}
    second = next(it)
    torch.cuda.synchronize()
    for k in first:   # a batch taken earlier is unchanged after the next one has been requested
        assert np.array_equal(first[k].cpu().numpy(), kept[k]), k
    assert not np.array_equal(second["img"].cpu().numpy(), kept["img"])
    # the labels are the host's up to silhouette pixels, the counts are the labels', the image is the host's picture under other noise
    lab = kept["filtered_seg"][..., 0]
    differ = lab != want["filtered_seg"].numpy()[..., 0]
    assert differ.reshape(bs, -1).sum(axis=1).max() <= T.MAX_LABEL_DIFFS
    assert np.array_equal(kept["target_seg"], np.eye(oc + 1, dtype=np.float32)[lab])
    assert np.array_equal(kept["pixel_gt_count"][:, :, 0, 0], np.stack([[(l == o + 1).sum() for o in range(oc)] for l in lab]).astype(np.float32))
    assert np.abs(kept["img"] - want["img"].numpy())[~differ].max() <= 6.0 * (0.0447 + 0.0447)   # two noise samples of sigma <= 0.0447, 6 sigma each
    # the epochs + 1 passes of the host iterator, and nothing after them
    assert sum(1 for _ in it) == 2 * n - 2


def test_train_step_runs_on_a_device_batch(device):
    from types import SimpleNamespace

    from casapose_amd import training as TR
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler

    oc, H, W = 3, 64, 64
    ds = SyntheticSceneDataset(oc, (H, W), length=4, seed=9)
    it, _ = ds.generate_dataset(2, device=device, prefetch=2)
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=oc + 1, input_shape=(H, W, 3), input_segmentation_shape=(H, W, oc + 1), weights=None,
                                             base_model="resnet18", device=device, seed=3)
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=True, max_keypoint_pixel_error=12.5, confidence_regularization=True,
                          use_bpnp_reprojection_loss=False)
    lf, optim = LossWeightHandler(1.0, 0.5, 0.015, 0.007, filter_vertex_with_segmentation=True), TR.Adam(learning_rate=1e-3)
    for _ in range(2):
        losses = TR.train_step(net, next(it), lf, optim, opt)
        assert len(losses) == 5 and np.all(np.isfinite(losses)), losses


def test_without_a_device_the_batch_is_todays(monkeypatch):
    monkeypatch.delenv("CASAPOSE_DEVICE_SCENES", raising=False)
    ds = SyntheticSceneDataset(3, (40, 72), seed=5)
    got = ds.batch(2, 2)
    items = [ds._render(np.random.default_rng([5, 4 + i])) for i in range(2)]
    assert all(v.device.type == "cpu" for v in got.values()) and not ds._device_scenes
    assert np.array_equal(got["img"].numpy(), np.stack([it["img"] for it in items]))
    assert np.array_equal(got["filtered_seg"].numpy()[..., 0], np.stack([it["label"] for it in items]))
    assert np.array_equal(got["target_seg"].numpy(), np.eye(4, dtype=np.float32)[np.stack([it["label"] for it in items])])
    assert np.array_equal(got["poses_gt"].numpy()[:, :, 0], np.stack([it["poses"] for it in items]).astype(np.float32))
    assert np.array_equal(got["pixel_gt_count"].numpy()[:, :, 0, 0], np.stack([it["counts"] for it in items]).astype(np.float32))
    first = next(ds.generate_dataset(2, 1, 0)[0])
    assert np.array_equal(first["img"].numpy(), ds.batch(0, 2)["img"].numpy())


def test_scripts_take_the_device_path_when_the_variable_is_set(device, tmp_path, monkeypatch, capsys):
    """CASAPOSE_DEVICE_SCENES=1: train_casapose.py and test_casapose.py render their `synthetic` sources on the device, say so in one line and
    run to their reports; without the variable neither prints the line (tests/test_gpu_scripts.py runs that path to its reports)."""
    import csv
    import os

    import test_casapose
    import train_casapose

    out = str(tmp_path / "run")
    common = ["-c", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "config_8.ini"), "--outf", out, "--manualseed", "7",
              "--workers", "0"]
    monkeypatch.setenv("CASAPOSE_DEVICE_SCENES", "1")
    train_casapose.main(common + ["--data", "synthetic:4", "--datatest", "synthetic:2", "--epochs", "1", "--batchsize", "2", "--imagesize", "128", "160",
                                  "--saveinterval", "1", "--loginterval", "1", "--validationinterval", "1"])
    assert capsys.readouterr().out.count("input: synthetic scenes rendered on the device\n") == 1
    rows = list(csv.reader(open(out + "/loss_train.csv")))
    vals = np.array([[float(v) for v in r[2:7]] for r in rows[1:]])
    assert len(rows) == 3 and np.all(np.isfinite(vals))
    res = test_casapose.main(common + ["--datatest", "synthetic:2", "--load_h5_weights", "1", "--imagesize_test", "128", "160"])
    assert capsys.readouterr().out.count("input: synthetic scenes rendered on the device\n") == 1
    assert np.all(np.isfinite(res["loss"])) and res["valid_3d"].shape == (8,)
    monkeypatch.delenv("CASAPOSE_DEVICE_SCENES")
    test_casapose.main(common + ["--datatest", "synthetic:2", "--load_h5_weights", "1", "--imagesize_test", "128", "160"])
    assert "rendered on the device" not in capsys.readouterr().out


def test_offsets_past_2_to_the_31(device):
    """172 images of 2048 x 2048 with one object: img holds 2.16e9 floats, so the last image's elements lie past 2^31.  The last image is compared
    with the twin of its record; the first one too (a wrapped offset would have landed there)."""
    H = W = 2048
    b = 172
    assert b * H * W * 3 > 2 ** 31
    ds = SyntheticSceneDataset(1, (H, W), seed=2, random_crop=False)   # (larger than the 480 x 640 frame: the crop origin is negative)
    scenes = DeviceScenes(ds, device)
    one = scenes.host_half(range(2))["records"].numpy()
    records = np.concatenate([one[:1], np.repeat(one[1:2], b - 2, axis=0), one[:1]])
    records[-1, 6:7].view(np.uint64)[0] += 1   # the last image: image 0 under another seed
    out, done = scenes.launch_records(torch.from_numpy(records), True)
    done.synchronize()
    twin = scenes.twin(records[[0, -1]], True)
    for j, i in enumerate((0, b - 1)):
        assert np.array_equal(out["label"][i].cpu().numpy(), twin["label"][j])
        assert np.array_equal(out["target_seg"][i].cpu().numpy(), twin["target_seg"][j])
        assert np.abs(out["img"][i].cpu().numpy().astype(np.float64) - twin["img"][j]).max() <= NOISY_TOL
    counts = out["counts_host"].numpy()
    assert np.array_equal(counts[[0, -1]], twin["counts"]) and (counts[1:-1] == counts[1]).all() and counts[0, 0] > 0
