"""The device scene renderer's arithmetic on the CPU: `cp_render_scenes_host_f32` (the host twin of `cp_render_scenes_f32`: the same
csrc/scene_math.h, serially) against `SyntheticSceneDataset._render` for the same `default_rng([seed, i])` draws.  No kernel is launched here.

Bounds, none of them taken from the code under test:
  labels   at most 4 pixels of an image may differ from the host's map, and each of them must be a silhouette pixel of the host's map (an
           8-neighbour with another label): both sides decide disc > 0 and s < depth in fp64, and only a pixel whose decision lies within a few
           ulps of the boundary can fall the other way (the host's `rays @ R` is a BLAS product whose summation order and FMA use are its own).
  image    where the labels agree, |twin - host| <= 2.4e-7 on the noise-free image: both are fp64 values in [-1, 1] rounded once to fp32, one fp32
           ulp there is 1.2e-7, and 2 ulps allow for a last-bit difference of sqrt / sin / cos.
  counts   equal to the twin's own label map exactly, and to the host's within the number of differing pixels.
  noise    (noisy - noise-free) away from the clip: standard deviation 2 x 0.01 = 0.0200 on foreground and 2 x sqrt(0.02^2 + 0.01^2) = 0.04472 on
           background, each within 3 % (the estimator's own error at >= 10^4 pixels x 3 channels is below 0.5 %); |mean| <= 4 sigma / sqrt(N);
           correlations between channels and between two images of a batch below 4 / sqrt(N).

Every comparison first asserts that the compared images contain hit, miss and occlusion pixels.

The scenes, records and references of this module are shared with tests/test_gpu_scenes.py."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from casapose_amd.data_handler.device_scenes import DeviceScenes
from casapose_amd.data_handler.synthetic_scene import CAMERA, SyntheticSceneDataset

SEED, B = 0, 3
# (H, W, objects, images compared with the host's _render).  40 x 72: a width that is no multiple of 64, 2880 pixels = 2 full blocks and a part
# of one.  The host renders a 480 x 640 image in 0.7 s, so one of them is compared.
SHAPES = ((40, 72, 3, B), (64, 64, 3, B), (96, 128, 8, B), (480, 640, 13, 1))
IMG_TOL = 2.4e-7
MAX_LABEL_DIFFS = 4

# records [B, words]; twin / twin_noisy: cp_render_scenes_host_f32's outputs without / with noise; host: _render(noise=False) of the first
# `compared` images; hits [compared, oc, H, W]: the rays of the host's formula that meet object o in front of the camera
Scene = namedtuple("Scene", "ds scenes records twin twin_noisy host hits")


def host_hits(ds, hc, wc, poses):
    """[oc, H, W] bool: SyntheticSceneDataset._pixels' `hit & (s > 0)` per object, without the depth test."""
    H, W = ds.size
    ys, xs = np.mgrid[hc:hc + H, wc:wc + W].astype(np.float64) + 0.5
    rays = np.stack([(xs - CAMERA[0, 2]) / CAMERA[0, 0], (ys - CAMERA[1, 2]) / CAMERA[1, 1], np.ones_like(xs)], axis=-1)
    out = np.zeros((ds.oc, H, W), bool)
    for o in range(ds.oc):
        R, t = poses[o, :, :3], poses[o, :, 3]
        inv = 1.0 / ds.axes[o]
        d = (rays @ R) * inv
        c = (-(R.T @ t)) * inv
        a, bq = (d * d).sum(-1), (d * c).sum(-1)
        disc = bq * bq - a * (c @ c - 1.0)
        hit = disc > 0
        s = np.where(hit, (-bq - np.sqrt(np.where(hit, disc, 0.0))) / a, np.inf)
        out[o] = hit & (s > 0)
    return out


@functools.lru_cache(maxsize=None)
def scene(H, W, oc, compared=B) -> Scene:
    ds = SyntheticSceneDataset(oc, (H, W), seed=SEED)
    scenes = DeviceScenes(ds, "cuda:0")   # the host half and the twin touch no GPU
    records = scenes.host_half(range(B))["records"].numpy()
    host, hits = [], []
    for i in range(compared):
        host.append(ds._render(np.random.default_rng([SEED, i]), noise=False))
        hc, wc, poses = ds._draw(np.random.default_rng([SEED, i]))
        hits.append(host_hits(ds, hc, wc, poses))
    return Scene(ds, scenes, records, scenes.twin(records, noise=False), scenes.twin(records, noise=True), host, np.stack(hits))


def silhouette(label):
    """bool [H, W]: pixels with an 8-neighbour of another label"""
    H, W = label.shape
    padded = np.pad(label, 1, mode="edge")
    out = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= padded[dy:dy + H, dx:dx + W] != label
    return out


def assert_meaningful(s: Scene):
    """the compared images contain hit, miss and occlusion pixels"""
    labels = np.stack([h["label"] for h in s.host])
    occluded = s.hits.sum(axis=1) >= 2
    assert (labels > 0).sum() >= 100 and (labels == 0).sum() >= 100 and occluded.sum() >= 20, ((labels > 0).sum(), (labels == 0).sum(), occluded.sum())


def noise_statistics(noisy, clean, label):
    """(noisy - clean) of a batch [b, H, W, 3] away from the clip -> dict of the figures the noise bounds are about."""
    d = noisy.astype(np.float64) - clean.astype(np.float64)
    inside = (np.abs(clean) <= 0.88).all(axis=-1)          # 6 sigma of the foreground noise away from -1 and 1; the background lies in [-0.5, -0.1]
    fg, bg = inside & (label > 0), inside & (label == 0)
    out = dict(n_fg=int(fg.sum()), n_bg=int(bg.sum()))
    for name, mask in (("fg", fg), ("bg", bg)):
        v = d[mask]                                         # [n, 3]
        out["std_" + name], out["mean_" + name] = float(v.std()), float(v.mean())
        out["corr_channels_" + name] = max(abs(float(np.corrcoef(v[:, a], v[:, b])[0, 1])) for a, b in ((0, 1), (0, 2), (1, 2)))
    both = fg[0] & fg[1] | bg[0] & bg[1]                    # the same pixel of two images of the batch, with the same variance in both
    out["n_images"] = int(both.sum())
    out["corr_images"] = max(abs(float(np.corrcoef(d[0][both][:, c], d[1][both][:, c])[0, 1])) for c in range(3))
    return out


def assert_noise(st):
    print("noise statistics:", st)
    assert st["n_fg"] >= 10_000 and st["n_bg"] >= 10_000
    for name, sigma in (("fg", 0.02), ("bg", 2.0 * (0.02 ** 2 + 0.01 ** 2) ** 0.5)):
        n = st["n_" + name]
        assert abs(st["std_" + name] / sigma - 1.0) <= 0.03, (name, st["std_" + name])
        assert abs(st["mean_" + name]) <= 4.0 * sigma / (3 * n) ** 0.5, (name, st["mean_" + name])
        assert st["corr_channels_" + name] <= 4.0 / n ** 0.5, (name, st["corr_channels_" + name])
    assert st["corr_images"] <= 4.0 / st["n_images"] ** 0.5, st["corr_images"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_twin_matches_the_host_renderer(shape):
    s = scene(*shape)
    assert_meaningful(s)
    H, W, oc, compared = shape
    for i in range(compared):
        ref, lab = s.host[i], s.twin["label"][i]
        differ = lab != ref["label"]
        print("%dx%d image %d: %d label differences" % (H, W, i, differ.sum()))
        assert differ.sum() <= MAX_LABEL_DIFFS
        assert silhouette(ref["label"])[differ].all()
        err = np.abs(s.twin["img"][i].astype(np.float64) - ref["img"].astype(np.float64))[~differ]
        print("%dx%d image %d: noise-free image max |twin - host| = %.3g" % (H, W, i, err.max()))
        assert err.max() <= IMG_TOL
        own = np.array([(lab == o + 1).sum() for o in range(oc)])
        assert np.array_equal(s.twin["counts"][i], own)
        assert np.abs(s.twin["counts"][i].astype(np.int64) - ref["counts"]).sum() <= 2 * differ.sum()
        assert np.abs(s.twin["counts"][i].astype(np.int64) - ref["counts"]).max() <= differ.sum()
        assert np.array_equal(s.twin["target_seg"][i], np.eye(oc + 1, dtype=np.float32)[lab])
        assert np.array_equal(s.twin_noisy["label"][i], lab) and np.array_equal(s.twin_noisy["counts"][i], s.twin["counts"][i])


def test_small_arrays_of_the_host_half_are_the_host_paths():
    s = scene(64, 64, 3)
    want = s.ds.batch(1, 4)
    for shard, rows in (((0, 1), slice(0, 4)), ((1, 2), slice(2, 4))):
        from casapose_amd.parallel import shard_range

        begin, end = shard_range(4, *shard)
        got = s.scenes.host_half(range(4 + begin, 4 + end))["small"]
        assert sorted(got) == ["cam_mat", "diameters", "keypoints3d", "offsets", "poses_gt", "target_vert"]
        for k, v in got.items():
            assert v.dtype == want[k].dtype and np.array_equal(v.numpy(), want[k][rows].numpy()), k


def test_record_carries_the_host_draws_and_a_seed_drawn_after_them():
    s = scene(64, 64, 3)
    rec, small = s.scenes.record(5)
    rng = np.random.default_rng([SEED, 5])
    hc, wc, poses = s.ds._draw(rng)
    assert np.array_equal(small["poses"], poses) and rec[0] == hc and rec[1] == wc and rec[7] == 3
    assert int(rec[6:7].view(np.uint64)[0]) == int(rng.integers(0, 1 << 63, dtype=np.int64))
    assert np.array_equal(rec[8:17].reshape(3, 3), poses[0, :, :3]) and np.array_equal(rec[17:20], poses[0, :, 3])
    assert np.array_equal(rec[20:23], 1.0 / s.ds.axes[0]) and np.array_equal(rec[23:26], s.ds.colors[0])
    assert s.scenes.lib.cp_render_scenes_record_words(3) == rec.size


def test_render_keeps_its_draws_and_the_noise_switch_only_removes_the_noise():
    """_render(rng) consumes the generator as before (crop, poses, the two noise fields) and noise=False changes nothing but the noise"""
    ds = scene(64, 64, 3).ds
    a, b = np.random.default_rng([SEED, 2]), np.random.default_rng([SEED, 2])
    noisy = ds._render(a)
    hc, wc, poses = ds._draw(b)
    first, second = b.normal(0, 0.02, (64, 64, 3)), b.normal(0, 0.01, (64, 64, 3))
    assert a.random() == b.random()   # both generators stand at the same place
    clean = ds._render(np.random.default_rng([SEED, 2]), noise=False)
    assert np.array_equal(clean["label"], noisy["label"]) and np.array_equal(clean["poses"], poses) and np.array_equal(clean["kp2"], noisy["kp2"])
    v = (clean["img"].astype(np.float64) + 1.0) / 2.0
    want = np.clip(v + np.where(clean["label"][..., None] > 0, 0.0, first) + second, 0, 1) * 2.0 - 1.0
    assert np.abs(want - noisy["img"]).max() <= 2.4e-7


def test_generate_dataset_without_a_device_follows_the_variable(monkeypatch, capsys):
    """unset: the host path and no line; set without a GPU: an error, never the host path in silence"""
    import torch

    from casapose_amd.data_handler import device_scenes

    ds = scene(64, 64, 3).ds
    monkeypatch.delenv("CASAPOSE_DEVICE_SCENES", raising=False)
    assert device_scenes.device_from_environment() is None
    first = next(ds.generate_dataset(2, 1, 0)[0])
    assert first["img"].device.type == "cpu" and not ds._device_scenes and capsys.readouterr().out == ""
    monkeypatch.setenv("CASAPOSE_DEVICE_SCENES", "1")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="CASAPOSE_DEVICE_SCENES"):
        ds.generate_dataset(2, 1, 0)


def test_twin_noise_statistics():
    s = scene(96, 128, 8)
    big = s.scenes.host_half(range(6))["records"].numpy()   # 6 x 12288 pixels
    clean, noisy = s.scenes.twin(big, noise=False), s.scenes.twin(big, noise=True)
    assert_noise(noise_statistics(noisy["img"], clean["img"], clean["label"]))


def test_twin_image_does_not_depend_on_its_batch():
    s = scene(40, 72, 3)
    alone = s.scenes.twin(s.records[2:3], noise=True)
    for k in ("img", "label", "target_seg", "counts"):
        assert np.array_equal(alone[k][0], s.twin_noisy[k][2]), k


def test_arguments_are_checked_without_a_gpu():
    s = scene(40, 72, 3)
    lib, rec = s.scenes.lib, s.records
    img, lab, seg, cnt = (np.zeros(16, t) for t in (np.float32, np.uint8, np.float32, np.int32))
    p = lambda a: a.ctypes.data  # noqa: E731
    for fn, tail in ((lib.cp_render_scenes_host_f32, ()), (lib.cp_render_scenes_f32, (None,))):
        assert fn(None, 1, 3, 2, 2, 0, p(img), p(lab), p(seg), p(cnt), *tail) == -1 and b"null pointer" in lib.cp_last_error()
        for oc in (0, 255):
            assert fn(p(rec), 1, oc, 2, 2, 0, p(img), p(lab), p(seg), p(cnt), *tail) == -1 and b"oc must lie" in lib.cp_last_error()
        assert fn(p(rec), 0, 3, 2, 2, 0, p(img), p(lab), p(seg), p(cnt), *tail) == -1 and b"b must lie" in lib.cp_last_error()
        assert fn(p(rec), 1, 3, 0, 2, 0, p(img), p(lab), p(seg), p(cnt), *tail) == -1 and b"positive" in lib.cp_last_error()
        assert fn(p(rec), 1, 3, 65536, 32768, 0, p(img), p(lab), p(seg), p(cnt), *tail) == -1 and b"2^31" in lib.cp_last_error()
    assert lib.cp_render_scenes_record_words(0) == 0 and lib.cp_render_scenes_record_words(255) == 0 and lib.cp_render_scenes_record_words(13) == 8 + 18 * 13
