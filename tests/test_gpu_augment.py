"""GPU tests of the input pipeline (csrc/augment.hip, data_handler/device_pipeline.py): single ops against tests/aug_reference.py, the
Philox ops' determinism and statistics, geometry against PIL, whole batches against the host path, and the training script on the device
path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_reference as R  # noqa: E402

from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset  # noqa: E402
from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset, write_ndds_scene  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["obj_000001", "obj_000005", "obj_000006"]
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    root = tmp_path_factory.mktemp("ndds_gpu_aug")
    scene = SyntheticSceneDataset(len(NAMES), (480, 640), length=8, seed=21)
    write_ndds_scene(str(root / "data"), str(root / "models"), scene, 8, NAMES)
    return str(root / "data"), str(root / "models")


def programs(op_lists, seed=1):
    from casapose_amd import _lib
    from casapose_amd.data_handler import augment

    arr = (_lib.AugImage * len(op_lists))()
    for b, ops in enumerate(op_lists):
        arr[b].seed = seed + b
        augment.pack_image(arr[b], ops)
    raw = np.frombuffer(bytes(arr), np.uint8).copy()
    return torch.from_numpy(raw).to(DEV)


def photometric(imgs, op_lists, tile=0, seed=1):
    from casapose_amd import _lib

    lib = _lib.load()
    x = torch.from_numpy(np.ascontiguousarray(imgs)).to(DEV)
    out = torch.empty_like(x)
    progs = programs(op_lists, seed)
    _lib.check(lib.cp_aug_photometric(x.data_ptr(), progs.data_ptr(), x.shape[0], x.shape[1], x.shape[2], tile, out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def crops(n=2, h=45, w=61, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, h // 5 + 1, w // 5 + 1, 3)).astype(np.float64)
    smooth = np.repeat(np.repeat(base, 5, 1), 5, 2)[:, :h, :w]
    return np.clip(smooth + rng.normal(0, 20, smooth.shape), 0, 255).astype(np.uint8)


def test_pointwise_lut_ops_exact_and_hue_saturation():
    from casapose_amd import _lib
    from casapose_amd.data_handler import augment as A

    imgs = crops()
    luts = [A._three(A.lut_add([-7, 3, 9])), A._three(A.lut_multiply([1.2])), A._three(A.lut_gamma([0.8, 1.1, 1.2])),
            A._three(A.lut_sigmoid([7.0], [0.4])), A._three(A.lut_log([0.9])), A._three(A.lut_linear([1.25, 0.8, 1.0]))]
    for lut in luts:
        got = photometric(imgs, [[A.Op(_lib.AUG_LUT, "lut", lut=lut)]] * 2)
        assert (got == np.stack([R.apply_lut(im, lut) for im in imgs])).all()
    for dh, ds in ((10, 12), (-8, -15), (0, 5)):
        got = photometric(imgs, [[A.Op(_lib.AUG_HUE_SAT, "hs", i0=dh, i1=ds)]] * 2).astype(int)
        ref = np.stack([R.hue_saturation(im, dh, ds) for im in imgs]).astype(int)
        assert np.abs(got - ref).max() <= 1 and (got != ref).mean() < 0.01


def test_blurs_against_scipy():
    from casapose_amd import _lib
    from casapose_amd.data_handler import augment as A

    imgs = crops(h=40, w=52)
    linear = [A.gaussian_taps(1.3), A.gaussian_taps(0.4), np.full((4, 4), 1 / 16.0, np.float32), np.full((7, 7), 1 / 49.0, np.float32),
              A.motion_taps(5, 33.0, 0.4)]
    for t in linear:
        got = photometric(imgs, [[A.Op(_lib.AUG_BLUR_LINEAR, "blur", k=len(t), taps=t)]] * 2).astype(int)
        ref = np.stack([R.linear_blur(im, t) for im in imgs]).astype(int)
        assert np.abs(got - ref).max() <= 1, len(t)
    for k in (3, 5, 7):
        got = photometric(imgs, [[A.Op(_lib.AUG_BLUR_MEDIAN, "median", k=k)]] * 2)
        assert (got == np.stack([R.median_blur(im, k) for im in imgs])).all(), k
    got = photometric(imgs, [[A.Op(_lib.AUG_BLUR_BILATERAL, "bilateral", k=3, f0=40.0, f1=20.0)]] * 2).astype(int)
    ref = np.stack([R.bilateral(im, 3, 40.0, 20.0) for im in imgs]).astype(int)
    assert np.abs(got - ref).max() <= 1
    # two blurs in a row: the second sees the first's output with its own border
    t = A.gaussian_taps(1.0)
    got = photometric(imgs, [[A.Op(_lib.AUG_BLUR_LINEAR, "g", k=len(t), taps=t), A.Op(_lib.AUG_BLUR_MEDIAN, "m", k=5)]] * 2).astype(int)
    ref = np.stack([R.median_blur(R.linear_blur(im, t), 5) for im in imgs]).astype(int)
    assert np.abs(got - ref).max() <= 1 and (got != ref).mean() < 0.02


def test_random_ops_reproducible_across_tiles_and_halo():
    """Noise before two blurs: every halo pixel must be recomputed exactly as its owner computes it, so the 32x32 and 16x8 tilings agree
    bit for bit, and two runs agree."""
    from casapose_amd import _lib
    from casapose_amd.data_handler import augment as A

    imgs = crops(n=3, h=70, w=90, seed=4)
    t = A.gaussian_taps(1.5)
    ops = [A.Op(_lib.AUG_POISSON_NOISE, "poisson", per_channel=1, f0=6.0), A.Op(_lib.AUG_REPLACE, "sp", i0=0, f0=0.05),
           A.Op(_lib.AUG_BLUR_LINEAR, "g", k=len(t), taps=t), A.Op(_lib.AUG_BLUR_BILATERAL, "b", k=3, f0=60.0, f1=30.0),
           A.Op(_lib.AUG_DROPOUT, "drop", per_channel=0, f0=0.03)]
    a = photometric(imgs, [ops] * 3, tile=0)
    b = photometric(imgs, [ops] * 3, tile=0)
    c = photometric(imgs, [ops] * 3, tile=1)
    assert (a == b).all() and (a == c).all()
    # the pre-blur ops alone, then the blurs on the host restatement: same result within the blurs' rounding
    pre = photometric(imgs, [ops[:2]] * 3, tile=1)
    ref = np.stack([R.bilateral(R.linear_blur(im, t), 3, 60.0, 30.0) for im in pre]).astype(int)
    # the dropout alone, at the same Philox slot (4: four identity tables in front of it)
    drop_ref = photometric(imgs, [[A.Op(_lib.AUG_LUT, "id", lut=A._three(np.arange(256, dtype=np.uint8)))] * 4 + ops[4:]] * 3)
    mask = (drop_ref == 0).all(-1)   # pixels the slot-4 dropout zeroes in the full program
    assert ((a == 0).all(-1) >= mask).all()
    assert np.abs(a.astype(int) - ref)[~mask].max() <= 2


def test_random_op_statistics():
    from casapose_amd import _lib
    from casapose_amd.data_handler import augment as A

    n, h, w = 2, 256, 256
    imgs = np.full((n, h, w, 3), 128, np.uint8)
    N = n * h * w * 3

    def check_rate(x, p, count):
        assert abs(x - p) < 3 * np.sqrt(p * (1 - p) / count) + 1e-9, (x, p)

    got = photometric(imgs, [[A.Op(_lib.AUG_DROPOUT, "d", per_channel=1, f0=0.04)]] * n)
    check_rate((got == 0).mean(), 0.04, N)
    got = photometric(imgs, [[A.Op(_lib.AUG_DROPOUT, "d", per_channel=0, f0=0.04)]] * n)
    assert ((got == 0).all(-1) == (got == 0).any(-1)).all()
    check_rate((got[..., 0] == 0).mean(), 0.04, N // 3)
    lam = 5.0
    d = photometric(imgs, [[A.Op(_lib.AUG_POISSON_NOISE, "p", per_channel=1, f0=lam)]] * n).astype(np.float64) - 128
    assert abs(np.abs(d).mean() - lam) < 3 * np.sqrt(lam / N) and abs(d.mean()) < 3 * np.sqrt((lam + lam * lam) / N) and abs(d.var() - (lam + lam * lam)) < 0.1 * lam
    for mode, lo, hi in ((1, 128, 255), (2, 0, 128)):
        got = photometric(imgs, [[A.Op(_lib.AUG_REPLACE, "s", per_channel=0, i0=mode, f0=0.05)]] * n)
        changed = (got != 128).any(-1)
        check_rate(changed.mean(), 0.05 * (1 - 1 / 255.0), N // 3)
        assert got.min() >= lo and got.max() <= hi
    sigma = 12.0   # the op's formula at a scale where it moves pixels (the sequence's 0.05 almost never does)
    d = photometric(imgs, [[A.Op(_lib.AUG_GAUSS_NOISE, "g", per_channel=1, f0=sigma)]] * n).astype(np.float64) - 128
    assert abs(d.std() - sigma) < 0.02 * sigma and abs(d.mean()) < 0.05
    d = photometric(imgs, [[A.Op(_lib.AUG_LAPLACE_NOISE, "l", per_channel=1, f0=sigma)]] * n).astype(np.float64) - 128
    assert abs(np.abs(d).mean() - sigma) < 0.03 * sigma
    d = photometric(imgs, [[A.Op(_lib.AUG_GAUSS_NOISE, "g", per_channel=0, f0=0.05)]] * n)
    assert (d == 128).mean() > 0.999


def test_geometry_against_pil(exported):
    from PIL import Image

    from casapose_amd import _lib

    data, _ = exported
    img = np.asarray(Image.open(os.path.join(data, "000000", "000002.png")).convert("RGB"))
    seg = np.asarray(Image.open(os.path.join(data, "000000", "000002.seg.png")).convert("L"))
    H, W = seg.shape
    ds = VectorfieldDataset(root=data, path_meshes=exported[1], color_input=True, objectsofinterest=NAMES, seed=1)
    ds.rng = np.random.default_rng(0)
    ds.random_translation, ds.random_rotation = (20.0, 20.0), 15.0
    geo = ds.draw_geometry(W, H, (448, 448), 0.933333333)
    assert geo["angle"] != 0
    aff = geo["affine"]
    ref_img = np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, data=tuple(aff), resample=Image.BILINEAR))
    ref_seg = np.asarray(Image.fromarray(seg).transform((W, H), Image.AFFINE, data=tuple(aff), resample=Image.NEAREST))
    ch, cw, x0, y0 = geo["out_h"], geo["out_w"], geo["w_crop"], geo["h_crop"]
    ref_img, ref_seg = ref_img[y0:y0 + ch, x0:x0 + cw], ref_seg[y0:y0 + ch, x0:x0 + cw]
    p = _lib.AugImage()
    p.src_h, p.src_w, p.crop_x, p.crop_y, p.warp = H, W, x0, y0, 1
    for k in range(6):
        p.affine[k] = float(aff[k])
    for v in range(256):
        p.label_map[v] = v
    lib = _lib.load()
    progs = torch.from_numpy(np.frombuffer(bytes(p), np.uint8).copy()).to(DEV)
    src = torch.from_numpy(img.copy()).to(DEV)
    sg = torch.from_numpy(seg.copy()).to(DEV)
    out = torch.empty((1, ch, cw, 3), dtype=torch.uint8, device=DEV)
    lab = torch.empty((1, ch, cw), dtype=torch.uint8, device=DEV)
    _lib.check(lib.cp_aug_geometry(src.data_ptr(), sg.data_ptr(), progs.data_ptr(), 1, ch, cw, out.data_ptr(), lab.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.abs(out.cpu().numpy()[0].astype(int) - ref_img).max() <= 1
    # labels: the kernel follows PIL's 16.16 fixed-point nearest path, so they agree everywhere, ties included
    assert (lab.cpu().numpy()[0] == ref_seg).all()


def test_resize_against_pil():
    from PIL import Image

    from casapose_amd import _lib

    rng = np.random.default_rng(3)
    lib = _lib.load()
    for (ih, iw), (oh, ow) in (((60, 80), (45, 100)), ((50, 50), (120, 33))):
        img = rng.integers(0, 256, (2, ih, iw, 3), dtype=np.uint8)
        lab = rng.integers(0, 4, (2, ih, iw), dtype=np.uint8)
        x, lx = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
        o = torch.empty((2, oh, ow, 3), dtype=torch.uint8, device=DEV)
        ol = torch.empty((2, oh, ow), dtype=torch.uint8, device=DEV)
        _lib.check(lib.cp_aug_resize(x.data_ptr(), lx.data_ptr(), 2, ih, iw, oh, ow, o.data_ptr(), ol.data_ptr(), None))
        torch.cuda.synchronize()
        ref = np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), Image.BILINEAR)) for im in img])
        assert np.abs(o.cpu().numpy().astype(int) - ref).max() <= 1
        refl = np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), Image.NEAREST)) for im in lab])
        assert (ol.cpu().numpy() == refl).all()


def _ds(exported, **kw):
    data, models = exported
    args = dict(root=data, path_meshes=models, color_input=True, objectsofinterest=NAMES, seed=7, random_translation=(3.0, 3.0), random_rotation=10.0,
                noise=0, brightness=0.2, contrast=0.2)
    args.update(kw)
    return VectorfieldDataset(**args)


def _first(it):
    b = next(it)
    torch.cuda.synchronize()
    return b


def test_device_batch_matches_host_path(exported):
    for size, crop in (((448, 448), 0.933333333), ((224, 288), 0.8)):
        host = next(_ds(exported).generate_dataset(4, 1, imagesize=size, cropratio=crop, shard=(0, 1))[0])
        dev = _first(_ds(exported).generate_dataset(4, 1, imagesize=size, cropratio=crop, worker=2, prefetch=2, device=DEV)[0])
        assert set(host) == set(dev)
        for k in host:
            if k == "image_id":
                assert host[k] == dev[k]
                continue
            assert tuple(host[k].shape) == tuple(dev[k].shape) and host[k].dtype == dev[k].dtype, k
        for k in ("target_vert", "keypoints3d", "cam_mat", "diameters", "offsets", "cuboid3d", "poses_gt", "pixel_gt_count"):
            assert torch.equal(host[k], dev[k]), k
        assert dev["img"].is_cuda and dev["target_seg"].is_cuda
        assert (host["img"] - dev["img"].cpu()).abs().max().item() <= 1 / 127.5 + 1e-6
        assert torch.equal(host["target_seg"], dev["target_seg"].cpu()) and torch.equal(host["filtered_seg"], dev["filtered_seg"].cpu())


def test_device_batch_noise_sigma_recovered(exported):
    ds0, ds1 = _ds(exported, noise=0.3, brightness=0, contrast=0), _ds(exported, noise=0, brightness=0, contrast=0)
    a = _first(ds0.generate_dataset(4, 1, imagesize=(448, 448), cropratio=0.933333333, device=DEV)[0])["img"]
    b = _first(ds1.generate_dataset(4, 1, imagesize=(448, 448), cropratio=0.933333333, device=DEV)[0])["img"]
    # the sigma of each image is the host path's draw: uniform(0, noise) after the geometric draws
    ds2 = _ds(exported, noise=0.3, brightness=0, contrast=0)
    perm = np.random.default_rng([ds2.seed, 1]).permutation(8)[:4]
    for j, i in enumerate(perm):
        rng = np.random.default_rng([ds2.seed, 2, 0, int(i)])
        ds2.rng = rng
        ds2.draw_geometry(640, 480, (448, 448), 0.933333333)
        sigma = ds2.draw_photometric()[2]
        inside = (b[j].abs() < 0.9) & (a[j].abs() < 0.999)   # away from the clip
        d = (a[j] - b[j])[inside]
        assert abs(d.std().item() - sigma) < 0.03 * sigma + 2e-3, (d.std().item(), sigma)


def test_imgaug_batch_finite_different_and_shard_independent(exported):
    kw = dict(imagesize=(448, 448), cropratio=0.933333333)
    plain = _first(_ds(exported, noise=0.01).generate_dataset(4, 1, device=DEV, **kw)[0])
    full = _first(_ds(exported, noise=0.01, use_imgaug=True).generate_dataset(4, 1, device=DEV, **kw)[0])
    assert torch.isfinite(full["img"]).all() and full["img"].abs().max().item() <= 1
    assert (full["img"] - plain["img"]).abs().max().item() > 0.05
    assert torch.equal(full["target_seg"], plain["target_seg"])
    halves = [_first(_ds(exported, noise=0.01, use_imgaug=True).generate_dataset(4, 1, device=DEV, shard=(r, 2), **kw)[0]) for r in (0, 1)]
    for k in ("img", "target_seg", "filtered_seg"):
        assert torch.equal(torch.cat([h[k] for h in halves]), full[k]), k


def test_train_script_on_the_device_imgaug_path(exported, tmp_path, capsys):
    import train_casapose

    data, models = exported
    train_casapose.main(["-c", os.path.join(ROOT, "config", "config_8.ini"), "--data", data, "--datameshes", models, "--object", ",".join(NAMES),
                         "--datatest", "", "--imagesize", "128", "160", "--epochs", "1", "--batchsize", "4", "--outf", str(tmp_path / "out"),
                         "--pretrained", "0", "--loginterval", "1", "--saveinterval", "100"])
    out = capsys.readouterr().out
    assert "training input: device input pipeline (imgaug sequence on the device)" in out
    losses = [float(l.split("Loss: ")[1].split(",")[0]) for l in out.splitlines() if "Loss: " in l]
    assert losses and all(np.isfinite(losses))
