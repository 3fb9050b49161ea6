"""CPU checks of the inference-frame input (casapose_amd/data_handler/image_only_dataset.py, the reference's ImageOnlyDataset): folder
discovery, batching arithmetic, host decoding and its refusals, the `casapose.` alias, and the argument checks of cp_frames_to_input_f32
(refused before anything is launched, so no GPU is needed)."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image


def _png(path, arr, mode=None):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr, mode).save(path) if mode else Image.fromarray(arr).save(path)


def _rgb(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _png16_rgb(path, h, w):
    """a 16-bit RGB PNG written by hand (PIL cannot write one)"""
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)

    rows = b"".join(b"\x00" + (np.arange(w * 3, dtype=">u2") * 257).tobytes() for _ in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows))
                + chunk(b"IEND", b""))


def test_discovery_order_and_filters(tmp_path):
    from casapose_amd.data_handler.image_only_dataset import ImageOnlyDataset

    root = tmp_path / "frames"
    a, b = _rgb(4, 6, 0), _rgb(4, 6, 1)
    _png(str(root / "s2" / "000002.png"), a)
    _png(str(root / "s2" / "000001.png"), b)
    _png(str(root / "s2" / "000001.seg.png"), a[..., 0])        # masks end in ".seg.png": no digit before the extension
    _png(str(root / "s2" / "frame.png"), a)                     # no digit before the extension
    Image.fromarray(a).save(str(root / "s2" / "000003.jpg"))    # a PNG in the folder: JPGs are ignored
    os.makedirs(str(root / "s1" / "deep"))
    Image.fromarray(a).save(str(root / "s1" / "deep" / "7.jpg"))
    Image.fromarray(a).save(str(root / "s1" / "deep" / "10.jpg"))
    _png(str(root / "s1" / "99.png"), a)                        # s1 has a subfolder: its own files are not read
    _png(str(root / "5.png"), a)                                # so has the root
    ds = ImageOnlyDataset(str(root))
    rel = [os.path.relpath(p, str(root)) for p in ds.imgs]
    assert rel == [os.path.join("s1", "deep", "10.jpg"), os.path.join("s1", "deep", "7.jpg"), os.path.join("s2", "000001.png"),
                   os.path.join("s2", "000002.png")]
    assert len(ds) == 4
    assert ds[2] == {"path": str(root / "s2" / "000001.png"), "name": "000001"}
    assert [ds[i]["name"] for i in range(4)] == ["10", "7", "000001", "000002"]
    assert ds.normal == [0.5, 0.5]
    assert len(ImageOnlyDataset(str(tmp_path / "missing"))) == 0


def test_batches_drop_the_remainder_and_need_a_gpu(tmp_path, monkeypatch):
    import torch

    from casapose_amd import _lib
    from casapose_amd.data_handler.image_only_dataset import ImageOnlyDataset

    for i in range(7):
        _png(str(tmp_path / ("%06d.png" % i)), _rgb(3, 5, i))
    ds = ImageOnlyDataset(str(tmp_path))
    it, n = ds.generate_dataset(3)
    assert n == 2.0 and isinstance(n, float)                    # 7 frames, batches of 3: the last frame is dropped
    assert ds.generate_dataset(2)[1] == 3.0 and ds.generate_dataset(7)[1] == 1.0 and ds.generate_dataset(8)[1] == 0.0
    with pytest.raises(ValueError):
        ds.generate_dataset(0)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.CasaposeHipError, match="needs a ROCm GPU"):
        next(it)
    got = ds.load_frames([4, 1])
    assert got.dtype == np.uint8 and got.shape == (2, 3, 5, 3)
    assert np.array_equal(got[0], _rgb(3, 5, 4)) and np.array_equal(got[1], _rgb(3, 5, 1))


def test_a_frame_of_another_size_is_refused_by_name(tmp_path):
    from casapose_amd.data_handler.image_only_dataset import ImageOnlyDataset

    _png(str(tmp_path / "000000.png"), _rgb(4, 6, 0))
    _png(str(tmp_path / "000001.png"), _rgb(4, 6, 1))
    _png(str(tmp_path / "000002.png"), _rgb(5, 6, 2))
    _png(str(tmp_path / "000003.png"), _rgb(4, 6, 3)[..., 0])   # same size, one channel: also not the first frame's shape
    ds = ImageOnlyDataset(str(tmp_path))
    assert ds.frame_shape() == (4, 6, 3)
    assert ds.load_frames([0, 1]).shape == (2, 4, 6, 3)
    with pytest.raises(ValueError, match="000002.png"):
        ds.load_frames([0, 1, 2])
    with pytest.raises(ValueError, match="000003.png"):
        ds.load_frames([3])
    with pytest.raises(ValueError, match="no .* frames"):
        ImageOnlyDataset(str(tmp_path / "empty")).frame_shape()


def test_decoding_channel_counts(tmp_path):
    from casapose_amd.data_handler.image_only_dataset import decode_frame

    rgb = _rgb(3, 4, 5)
    grey = rgb[..., 1].copy()
    rgba = np.concatenate([rgb, grey[..., None]], -1)
    _png(str(tmp_path / "l.png"), grey)
    _png(str(tmp_path / "rgb.png"), rgb)
    _png(str(tmp_path / "rgba.png"), rgba, "RGBA")
    g = decode_frame(str(tmp_path / "l.png"))
    assert g.dtype == np.uint8 and g.shape == (3, 4, 1) and np.array_equal(g[..., 0], grey)
    assert np.array_equal(decode_frame(str(tmp_path / "rgb.png")), rgb)
    assert np.array_equal(decode_frame(str(tmp_path / "rgba.png")), rgba)
    pal = [10, 20, 30, 200, 100, 0, 0, 255, 7]
    idx = np.array([[0, 1, 2, 1], [2, 2, 0, 1], [1, 0, 0, 2]], np.uint8)
    p = Image.fromarray(idx, "P")
    p.putpalette(pal)
    p.save(str(tmp_path / "p.png"))
    p.save(str(tmp_path / "pt.png"), transparency=1)
    lut = np.array(pal, np.uint8).reshape(3, 3)
    assert np.array_equal(decode_frame(str(tmp_path / "p.png")), lut[idx])
    with_alpha = np.concatenate([lut[idx], np.where(idx == 1, 0, 255).astype(np.uint8)[..., None]], -1)
    assert np.array_equal(decode_frame(str(tmp_path / "pt.png")), with_alpha)
    Image.fromarray(grey > 127).save(str(tmp_path / "bw.png"))
    assert np.array_equal(decode_frame(str(tmp_path / "bw.png"))[..., 0], np.where(grey > 127, 255, 0).astype(np.uint8))


def test_two_channel_and_16_bit_images_are_refused(tmp_path):
    from casapose_amd.data_handler.image_only_dataset import decode_frame

    Image.fromarray(np.zeros((3, 4, 2), np.uint8), "LA").save(str(tmp_path / "la.png"))
    with pytest.raises(ValueError, match=r"la\.png: two-channel"):
        decode_frame(str(tmp_path / "la.png"))
    Image.fromarray(np.arange(12, dtype=np.uint16).reshape(3, 4) * 1000).save(str(tmp_path / "g16.png"))
    with pytest.raises(ValueError, match=r"g16\.png: 16-bit"):
        decode_frame(str(tmp_path / "g16.png"))
    _png16_rgb(str(tmp_path / "rgb16.png"), 3, 4)
    with pytest.raises(ValueError, match=r"rgb16\.png: 16-bit"):
        decode_frame(str(tmp_path / "rgb16.png"))


def test_reference_import_path_is_the_same_class():
    import casapose.data_handler.image_only_dataset as alias

    import casapose_amd.data_handler.image_only_dataset as real

    assert alias.ImageOnlyDataset is real.ImageOnlyDataset


@pytest.fixture(scope="module")
def lib():
    from casapose_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_frames_kernel_refuses_bad_arguments_before_any_launch(lib):
    """Never-dereferenced stand-in pointers: every call below is refused by its argument checks."""
    from casapose_amd import _lib

    src, out = C.c_void_p(4096), C.c_void_p(8192)
    good = dict(src=src, batch=2, h=4, w=5, channels=3, pitch=15, stride=60, n0=0.5, n1=0.5, out=out)
    bad = [dict(channels=2, pitch=10, stride=40), dict(channels=0), dict(channels=5, pitch=25, stride=100), dict(batch=0), dict(h=-1), dict(w=0),
           dict(pitch=14), dict(stride=59), dict(src=None), dict(out=None), dict(batch=1 << 20, h=1 << 10, w=2)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.cp_frames_to_input_f32(a["src"], a["batch"], a["h"], a["w"], a["channels"], a["pitch"], a["stride"], a["n0"], a["n1"], a["out"], None)
        assert rc == -1, change                                     # CP_ERR_INVALID
        assert lib.cp_last_error().startswith(b"cp_frames_to_input_f32:"), change
    with pytest.raises(_lib.CasaposeHipError, match="channels must be 1, 3 or 4"):
        _lib.check(lib.cp_frames_to_input_f32(src, 1, 4, 5, 2, 10, 40, 0.5, 0.5, out, None), "cp_frames_to_input_f32")
