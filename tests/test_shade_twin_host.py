"""The shaded mesh renderer's arithmetic on the CPU: `cp_render_shaded_host_f32` (the host twin of `cp_render_shaded_f32`: csrc/shade_math.h run
serially) and the source built on it (casapose_amd/data_handler/mesh_scene.py).

  twin label == mask twin label   byte for byte on the scenes of tests/test_masks_twin_host.py, at both sample offsets, no pixel excluded.
  twin == NumPy restatement       tests/shade_reference.py: keys, label, depth and dropped equal; img within 2.4e-7 (two fp32 ulps of 1) with a
                                  supplied background and against the procedural one.
  known answers                   a fronto-parallel quad whose vertices project onto exact 1/256 positions: the affine albedo, the shade under
                                  two lights, both windings, the flat colour.
  the triangle tie                a roof whose ridge projects through pixel centres: the lower triangle index wins exactly the ridge pixels.
  MeshSceneDataset on the twin    reproducibility across batches and shards, SyntheticSceneDataset's keys, the instance axis, keypoints on
                                  their instances, the refusals, read_vertex_colors."""
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import raster_reference as RR
import shade_reference as SR
import test_masks_twin_host as TM
from casapose_amd.data_handler.mesh_scene import MeshSceneDataset, ShadedRenderer, frame_record, parse_spec
from casapose_amd.data_handler.model_prep import write_keypoints_ply
from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
from casapose_amd.data_handler.vectorfield_dataset import read_vertex_colors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2.4e-7   # two fp32 ulps of 1: the image is fp64 arithmetic rounded once to fp32 in [-1, 1]
SCENES = ("three_ellipsoids", "batch_of_three", "full_frame_quad", "identical_twice", "near_plane")


def vertex_colors(meshes):
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (len(v), 3), dtype=np.uint8) for v, _ in meshes]


def flat_colors(meshes):
    return np.random.default_rng(6).uniform(0.15, 0.95, (len(meshes), 3)).astype(np.float32)


def lights_for(n):
    rng = np.random.default_rng(7)
    out = []
    for f in range(n):
        l = rng.normal(size=3)
        l /= np.linalg.norm(l)
        l[2] = -abs(l[2])
        out.append(frame_record(l, 0.3 + 0.05 * f, 0.6, 1000 + f, 17.0 + f, 23.0))
    return np.stack(out)


def renderer_for(meshes, colors=None, flat=None, device=None):
    return ShadedRenderer(device, {i: m for i, m in enumerate(meshes)}, None if colors is None else dict(enumerate(colors)),
                          None if flat is None else dict(enumerate(flat)))


def background_for(n, H, W):
    return np.random.default_rng(8).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def shaded(name, offset, with_background=True):
    """(scene, twin outputs, reference outputs) of a case: computed once, shared, never modified"""
    scene = TM.CASES[name]()
    meshes, frames, H, W, near, far = scene
    colors, flat, lights = vertex_colors(meshes), flat_colors(meshes), lights_for(len(frames))
    bg = background_for(len(frames), H, W) if with_background else None
    got = renderer_for(meshes, colors, flat).render_host(frames, lights, H, W, near, far, offset, background=bg)
    ref = SR.render_shaded_reference(meshes, colors, flat, frames, lights, H, W, near, far, offset, bg)
    for d in (got, ref):
        for a in d.values():
            if a is not None:
                a.setflags(write=False)
    return scene, got, ref


@pytest.mark.parametrize("offset", TM.OFFSETS)
@pytest.mark.parametrize("name", SCENES)
def test_label_is_the_mask_renderers(name, offset):
    _, labels, records, _, _ = TM.rendered(name, offset)
    _, got, _ = shaded(name, offset)
    assert got["label"].dtype == np.uint8 and np.array_equal(got["label"], labels), np.argwhere(got["label"] != labels)[:5]
    assert np.array_equal(got["dropped"], records[..., 10].sum(axis=1))


@pytest.mark.parametrize("offset", TM.OFFSETS)
@pytest.mark.parametrize("name", SCENES)
def test_twin_equals_the_numpy_restatement(name, offset):
    _, got, ref = shaded(name, offset)
    assert np.array_equal(got["keys"], ref["keys"]), np.argwhere(got["keys"] != ref["keys"])[:5]
    assert np.array_equal(got["label"], ref["label"]) and np.array_equal(got["dropped"], ref["dropped"])
    assert got["depth"].dtype == np.float32 and np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32))
    err = np.abs(got["img"].astype(np.float64) - ref["img"].astype(np.float64)).max()
    print("%s at offset %.1f: img differs from the restatement by at most %.3g" % (name, offset, err))
    assert got["img"].dtype == np.float32 and err <= TOL
    if name != "batch_of_three":
        assert (got["label"] > 0).sum() > 40 and np.ptp(got["img"][got["label"] > 0]) > 0.1   # something is shaded, and not flat


@pytest.mark.parametrize("name", ("three_ellipsoids", "batch_of_three"))
def test_procedural_background_against_the_restatement(name):
    _, got, ref = shaded(name, 0.5, False)
    err = np.abs(got["img"].astype(np.float64) - ref["img"].astype(np.float64)).max()
    print("%s, procedural background: img differs from the restatement by at most %.3g" % (name, err))
    assert err <= TOL and np.array_equal(got["keys"], ref["keys"])
    bgpix = got["img"][got["label"] == 0]
    assert len(bgpix) > 500 and np.ptp(bgpix) > 1e-3 and (bgpix[:, 0] == bgpix[:, 2]).all()   # the wave varies over the frame and is grey


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------
KA_CAM, KA_H, KA_W = (64.0, 64.0, 32.0, 32.0), 48, 56
KA_X, KA_Y = (-20, 12), (-15, 10)   # the quad's extent at Z = 64: columns 12 .. 43 and rows 17 .. 41 hold its interior pixel centres


def ka_quad(reverse=False):
    """X, Y integer at Z = 64 with fx = 64: u = X + 32 exactly.  Colours affine in (X, Y) and integer, so both triangles interpolate one plane."""
    v = np.array([[KA_X[0], KA_Y[0], 0], [KA_X[1], KA_Y[0], 0], [KA_X[1], KA_Y[1], 0], [KA_X[0], KA_Y[1], 0]], np.float32)
    col = np.stack([100 + 3 * v[:, 0], 120 + 4 * v[:, 1], 50 + v[:, 0] + 2 * v[:, 1]], axis=1).astype(np.uint8)
    f = np.array([[0, 2, 1], [0, 3, 2]] if reverse else [[0, 1, 2], [0, 2, 3]], np.int32)
    return (v, f), col


def ka_render(light, reverse=False, colors=True):
    mesh, col = ka_quad(reverse)
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [64.0]]], axis=1)
    frames = [dict(cam=KA_CAM, instances=[(0, 9, pose)])]
    r = renderer_for([mesh], [col], [(0.2, 0.5, 0.8)])
    return r.render_host(frames, frame_record(light, 0.3, 0.6, 1)[None], KA_H, KA_W, 1.0, 1000.0, 0.5, colors=colors)


def ka_albedo():
    jj, ii = np.meshgrid(np.arange(KA_W) + 0.5 - 32.0, np.arange(KA_H) + 0.5 - 32.0)
    return np.stack([100 + 3 * jj, 120 + 4 * ii, 50 + jj + 2 * ii], axis=-1) / 255.0


def test_known_answers_on_a_fronto_parallel_quad():
    inside = np.zeros((KA_H, KA_W), bool)
    inside[KA_Y[0] + 32:KA_Y[1] + 32, KA_X[0] + 32:KA_X[1] + 32] = True
    straight = ka_render((0.0, 0.0, -1.0))
    assert np.array_equal(straight["label"][0] == 9, inside) and (straight["depth"][0][inside] == 64.0).all()
    want = np.clip(ka_albedo() * (0.3 + 0.6), 0, 1) * 2 - 1
    err = np.abs(straight["img"][0].astype(np.float64) - want)[inside].max()
    assert err <= TOL, err
    tilted = ka_render((0.0, 0.6, -0.8))
    want = np.clip(ka_albedo() * (0.3 + 0.8 * 0.6), 0, 1) * 2 - 1
    err = np.abs(tilted["img"][0].astype(np.float64) - want)[inside].max()
    assert err <= TOL, err
    for light in ((0.0, 0.0, -1.0), (0.0, 0.6, -0.8)):
        a, b = ka_render(light), ka_render(light, reverse=True)
        assert a["img"].tobytes() == b["img"].tobytes() and a["label"].tobytes() == b["label"].tobytes() and a["depth"].tobytes() == b["depth"].tobytes()
    flat = ka_render((0.0, 0.0, -1.0), colors=False)
    want = np.clip(np.float32([0.2, 0.5, 0.8]).astype(np.float64) * 0.9, 0, 1) * 2 - 1
    assert np.abs(flat["img"][0][inside].astype(np.float64) - want).max() <= TOL and np.array_equal(flat["label"], straight["label"])


# ---- the triangle tie ------------------------------------------------------------------------------------------------------------------------
def roof(swap):
    """the ridge X = 0.5 at Z = 64 projects to u = 32.5, the centre of column 32, over rows 22 .. 41; the eaves lie 16 further back"""
    v = np.array([[0.5, -10, 0], [0.5, 10, 0], [-19.5, 0, 16], [20.5, 0, 16]], np.float32)
    f = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    return v, (f[::-1].copy() if swap else f)


def test_the_lower_triangle_index_wins_a_tie():
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [64.0]]], axis=1)
    frames = [dict(cam=KA_CAM, instances=[(0, 4, pose)])]
    light = frame_record((0.6, 0.0, -0.8), 0.3, 0.6, 1)[None]
    out = [renderer_for([roof(swap)], None, [(0.4, 0.6, 0.8)]).render_host(frames, light, 64, 64, 1.0, 1000.0, 0.5) for swap in (False, True)]
    ridge = np.zeros((64, 64), bool)
    ridge[22:42, 32] = True
    for o in out:
        tri = (o["keys"][0] & np.uint64(0xFFFFFF)).astype(np.int64)
        assert (o["label"][0][ridge] == 4).all() and (tri[ridge] == 0).all() and (o["depth"][0][ridge] == 64.0).all()
    left, right = out[0]["img"][0][30, 28], out[0]["img"][0][30, 36]     # triangle 0 is the left slope before the swap
    assert np.abs(left - right).max() > 0.05                               # the two slopes shade differently under this light
    assert (out[0]["img"][0][ridge] == left).all() and (out[1]["img"][0][ridge] == right).all()
    changed = (out[0]["img"][0] != out[1]["img"][0]).any(axis=-1)
    assert np.array_equal(changed, ridge)
    assert np.array_equal(out[0]["label"], out[1]["label"]) and np.array_equal(out[0]["depth"], out[1]["depth"])


# ---- the library's refusals --------------------------------------------------------------------------------------------------------------------
def test_library_refuses_bad_arguments(hip_lib):
    a, img, label, dropped, keys = np.zeros(64, np.float64), np.ones(48, np.float32), np.ones(16, np.uint8), np.ones(1, np.int32), np.zeros(16, np.uint64)
    p = a.ctypes.data
    ok = [p, p, 4, p, p, 4, 1, p, p, p, p, p, 1, 1, 4, 4, 1.0, 10.0, 0.5, None, p, p, None, 0, img.ctypes.data, label.ctypes.data, None,
          dropped.ctypes.data, keys.ctypes.data, 128]
    assert hip_lib.cp_render_shaded_host_f32(*ok) == 0 and (label == 0).all() and dropped[0] == 0 and (keys == SR.EMPTY).all()
    for at, bad, word in ((12, 0, b"frames"), (13, 257, b"instances_max"), (14, 16385, b"H and W"), (16, 0.0, b"near"), (5, (1 << 24) + 1, b"Tmax"),
                          (29, 127, b"workspace"), (20, None, b"null")):
        args = list(ok)
        args[at] = bad
        assert hip_lib.cp_render_shaded_host_f32(*args) == -1 and word in hip_lib.cp_last_error(), word
        assert hip_lib.cp_render_shaded_f32(*args, None) == -1 and word in hip_lib.cp_last_error(), word
    assert hip_lib.cp_render_shaded_workspace_bytes(3, 480, 640) == 3 * 480 * 640 * 8
    assert hip_lib.cp_render_shaded_workspace_bytes(0, 480, 640) == 0 and hip_lib.cp_render_shaded_workspace_bytes(1, 16385, 4) == 0


def test_the_pair_is_listed_and_reachable():
    from casapose_amd import _lib

    assert _lib.host_twin("cp_render_shaded_f32") == "cp_render_shaded_host_f32" and "cp_render_shaded_f32" not in _lib.TWINS
    assert _lib.TWIN_OUTPUT_VARIANTS == {"cp_render_shaded_f32": "cp_render_shaded_host_f32"}
    assert _lib.POINTEES["cp_render_shaded_f32"] == _lib.POINTEES["cp_render_shaded_host_f32"] + ("void",)


def test_selftest_passes():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "casapose_amd", "csrc"), "shade-selftest"], capture_output=True, text=True)
    assert r.returncode == 0 and "shade_selftest: ok" in r.stdout, r.stdout + r.stderr


# ---- MeshSceneDataset --------------------------------------------------------------------------------------------------------------------------
AXES = {"obj_000001": (26.0, 20.0, 23.0), "obj_000004": (19.0, 28.0, 17.0), "obj_000009": (22.0, 22.0, 22.0)}
SIZE = (40, 72)


def write_colored_ply(path, vertices, faces, colors=None):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(vertices))
        if colors is not None:
            f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces))
        for n, p in enumerate(vertices):
            f.write("%.9g %.9g %.9g" % tuple(p) + ("" if colors is None else " %d %d %d" % tuple(colors[n])) + "\n")
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(t))


def write_mesh_folder(root, keypoints=True, faces=True, points=9):
    """BOP's flat layout: three ellipsoids (the first two with vertex colours), their keypoint files and models_info.json"""
    os.makedirs(root)
    rng = np.random.default_rng(3)
    for n, (stem, axes) in enumerate(AXES.items()):
        v, f = TM.ellipsoid(2, axes)
        write_colored_ply(root / (stem + ".ply"), v, f if faces else f[:0], rng.integers(30, 256, (len(v), 3)) if n < 2 else None)
        if keypoints:
            write_keypoints_ply(str(root / (stem + "_keypoints.ply")), TM.keypoints_of(axes)[:points])
    json.dump({str(int(s[4:])): {"diameter": 2.0 * max(a)} for s, a in AXES.items()}, open(root / "models_info.json", "w"))
    return str(root)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return write_mesh_folder(tmp_path_factory.mktemp("meshes") / "models")


def test_image_i_is_the_same_alone_in_a_batch_and_from_a_shard(folder):
    ds = MeshSceneDataset(folder, 2, SIZE, length=8, seed=4)
    whole = ds.batch(0, 4)
    for i in range(4):
        alone = ds.batch(i, 1)
        for k in whole:
            assert np.array_equal(alone[k][0].numpy(), whole[k][i].numpy()), (k, i)
    for rank in (0, 1):
        part = ds.batch(0, 4, shard=(rank, 2))
        for k in whole:
            assert np.array_equal(part[k].numpy(), whole[k][2 * rank:2 * rank + 2].numpy()), (k, rank)
    again = MeshSceneDataset(folder, 2, SIZE, length=8, seed=4).batch(0, 4)
    assert all(np.array_equal(again[k].numpy(), whole[k].numpy()) for k in whole)
    assert not np.array_equal(whole["img"][0].numpy(), whole["img"][1].numpy())
    assert (whole["pixel_gt_count"].numpy() > 20).all() and np.abs(whole["img"].numpy()).max() <= 1.0


def test_batch_has_the_synthetic_sources_keys_shapes_and_dtypes(folder):
    for instances in (1, 3):
        want = SyntheticSceneDataset(2, SIZE, length=4, seed=4, instances=instances).batch(0, 2)
        got = MeshSceneDataset(folder, 2, SIZE, length=4, seed=4, instances=instances).batch(0, 2)
        assert list(got) == list(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        assert np.array_equal(got["offsets"].numpy(), want["offsets"].numpy())            # the same crop draw comes first
        assert np.array_equal(got["poses_gt"].numpy(), want["poses_gt"].numpy())          # and the same pose draws follow it
        lab = got["filtered_seg"][..., 0].numpy()
        assert np.array_equal(got["target_seg"].numpy(), np.eye(3, dtype=np.float32)[lab])
        assert np.array_equal(got["pixel_gt_count"][:, :, 0, 0].numpy(), np.stack([(lab == o + 1).sum((1, 2)) for o in range(2)], 1))


def test_instance_axis_padding_and_keypoints_on_their_instances(folder):
    I = 3
    ds = MeshSceneDataset(folder, 2, SIZE, length=6, seed=9, instances=I)
    b = ds.batch(0, 6)
    raw = ds.render_twin(range(6), depth=True)
    count = b["instance_count"].numpy()
    assert count.dtype == np.int32 and count.min() >= 1 and count.max() == I and len(np.unique(count)) > 1
    lab, iseg = ds.split_slots(raw["slots"])
    assert np.array_equal(b["filtered_seg"][..., 0].numpy(), lab) and np.array_equal(b["instance_seg"].numpy(), iseg)
    kp2, poses = b["target_vert"].numpy(), b["poses_gt"].numpy()
    checked = 0
    for n in range(6):
        present = set(np.unique(raw["slots"][n]).tolist()) - {0}
        assert present <= {o * I + r + 1 for o in range(2) for r in range(count[n, o])}          # the slot map names drawn instances only
        for o in range(2):
            for r in range(I):
                if r >= count[n, o]:
                    assert (kp2[n, o, r] == -1000).all() and (poses[n, o, r] == 0).all() and b["diameters"][n, o, r] == -1
                    assert (b["keypoints3d"][n, o, r].numpy() == -1000).all()
                    continue
                assert b["diameters"][n, o, r] == 2.0 * max(list(AXES.values())[o])
                y, x = np.floor(kp2[n, o, r, 0]).astype(int)      # keypoint 0 is the model origin: the ellipsoid's centre
                assert 0 <= y < SIZE[0] and 0 <= x < SIZE[1]
                slot = raw["slots"][n, y, x]
                assert slot == o * I + r + 1 or (slot > 0 and raw["depth"][n, y, x] < poses[n, o, r, 2, 3]), (n, o, r, slot)
                checked += slot == o * I + r + 1
    assert checked > 0   # the first branch was taken: some centres are visible themselves


def test_refusals_name_the_file_and_the_command(tmp_path):
    with pytest.raises(ValueError, match=r"obj_000001_keypoints\.ply is missing.*make_keypoints\.py --model_folder"):
        MeshSceneDataset(write_mesh_folder(tmp_path / "a", keypoints=False), 2, SIZE)
    with pytest.raises(ValueError, match=r"obj_000001\.ply has no faces"):
        MeshSceneDataset(write_mesh_folder(tmp_path / "b", faces=False), 2, SIZE)
    with pytest.raises(ValueError, match=r"obj_000001_keypoints\.ply holds 8 keypoints, no_points is 9"):
        MeshSceneDataset(write_mesh_folder(tmp_path / "c", points=8), 2, SIZE)
    folder = write_mesh_folder(tmp_path / "d")
    os.remove(os.path.join(folder, "models_info.json"))
    with pytest.raises(ValueError, match=r"diameter in models_info\.json is missing for obj_000001.*make_keypoints\.py"):
        MeshSceneDataset(folder, 2, SIZE)
    with pytest.raises(ValueError, match="holds 3 meshes, 4 objects"):
        MeshSceneDataset(write_mesh_folder(tmp_path / "e"), 4, SIZE)
    assert parse_spec("meshes:/a/b:16") == ("/a/b", 16) and parse_spec("meshes:/a/b") == ("/a/b", None) and parse_spec("meshes:c:\\m") == ("c:\\m", None)


def test_backgrounds_from_a_folder_of_pictures(folder, tmp_path):
    from PIL import Image

    os.makedirs(tmp_path / "bg")
    rng = np.random.default_rng(1)
    for n, size in enumerate(((50, 90), (120, 80))):
        Image.fromarray(rng.integers(0, 256, size + (3,), dtype=np.uint8)).save(tmp_path / "bg" / ("%d.png" % n))
    plain = MeshSceneDataset(folder, 2, SIZE, length=4, seed=4)
    ds = MeshSceneDataset(folder, 2, SIZE, length=4, seed=4, backgrounds=str(tmp_path / "bg"))
    a, b = plain.batch(0, 2, noise=False), ds.batch(0, 2, noise=False)
    lab = a["filtered_seg"][..., 0].numpy()
    assert np.array_equal(lab, b["filtered_seg"][..., 0].numpy()) and np.array_equal(a["img"].numpy()[lab > 0], b["img"].numpy()[lab > 0])
    assert np.ptp(b["img"].numpy()[lab == 0]) > 1.0 > np.ptp(a["img"].numpy()[lab == 0])   # a random picture against the wave
    assert np.array_equal(ds.batch(0, 2, noise=False)["img"].numpy(), b["img"].numpy())


def test_read_vertex_colors(tmp_path):
    v, f = TM.ellipsoid(0, (1, 1, 1))
    col = np.random.default_rng(2).integers(0, 256, (len(v), 3)).astype(np.uint8)
    write_colored_ply(tmp_path / "a.ply", v, f, col)
    got = read_vertex_colors(str(tmp_path / "a.ply"))
    assert got.dtype == np.uint8 and np.array_equal(got, col)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
            "property uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n" % len(v)).encode()
    (tmp_path / "b.ply").write_bytes(head + b"".join(struct.pack("<fff4B", *p, *c, 255) for p, c in zip(v.tolist(), col.tolist())))
    assert np.array_equal(read_vertex_colors(str(tmp_path / "b.ply")), col)
    write_colored_ply(tmp_path / "c.ply", v, f)
    assert read_vertex_colors(str(tmp_path / "c.ply")) is None
    (tmp_path / "d.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert read_vertex_colors(str(tmp_path / "d.obj")) is None


def test_the_folder_reader_serves_a_meshes_root(folder):
    """what test_casapose.py does with `--datatest meshes:<folder>:4`: its folder branch builds VectorfieldDataset and calls these methods"""
    from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset

    ds = VectorfieldDataset(root="meshes:%s:4" % folder, path_meshes="", no_points=9, objectsofinterest=["obj_000001", "obj_000004"], noise=0.00001,
                            contrast=0.00001, brightness=0.00001, random_translation=(0, 0), random_rotation=0, random_crop=False)
    it, batches = ds.generate_dataset(1, 1, 0, SIZE, 1.0, 1, 2, shuffle=False)
    want = MeshSceneDataset(folder, 2, SIZE, length=4, seed=0, random_crop=False)
    assert batches == 4 == len(ds)
    for i in range(4):
        got, ref = next(it), want.batch(i, 1)
        assert list(got) == list(ref) and all(np.array_equal(got[k].numpy(), ref[k].numpy()) for k in ref)
    verts, counts = ds.generate_object_vertex_array()
    assert verts.shape == (2, 162, 3) and verts.dtype == np.float32 and counts.tolist() == [[162], [162]]
    assert VectorfieldDataset(root="meshes:%s" % folder, path_meshes="", objectsofinterest=["a", "b"]).mesh_scenes(SIZE).length == 32
