"""The mask renderer's arithmetic on the CPU: `cp_render_masks_host_u8` (the host twin of `cp_render_masks_u8`: csrc/mask_math.h run serially)
against three references of tests/raster_reference.py, and the BOP converter built on it (casapose_amd/data_handler/bop_converter.py).

  twin == NumPy restatement      labels and records byte for byte on every case of CASES, at sample offsets 0.5 and 0.0.
  twin ~ un-snapped ray caster   labels equal on every pixel whose sample is at least 2/256 px from the edge lines around it; the excluded
                                 share is itself asserted to be at most 5 % of the image.
  twin ~ analytic ellipsoid      one subdivision-4 icosphere stretched to SyntheticSceneDataset's own axes against that dataset's analytic hit
                                 test: the rendered silhouette lies between the analytic one and the analytic one of the ellipsoid shrunk by the
                                 tessellation's sagitta (derived below), so every differing pixel touches the analytic boundary.
  read_faces, the conversion against files the reference's own code wrote (tests/golden/bop_converter/, made by
  tests/golden/make_bop_converter_golden.py), the round trip converter -> VectorfieldDataset, the refusals, the command line."""
import functools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import raster_reference as RR
from casapose_amd._lib import CasaposeHipError
from casapose_amd.data_handler import bop_converter as BC
from casapose_amd.data_handler.synthetic_scene import CAMERA, SyntheticSceneDataset
from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset, read_faces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bop_converter")
CAM = (100.0, 101.0, 31.7, 23.4)
OFFSETS = (0.5, 0.0)


def ellipsoid(subdivisions, axes):
    v, f = RR.icosphere(subdivisions)
    return (v * np.asarray(axes, np.float64)).astype(np.float32), f


def three_ellipsoids():
    """48 x 64: A in front of B (they overlap in the image, 5 mm apart in depth at the closest), C cut by the right border"""
    meshes = [ellipsoid(2, (70, 50, 60)), ellipsoid(2, (55, 75, 45)), ellipsoid(2, (60, 60, 80))]
    inst = [(0, 3, RR.pose_at(CAM, 22.3, 24.1, 500.0, RR.rotation((1, 2, 3), 0.7))),
            (1, 7, RR.pose_at(CAM, 31.6, 26.2, 650.0, RR.rotation((3, -1, 2), 1.9))),
            (2, 200, RR.pose_at(CAM, 60.2, 11.3, 560.0, RR.rotation((-1, 1, 4), 2.6)))]
    return meshes, [dict(cam=CAM, instances=inst)], 48, 64, 100.0, 2000.0


def batch_of_three():
    """50 x 70 (a width that is no multiple of 4), frames with 0, 1 and 3 instances and their own cameras"""
    meshes, frames, _, _, near, far = three_ellipsoids()
    inst = frames[0]["instances"]
    cam1, cam2 = (90.0, 92.0, 35.2, 24.9), (110.0, 108.0, 33.1, 26.6)
    return meshes, [dict(cam=CAM, instances=[]), dict(cam=cam1, instances=[inst[1]]), dict(cam=cam2, instances=list(inst))], 50, 70, near, far


def full_frame_quad():
    """40 x 72: a two-triangle quad that covers every pixel (each triangle's box holds far more than 1024 samples: the cooperative path) behind a
    small ellipsoid"""
    quad = (np.array([[-900, -700, 0], [900, -700, 0], [900, 700, 0], [-900, 700, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    cam = (100.0, 100.0, 36.3, 19.8)
    inst = [(0, 1, RR.pose_at(cam, 36.0, 20.0, 900.0, RR.rotation((1, 0.3, 0), 0.2))), (1, 2, RR.pose_at(cam, 30.5, 15.5, 400.0))]
    return [quad, ellipsoid(2, (40, 30, 35))], [dict(cam=cam, instances=inst)], 40, 72, 100.0, 2000.0


def tiny_and_degenerate():
    """24 x 32: an ellipsoid three pixels across (triangles far smaller than a pixel) with zero-area faces appended (a repeated vertex, three
    collinear vertices, one vertex three times), in front of a larger one"""
    v, f = ellipsoid(2, (8, 6, 7))
    v = np.concatenate([v, np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)])
    n = len(v)
    f = np.concatenate([f, np.array([[0, 0, 5], [n - 3, n - 2, n - 1], [4, 4, 4]], np.int32)])
    cam = (100.0, 100.0, 15.6, 12.2)
    inst = [(0, 9, RR.pose_at(cam, 14.2, 11.7, 500.0)), (1, 4, RR.pose_at(cam, 17.0, 12.0, 700.0, RR.rotation((0, 1, 1), 0.5)))]
    return [(v, f), ellipsoid(2, (50, 40, 45))], [dict(cam=cam, instances=inst)], 24, 32, 100.0, 2000.0


def identical_twice():
    """two identical instances at one pose, labels 7 and 9: every depth ties, the lower index wins every pixel"""
    meshes, frames, H, W, near, far = three_ellipsoids()
    pose = frames[0]["instances"][0][2]
    return meshes, [dict(cam=CAM, instances=[(0, 7, pose), (0, 9, pose)])], H, W, near, far


def near_plane():
    """an ellipsoid that reaches in front of the near plane (centre at 150, near 120): the triangles with a vertex there are dropped whole"""
    meshes = [ellipsoid(2, (30, 25, 40)), ellipsoid(2, (30, 30, 30))]
    inst = [(0, 5, RR.pose_at(CAM, 30.0, 22.0, 150.0, RR.rotation((1, 1, 0), 0.4))), (1, 6, RR.pose_at(CAM, 54.0, 38.0, 600.0))]
    return meshes, [dict(cam=CAM, instances=inst)], 48, 64, 120.0, 2000.0


CASES = {"three_ellipsoids": three_ellipsoids, "batch_of_three": batch_of_three, "full_frame_quad": full_frame_quad,
         "tiny_and_degenerate": tiny_and_degenerate, "identical_twice": identical_twice, "near_plane": near_plane}


def renderer_for(meshes, device=None):
    return BC.MaskRenderer(device, {i: m for i, m in enumerate(meshes)})


@functools.lru_cache(maxsize=None)
def rendered(name, offset):
    """(scene, twin labels, twin records, reference labels, reference records) of a case: computed once, shared, never modified"""
    scene = CASES[name]()
    meshes, frames, H, W, near, far = scene
    labels, records = renderer_for(meshes).render_host(frames, H, W, near, far, offset)
    ref_labels, ref_records = RR.render_reference(meshes, frames, H, W, near, far, offset)
    for a in (labels, records, ref_labels, ref_records):
        a.setflags(write=False)
    return scene, labels, records, ref_labels, ref_records


def check_case_content(name, labels, records):
    """the case holds what it means to hold"""
    all_, visib, dropped = records[..., 0], records[..., 1], records[..., 10]
    if name == "three_ellipsoids":
        assert (labels == 0).sum() > 500 and all((labels == lab).sum() > 40 for lab in (3, 7, 200))
        assert all_[0, 0] == visib[0, 0] > 0 and all_[0, 1] > visib[0, 1] > 0                       # A whole, B partly occluded
        assert records[0, 2, 2] + records[0, 2, 4] == 63 and (dropped == 0).all()                    # C reaches the last column
    elif name == "batch_of_three":
        assert (labels[0] == 0).all() and (records[0, :, 0] == 0).all() and (records[0, :, 2:10] == -1).all()
        assert visib[1, 0] == all_[1, 0] > 40 and (records[1, 1:, 0] == 0).all() and set(np.unique(labels[1])) == {0, 7}
        assert set(np.unique(labels[2])) == {0, 3, 7, 200} and all_[2, 1] > visib[2, 1] > 0
    elif name == "full_frame_quad":
        assert (labels == 0).sum() == 0 and all_[0, 0] == 40 * 72 and list(records[0, 0, 2:6]) == [0, 0, 71, 39]
        assert visib[0, 1] == all_[0, 1] > 40 and visib[0, 0] == 40 * 72 - visib[0, 1]
    elif name == "tiny_and_degenerate":
        assert 3 <= all_[0, 0] <= 16 and visib[0, 0] == all_[0, 0] and all_[0, 1] > visib[0, 1] > 40 and (labels == 0).sum() > 100
        assert (dropped == 0).all()
    elif name == "identical_twice":
        assert all_[0, 0] == all_[0, 1] == visib[0, 0] > 40 and visib[0, 1] == 0 and set(np.unique(labels)) == {0, 7}
        assert list(records[0, 1, 6:10]) == [-1, -1, -1, -1] and list(records[0, 1, 2:6]) == list(records[0, 0, 2:6])
    elif name == "near_plane":
        assert 0 < dropped[0, 0] < 320 and dropped[0, 1] == 0 and all_[0, 0] > 40 and all_[0, 1] > 40 and (labels == 0).sum() > 100


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_the_numpy_restatement(name, offset):
    _, labels, records, ref_labels, ref_records = rendered(name, offset)
    check_case_content(name, ref_labels, ref_records)
    assert labels.dtype == np.uint8 and records.dtype == np.int32 and records.shape == ref_records.shape
    assert np.array_equal(records, ref_records), np.argwhere(records != ref_records)[:5]
    assert np.array_equal(labels, ref_labels), np.argwhere(labels != ref_labels)[:5]


def test_near_plane_drops_are_counted_from_the_vertices():
    """the dropped count is the number of faces with a vertex at Z < near, computed here from the camera points alone"""
    (meshes, frames, H, W, near, far), _, records, _, _ = rendered("near_plane", 0.5)
    obj, _, pose = frames[0]["instances"][0]
    Z = RR.camera_points(meshes[obj][0], pose)[2]
    assert records[0, 0, 10] == int((Z[meshes[obj][1]] < near).any(axis=1).sum()) > 0


@pytest.mark.parametrize("offset", OFFSETS)
def test_twin_against_the_unsnapped_ray_caster(offset):
    (meshes, frames, H, W, near, far), labels, _, _, _ = rendered("three_ellipsoids", offset)
    cast, depths = RR.ray_cast(meshes, frames[0], H, W, near, far, offset)
    # the instances do not interpenetrate: wherever two are hit, the two nearest hit depths are apart
    two = np.sort(depths, axis=0)[:2]
    both = np.isfinite(two[1])
    assert both.sum() > 20 and (two[1][both] - two[0][both] > 1e-3 * two[1][both]).all()
    band = RR.edge_band(meshes, frames[0], H, W, near, offset)
    share, differing = band.mean(), int((labels[0] != cast).sum())
    print("offset %.1f: %.2f %% of the image within 2/256 px of an edge line, %d pixels differ in all, %d outside the band"
          % (offset, 100 * share, differing, int(((labels[0] != cast) & ~band).sum())))
    assert share <= 0.05
    assert np.array_equal(labels[0][~band], cast[~band])
    assert (cast > 0).sum() > 300 and (cast == 0).sum() > 500


def test_twin_against_the_analytic_ellipsoid():
    """A mesh inscribed in an ellipsoid, rendered at sample offset 0.5, against SyntheticSceneDataset's analytic ray / ellipsoid test (pixel centres
    at + 0.5 too).  With d = the smallest distance of a face plane of the unit icosphere from the origin, the polyhedron contains the ball of
    radius d, and a linear map keeps containment: the mesh contains the ellipsoid scaled by d about its centre, and is contained in the
    ellipsoid.  Projection keeps containment as well, so   analytic(d * axes)  <=  rendered  <=  analytic(axes)   pixel by pixel, up to what
    moves a silhouette edge: vertices snapped by at most 1/512 px per coordinate (sqrt(2) / 512 px) and stored in fp32 (1e-5 mm).  The inner
    ellipsoid is therefore shrunk once more by that distance over the smallest projected semi-axis."""
    H, W, hc, wc = 120, 160, 180, 240
    ds = SyntheticSceneDataset(1, (H, W), seed=3, random_crop=False)
    z = 700.0
    pose = RR.pose_at((CAMERA[0, 0], CAMERA[1, 1], CAMERA[0, 2], CAMERA[1, 2]), wc + 81.3, hc + 58.6, z, RR.rotation((2, -1, 1), 1.1))
    _, outer = ds._pixels(None, hc, wc, pose[None], noise=False)
    sphere, faces = RR.icosphere(4)
    tri = sphere[faces]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    d = float(np.abs((normal * tri[:, 0]).sum(1) / np.linalg.norm(normal, axis=1)).min())   # 1 - d is the sagitta of the unit tessellation
    smallest_px = CAMERA[0, 0] * ds.axes.min() / (z + ds.axes.max())
    shrink = d - (np.sqrt(2.0) / 512.0 + 1e-4) / smallest_px
    assert 0.99 < shrink < d < 1.0
    inner_ds = SyntheticSceneDataset(1, (H, W), seed=3, random_crop=False)
    inner_ds.axes = ds.axes * shrink
    _, inner = inner_ds._pixels(None, hc, wc, pose[None], noise=False)
    mesh = ((sphere * ds.axes[0]).astype(np.float32), faces)
    cam = (CAMERA[0, 0], CAMERA[1, 1], CAMERA[0, 2] - wc, CAMERA[1, 2] - hc)
    labels, records = renderer_for([mesh]).render_host([dict(cam=cam, instances=[(0, 1, pose)])], H, W, 100.0, 2000.0, 0.5)
    got, outer, inner = labels[0] > 0, outer > 0, inner > 0
    print("analytic %d px, rendered %d px, shrunk analytic %d px (sagitta %.2e of the radius)" % (outer.sum(), got.sum(), inner.sum(), 1 - d))
    assert outer.sum() > 3000 and records[0, 0, 0] == got.sum() and records[0, 0, 10] == 0
    assert not (got & ~outer).any() and got.sum() <= outer.sum()          # an inscribed mesh cannot exceed the analytic silhouette
    assert not (inner & ~got).any()                                        # and falls short by no more than the sagitta allows
    assert outer.sum() - got.sum() <= outer.sum() - inner.sum()
    pad = np.pad(outer, 1, mode="edge")
    boundary = np.zeros_like(outer)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            boundary |= pad[di:di + H, dj:dj + W] != outer                  # a pixel with an 8-neighbour on the other side of the silhouette
    assert not ((got != outer) & ~boundary).any()


# ---- read_faces ----------------------------------------------------------------------------------------------------------------------------
QUAD_AND_TRIANGLE = np.array([[0, 1, 2], [0, 2, 3], [4, 0, 3]], np.int32)   # the quad 0 1 2 3 as a fan, then the triangle 4 0 3


def test_read_faces_ascii_ply(tmp_path):
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 2\nproperty uchar flags\nproperty list uchar int vertex_indices\nproperty float quality\nend_header\n"
                 "0 0 0\n1 0 0\n1 1 0\n0 1 0\n0 0 1\n7 4 0 1 2 3 0.5\n9 3 4 0 3 0.25\n")
    assert np.array_equal(read_faces(str(p)), QUAD_AND_TRIANGLE) and read_faces(str(p)).dtype == np.int32


def test_read_faces_binary_ply(tmp_path):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
            "element face 2\nproperty list uchar uint vertex_index\nproperty float quality\nend_header\n").encode()
    verts = b"".join(struct.pack("<fffB", *v, 200) for v in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1)))
    faces = struct.pack("<B4If", 4, 0, 1, 2, 3, 0.5) + struct.pack("<B3If", 3, 4, 0, 3, 0.25)
    p = tmp_path / "b.ply"
    p.write_bytes(head + verts + faces)
    assert np.array_equal(read_faces(str(p)), QUAD_AND_TRIANGLE)
    # all triangles: the structured read
    p.write_bytes(head.replace(b"element face 2", b"element face 3") + verts + b"".join(struct.pack("<B3If", 3, *t, 1.0) for t in QUAD_AND_TRIANGLE.tolist()))
    assert np.array_equal(read_faces(str(p)), QUAD_AND_TRIANGLE)
    # a file without faces
    p.write_bytes(head.replace(b"element face 2", b"element face 0") + verts)
    assert read_faces(str(p)).shape == (0, 3)


def test_read_faces_obj(tmp_path):
    p = tmp_path / "c.obj"
    p.write_text("# by hand\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1 4/1/1\nf 5//1 1//1 -2//1\n")
    assert np.array_equal(read_faces(str(p)), QUAD_AND_TRIANGLE)


def test_read_faces_refusals(tmp_path):
    p = tmp_path / "mesh.stl"
    p.write_text("solid\n")
    with pytest.raises(ValueError, match="mesh.stl"):
        read_faces(str(p))
    q = tmp_path / "big.ply"
    q.write_text("ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="big.ply.*binary_big_endian"):
        read_faces(str(q))
    r = tmp_path / "short.ply"
    r.write_text("ply\nformat ascii 1.0\nelement face 1\nproperty list ushort int vertex_indices\nend_header\n3 0 1 2\n")
    with pytest.raises(ValueError, match="short.ply.*property list uchar"):
        read_faces(str(r))
    s = tmp_path / "no.ply"
    s.write_text("plx\n")
    with pytest.raises(ValueError, match="no.ply"):
        read_faces(str(s))


# ---- the conversion against files written by the reference's own code ---------------------------------------------------------------------------
def assert_json_equal(got, want, where=""):
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (where, list(got), list(want))
        for k in want:
            if k in ("cuboid", "projected_cuboid"):   # the stated difference: the axis-aligned box instead of trimesh's oriented one
                continue
            assert_json_equal(got[k], want[k], where + "/" + k)
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            assert_json_equal(g, w, "%s[%d]" % (where, i))
    elif isinstance(want, float):
        assert isinstance(got, float) and abs(got - want) <= 1e-12 * abs(want), (where, got, want)
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


def golden_meshes():
    raw = json.load(open(os.path.join(GOLDEN, "meshes.json")))
    return {int(k): dict(name=m["name"], keypoints=np.array(m["keypoints"]), volume=np.array(m["volume"]), volume_size=np.array(m["volume_size"]),
                         center=np.array(m["center"]), counter=0, fixed_model_transform=np.array(m["fixed_model_transform"]), id=m["id"])
            for k, m in raw.items()}


@pytest.mark.parametrize("variant", ("with_info", "without_info"))
def test_conversion_equals_the_reference_code(tmp_path, variant):
    files = [os.path.join(GOLDEN, "scene", n) for n in ("scene_camera.json", "scene_gt.json") + (("scene_gt_info.json",) if variant == "with_info" else ())]
    info, gt = BC.load_json_info(sorted(files))
    meshes = golden_meshes()
    BC.write_camera_setting(str(tmp_path / "_camera_settings.json"), "Viewpoint", next(iter(info.values()))["cam_mat"], 640, 480)
    for idx in sorted(gt):
        meshes = BC.create_ndds_json(str(tmp_path / ("%06d.json" % idx)), info[idx]["cam_mat"], gt[idx], meshes)
    BC.write_object_settings(str(tmp_path / "_object_settings.json"), meshes)
    names = sorted(n for n in os.listdir(os.path.join(GOLDEN, variant)) if n != "reference_raises.json")
    assert names == sorted(os.listdir(tmp_path)) and len(names) == 4
    for n in names:
        assert_json_equal(json.load(open(tmp_path / n)), json.load(open(os.path.join(GOLDEN, variant, n))), n)
    if variant == "without_info":
        # the stated difference: without scene_gt_info.json the reference's create_ndds_json stops at mesh_gt["bb"]; its files in this folder were
        # written after the generator gave every ground-truth entry the empty box this build writes
        assert json.load(open(os.path.join(GOLDEN, variant, "reference_raises.json"))) == {"error": "KeyError", "key": "bb", "bb_given": [-1, -1, -1, -1]}
        assert "px_count_all" not in json.load(open(tmp_path / "000000.json"))["objects"][0]


def test_to_json_layout():
    from casapose_amd.utils.io_utils import to_json

    text = to_json({"a": [1, 2.5, "x"], "b": [[1, 2], [3, 4]], "c": {"d": np.array([1.0, 2.0]), "e": None, "f": True}, "g": np.array([1, 2])})
    assert text == ('{\n    "a": [ 1, 2.5, "x" ],\n    "b": [ \n        [ 1, 2 ], \n        [ 3, 4 ]\n     ],\n    "c": \n    {\n        "d": [1,2],\n'
                    '        "e": null,\n        "f": true\n    },\n    "g": [1,2]\n}')
    assert json.loads(text) == {"a": [1, 2.5, "x"], "b": [[1, 2], [3, 4]], "c": {"d": [1, 2], "e": None, "f": True}, "g": [1, 2]}
    with pytest.raises(TypeError):
        to_json({"a": np.int64(3)})


# ---- the round trip into the reader ------------------------------------------------------------------------------------------------------------
H, W = 96, 128
BOP_CAM = (120.0, 121.0, 63.6, 47.2)
OBJECTS = {1: (40.0, 30.0, 35.0), 5: (30.0, 45.0, 25.0)}
NAMES = ["obj_000001", "obj_000005"]


def bop_poses():
    return [[(1, RR.pose_at(BOP_CAM, 50.0, 45.0, 500.0, RR.rotation((1, 2, 3), 0.7))), (5, RR.pose_at(BOP_CAM, 62.0, 50.0, 640.0, RR.rotation((3, -1, 2), 1.9)))],
            [(5, RR.pose_at(BOP_CAM, 40.0, 40.0, 450.0, RR.rotation((0, 1, 1), 0.5))), (1, RR.pose_at(BOP_CAM, 100.0, 70.0, 560.0, RR.rotation((-1, 1, 4), 2.6)))]]


def write_ply(path, vertices, faces=None):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(vertices))
        if faces is not None:
            f.write("element face %d\nproperty list uchar int vertex_indices\n" % len(faces))
        f.write("end_header\n")
        for p in vertices:
            f.write("%.9g %.9g %.9g\n" % tuple(p))
        for t in ([] if faces is None else faces):
            f.write("3 %d %d %d\n" % tuple(t))


def keypoints_of(axes):
    a = np.asarray(axes)
    return np.concatenate([np.zeros((1, 3)), np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * a])


def write_bop_tree(root, with_masks=None, faces=True):
    """<root>/models and <root>/test/000002 in BOP layout; with_masks: the label maps to cut mask_visib/ from"""
    from PIL import Image

    models, scene = root / "models", root / "test" / "000002"
    os.makedirs(models)
    os.makedirs(scene / "rgb")
    meshes = {}
    for obj, axes in OBJECTS.items():
        v, f = ellipsoid(2, axes)
        meshes[obj] = (v, f)
        write_ply(models / ("obj_%06d.ply" % obj), v, f if faces else None)
        write_ply(models / ("obj_%06d_keypoints.ply" % obj), keypoints_of(axes))
    json.dump({str(o): {"diameter": 2.0 * max(a)} for o, a in OBJECTS.items()}, open(models / "models_info.json", "w"))
    poses = bop_poses()
    K = [BOP_CAM[0], 0.0, BOP_CAM[2], 0.0, BOP_CAM[1], BOP_CAM[3], 0.0, 0.0, 1.0]
    json.dump({str(i): {"cam_K": K, "depth_scale": 1.0} for i in range(2)}, open(scene / "scene_camera.json", "w"))
    json.dump({str(i): [{"cam_R_m2c": P[:, :3].reshape(-1).tolist(), "cam_t_m2c": P[:, 3].tolist(), "obj_id": o} for o, P in poses[i]] for i in range(2)},
              open(scene / "scene_gt.json", "w"))
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(scene / "rgb" / ("%06d.png" % i))
    if with_masks is not None:
        os.makedirs(scene / "mask_visib")
        for i in range(2):
            for k, (o, _) in enumerate(poses[i]):
                Image.fromarray(((with_masks[i] == o) * 255).astype(np.uint8)).save(scene / "mask_visib" / ("%06d_%06d.png" % (i, k)))
    return meshes, poses


def settings_for(**kw):
    return dict(dict(near=100.0, far=2000.0, width=W, height=H, filetype_in="png", mask="render", copy_meshes=True, draw_debug_image=False,
                     gt_info="render", renderer="host"), **kw)


def read_back(out):
    ds = VectorfieldDataset(str(out / "test"), str(out / "models"), objectsofinterest=NAMES, color_input=True, noise=0, brightness=0, contrast=0,
                            random_translation=(0, 0), random_rotation=0, random_crop=False, test=True)
    assert len(ds) == 2
    it, nb = ds.generate_dataset(2, 1, 0, (H, W), 1.0, 1, len(NAMES), shuffle=False)
    assert nb == 1
    return next(it)


def check_round_trip(out, meshes, poses, labels, records):
    """the reader's batch of the converted tree against the scene and the renderer's labels / records of it"""
    from PIL import Image

    b = read_back(out)
    K = np.array([[BOP_CAM[0], 0, BOP_CAM[2]], [0, BOP_CAM[1], BOP_CAM[3]], [0, 0, 1]])
    assert np.allclose(b["cam_mat"].numpy(), K[None].repeat(2, 0), rtol=1e-6)
    relabel = np.zeros(256, np.uint8)
    relabel[1], relabel[5] = 1, 2
    for i in range(2):
        seg = np.array(Image.open(out / "test" / "000002" / "rgb" / ("%06d.seg.png" % i)))
        assert np.array_equal(seg, labels[i])
        assert np.array_equal(b["filtered_seg"][i, ..., 0].numpy(), relabel[labels[i]])
        assert np.array_equal(np.array(Image.open(out / "test" / "000002" / "rgb" / ("%06d.png" % i))),
                              np.array(Image.open(out.parent / "bop" / "test" / "000002" / "rgb" / ("%06d.png" % i))))
        for k, (obj, P) in enumerate(poses[i]):
            o = NAMES.index("obj_%06d" % obj)
            assert np.allclose(b["poses_gt"][i, o, 0].numpy(), P, rtol=1e-5, atol=1e-3)
            kp = keypoints_of(OBJECTS[obj])
            assert np.allclose(b["keypoints3d"][i, o, 0].numpy(), kp, atol=1e-4)
            uv, _ = BC.project(kp, K, P)
            assert np.allclose(b["target_vert"][i, o, 0].numpy(), uv[:, ::-1], atol=1e-3)
            assert int(b["pixel_gt_count"][i, o, 0, 0]) == int(records[i, k, 0]) > 0
    assert (labels > 0).sum() > 500 and (records[..., 0] > records[..., 1]).any()   # something is occluded


def scene_frames(poses):
    return [dict(cam=BOP_CAM, instances=[(o, o, P) for o, P in poses[i]]) for i in range(2)]


def test_round_trip_rendered_masks_into_the_reader(tmp_path):
    meshes, poses = write_bop_tree(tmp_path / "bop")
    BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "out"), settings_for(), model_folder="models", model_folder_out="models", image_folder="test")
    labels, records = BC.MaskRenderer(None, meshes).render_host(scene_frames(poses), H, W, 100.0, 2000.0, 0.5)
    check_round_trip(tmp_path / "out", meshes, poses, labels, records)
    data = json.load(open(tmp_path / "out" / "test" / "000002" / "rgb" / "000000.json"))
    for k, obj in enumerate(data["objects"]):
        r = records[0, k].tolist()
        assert obj["px_count_all"] == r[0] and obj["px_count_visib"] == r[1] and "px_count_valid" not in obj
        assert obj["visibility"] == r[1] / r[0] and 0 < obj["visibility"] <= 1
        assert obj["bounding_box"] == {"top_left": r[2:4], "bottom_right": [r[2] + r[4], r[3] + r[5]]}
        assert obj["bounding_box_visible"] == {"top_left": r[6:8], "bottom_right": [r[6] + r[8], r[7] + r[9]]}
    settings = json.load(open(tmp_path / "out" / "test" / "000002" / "rgb" / "_object_settings.json"))
    assert settings["exported_object_classes"] == NAMES and [o["segmentation_class_id"] for o in settings["exported_objects"]] == [1, 5]


def test_round_trip_reused_masks_into_the_reader(tmp_path):
    """mask = "reuse" against hand-made mask_visib PNGs (rectangles, the later instance over the earlier); gt_info = "render" still fills the counts"""
    hand = np.zeros((2, H, W), np.uint8)
    hand[0, 20:60, 30:70], hand[0, 40:80, 50:100] = 1, 5
    hand[1, 10:50, 20:60], hand[1, 50:90, 80:120] = 5, 1
    meshes, poses = write_bop_tree(tmp_path / "bop", with_masks=hand)
    BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "out"), settings_for(mask="reuse"), model_folder="models", model_folder_out="models",
                     image_folder="test")
    _, records = BC.MaskRenderer(None, meshes).render_host(scene_frames(poses), H, W, 100.0, 2000.0, 0.5)
    check_round_trip(tmp_path / "out", meshes, poses, hand, records)


def test_file_gt_info_without_a_file_keeps_the_reference_defaults(tmp_path):
    write_bop_tree(tmp_path / "bop")
    BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "out"), settings_for(gt_info="file", mask="none"), model_folder="models",
                     model_folder_out="models", image_folder="test")
    rgb = tmp_path / "out" / "test" / "000002" / "rgb"
    obj = json.load(open(rgb / "000001.json"))["objects"][0]
    assert obj["visibility"] == 1 and "px_count_all" not in obj and not os.path.exists(rgb / "000001.seg.png")


def test_near_plane_drops_are_reported_by_frame_and_object(tmp_path, capsys):
    """near = 480 cuts into object 1 of frame 0 (centre at 500, 40 mm deep): one warning line for that frame and object, none for the others"""
    write_bop_tree(tmp_path / "bop")
    BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "out"), settings_for(near=480.0), model_folder="models", model_folder_out="models",
                     image_folder="test")
    warnings = [line for line in capsys.readouterr().out.splitlines() if line.startswith("warning")]
    assert len(warnings) == 2 and "000000.png: object 1 (instance 0)" in warnings[0] and "000001.png: object 5 (instance 0)" in warnings[1]
    data = json.load(open(tmp_path / "out" / "test" / "000002" / "rgb" / "000000.json"))
    assert data["objects"][0]["px_count_all"] > 0   # the triangles behind the plane are still drawn


def test_refusals(tmp_path, monkeypatch):
    write_bop_tree(tmp_path / "bop")
    with pytest.raises(NotImplementedError, match="draw_debug_image"):
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o1"), settings_for(draw_debug_image=True), image_folder="test")
    with pytest.raises(ValueError, match="gt_info"):
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o2"), settings_for(gt_info="guess"), image_folder="test")
    import torch

    with monkeypatch.context() as m:   # mask = "render" without a GPU is an error, never the twin
        m.setattr(torch.cuda, "is_available", lambda: False)
        with pytest.raises(CasaposeHipError, match="renderer"):
            BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o5"), settings_for(renderer="device"), image_folder="test")
    gt_path = tmp_path / "bop" / "test" / "000002" / "scene_gt.json"
    gt = json.load(open(gt_path))
    gt["1"][0]["obj_id"] = 256
    json.dump(gt, open(gt_path, "w"))
    with pytest.raises(ValueError, match="obj_id 256"):
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / "o3"), settings_for(mask="reuse", gt_info="file"), image_folder="test")
    write_bop_tree(tmp_path / "faceless", faces=False)
    with pytest.raises(ValueError, match="obj_000001.ply has no faces"):
        BC.generate_data(str(tmp_path / "faceless"), str(tmp_path / "o4"), settings_for(), image_folder="test")
    with pytest.raises(ValueError, match="label 300"):
        renderer_for([ellipsoid(1, (1, 1, 1))]).render_host([dict(cam=CAM, instances=[(0, 300, np.eye(4)[:3])])], 8, 8, 1.0, 10.0)


def test_library_refuses_bad_arguments(hip_lib):
    a, label, records, planes = np.zeros(64, np.float64), np.ones(16, np.uint8), np.ones(11, np.int32), np.zeros(16, np.uint32)
    p = a.ctypes.data   # every input reads zeros: no vertices, no faces, no instances
    ok = [p, p, 4, p, p, 4, 1, p, p, p, p, p, 1, 1, 4, 4, 1.0, 10.0, 0.5, label.ctypes.data, records.ctypes.data, planes.ctypes.data, 64]
    assert hip_lib.cp_render_masks_host_u8(*ok) == 0 and (label == 0).all() and records.tolist() == [0, 0] + [-1] * 8 + [0]
    for at, bad, word in ((12, 0, b"frames"), (13, 257, b"instances_max"), (14, 16385, b"H and W"), (16, 0.0, b"near"), (18, 1.5, b"sample_offset"),
                          (22, 63, b"workspace"), (0, None, b"null")):
        args = list(ok)
        args[at] = bad
        assert hip_lib.cp_render_masks_host_u8(*args) == -1 and word in hip_lib.cp_last_error(), word
        assert hip_lib.cp_render_masks_u8(*args, None) == -1 and word in hip_lib.cp_last_error(), word
    assert hip_lib.cp_render_masks_workspace_bytes(3, 8, 480, 640) == 3 * 8 * 480 * 640 * 4
    assert hip_lib.cp_render_masks_workspace_bytes(0, 8, 480, 640) == 0 and hip_lib.cp_render_masks_workspace_bytes(1, 257, 4, 4) == 0


def test_command_line(tmp_path):
    meshes, poses = write_bop_tree(tmp_path / "bop")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "util_scripts", "dataset_converter.py"), "--dataset_path", str(tmp_path / "bop"),
                        "--dataset_path_out", str(tmp_path / "out"), "--image_folder", "test", "--width", str(W), "--height", str(H), "--mask", "render",
                        "--gt_info", "render", "--renderer", "host", "--copy_meshes"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    labels, records = BC.MaskRenderer(None, meshes).render_host(scene_frames(poses), H, W, 100.0, 2000.0, 0.5)
    check_round_trip(tmp_path / "out", meshes, poses, labels, records)
