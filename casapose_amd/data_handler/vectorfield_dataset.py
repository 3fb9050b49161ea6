"""NDDS / converted-BOP dataset reader producing the batch tuple of the training and evaluation steps -- the counterpart of
VectorfieldDataset (casapose/data_handler/vectorfield_dataset.py:24-180,291-509,545-762,764-1013,1047-1074) without
TensorFlow: PIL for images, NumPy for geometry, plain Python iteration instead of tf.data.

On-disk layout read (the reference's, :682-746):
    <root>/<scene...>/NNNNNN.png|bmp|jpg   colour image            NNNNNN.seg.png  uint8 segmentation-class ids
    <root>/<scene...>/NNNNNN.json           objects[]: class, visibility, px_count_all, keypoints_2d [[x,y]...], keypoints_3d,
                                            quaternion_xyzw, location
    <root>/<scene...>/_object_settings.json exported_objects[]: class, segmentation_class_id, fixed_model_transform (4x4, stored transposed)
    <root>/<scene...>/_camera_settings.json camera_settings[0].intrinsic_settings {fx, fy, cx, cy}
    <meshes>/<obj>/<obj>.ply|obj , <obj>_keypoints.ply , <meshes>/models_info.json {<obj>: {diameter}}

Per image (apply_preprocessing, :291-509): crop of height round(H*crop_factor) and the output aspect ratio (random or centred),
optional random rotation / translation about the image centre, resize to `imagesize`; 2-D keypoints follow the same map and
come out in (y,x); poses from quaternion_xyzw + location; offsets = [h_crop, w_crop, crop_h, crop_w, dx, dy, angle, scale, W, H];
segmentation ids are re-labelled to 1..len(objectsofinterest) in the order of `objectsofinterest` (:748-762, :996-1008).
Batches are dicts with the field names used by casapose_amd.training (img_batch indices of train_casapose.py:496-507):
img[0] target_seg[1] target_vert[3] keypoints3d[4] cam_mat[5] diameters[6] offsets[7] filtered_seg[8] poses_gt[10]
pixel_gt_count[11] image_id[12].

Not carried over: hue / saturation jitter of the non-imgaug branch; brightness / contrast jitter and the additive noise of
image_augmentation (:259-272) are.  use_imgaug (the reference's imgaug `seq`, augmentation_model.py:43-110) runs on the device path of
generate_dataset only (device_pipeline.py, augment.py); the host path refuses it.  Only one instance per object is read, like the reference
(`max_count = 1`, :795).  Parity with the reference's loader is untested here (no dataset on this machine): the round trip
against write_ndds_scene() below pins the conventions as read from the reference's code.
"""
from __future__ import annotations

import glob
import json
import math
import os
import weakref
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------
# small geometry / file helpers
# ------------------------------------------------------------------------------------------------
def quaternion_matrix(quaternion_xyzw, translation=None, wxyz_input=False) -> np.ndarray:
    """rotation (3x3) or pose (3x4) from a quaternion (utils/geometry_utils.py:144-181)."""
    q = np.array(quaternion_xyzw, dtype=np.float64)
    if not wxyz_input:
        q = np.array([q[3], q[0], q[1], q[2]])
    n = float(q @ q)
    if n < 1e-4:
        return np.identity(4)
    q = q * math.sqrt(2.0 / n)
    q = np.outer(q, q)
    R = np.array([[1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0]],
                  [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0]],
                  [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2]]])
    if translation is None:
        return R
    return np.concatenate([R, np.asarray(translation, np.float64).reshape(3, 1)], axis=1)


def matrix_to_quaternion_xyzw(R: np.ndarray) -> np.ndarray:
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        w, x, y, z = 0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        v = [0.0, 0.0, 0.0]
        v[i] = 0.25 * s
        v[j] = (R[j, i] + R[i, j]) / s
        v[k] = (R[k, i] + R[i, k]) / s
        w = (R[k, j] - R[j, k]) / s
        x, y, z = v
    return np.array([x, y, z, w])


def get_rotation_matrix_2D(center, angle_deg) -> np.ndarray:
    a_, b_ = math.cos(angle_deg * math.pi / 180), math.sin(angle_deg * math.pi / 180)
    return np.array([[a_, b_, (1 - a_) * center[0] - b_ * center[1]], [-b_, a_, b_ * center[0] + (1 - a_) * center[1]]], np.float64)


def transform_points(points, transform) -> np.ndarray:
    p = np.c_[np.asarray(points, np.float64), np.ones(len(points))]
    return (np.asarray(transform, np.float64) @ p.T).T[:, :3]


def read_vertices(path: str) -> np.ndarray:
    """Vertices of a .ply (ascii or binary_little_endian, float/double x y z first among the vertex properties) or .obj file."""
    if path.lower().endswith(".obj"):
        v = [[float(t) for t in line.split()[1:4]] for line in open(path) if line.startswith("v ")]
        return np.asarray(v, np.float64)
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, count, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                props.append((tok[1], tok[-1]))
            elif tok[0] == "end_header":
                break
        names = [p[1] for p in props]
        ix = [names.index(a) for a in ("x", "y", "z")]
        if fmt == "ascii":
            rows = [f.readline().split() for _ in range(count)]
            return np.asarray([[float(r[i]) for i in ix] for r in rows], np.float64)
        if fmt != "binary_little_endian":
            raise ValueError("%s: unsupported PLY format %s" % (path, fmt))
        types = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int8": "i1",
                 "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}
        dt = np.dtype([(n, types[t]) for t, n in props])
        data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        return np.stack([data["x"], data["y"], data["z"]], axis=1).astype(np.float64)


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int8": "i1",
              "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def read_vertex_colors(path: str):
    """Per-vertex colours uint8 [V, 3] of a .ply whose vertex element (the first element, as read_vertices expects it) has uchar `red`, `green`
    and `blue` properties, ascii or binary_little_endian.  A PLY without them, and an .obj file, give None."""
    if path.lower().endswith(".obj"):
        return None
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, count, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                props.append((tok[1], tok[-1]))
            elif tok[0] == "end_header":
                break
        names = [p[1] for p in props]
        if not all(c in names and props[names.index(c)][0] in ("uchar", "uint8") for c in ("red", "green", "blue")):
            return None
        if fmt == "ascii":
            ix = [names.index(c) for c in ("red", "green", "blue")]
            rows = [f.readline().split() for _ in range(count)]
            return np.asarray([[int(r[i]) for i in ix] for r in rows], np.uint8).reshape(-1, 3)
        if fmt != "binary_little_endian":
            raise ValueError("%s: unsupported PLY format %s" % (path, fmt))
        for t, _ in props:
            if t not in _PLY_TYPES:
                raise ValueError("%s: unsupported PLY property type %s" % (path, t))
        dt = np.dtype([(n, _PLY_TYPES[t]) for t, n in props])
        data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        return np.stack([data["red"], data["green"], data["blue"]], axis=1).astype(np.uint8)


def _fan(poly) -> List[Tuple[int, int, int]]:
    return [(poly[0], poly[k], poly[k + 1]) for k in range(1, len(poly) - 1)]


def read_faces(path: str) -> np.ndarray:
    """Triangles [T, 3] int32 of a .ply (ascii or binary_little_endian; `element face` with `property list uchar int|uint vertex_indices` or
    `vertex_index`) or .obj file (`f` lines, the vertex index before any `/`, 1-based or negative).  Polygons are fan-triangulated; the other
    properties of a face and every other element are skipped by size.  A file without faces gives [0, 3]."""
    if path.lower().endswith(".obj"):
        tris, vertices = [], 0
        for line in open(path):
            tok = line.split()
            if tok and tok[0] == "v":
                vertices += 1
            elif tok and tok[0] == "f":
                idx = [int(t.split("/")[0]) for t in tok[1:]]
                tris += _fan([i - 1 if i > 0 else vertices + i for i in idx])
        return np.asarray(tris, np.int32).reshape(-1, 3)
    if not path.lower().endswith(".ply"):
        raise ValueError("%s: read_faces reads .ply and .obj files" % path)
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elements = None, []   # elements: [name, count, [(kind, ...)]] in file order
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property" and elements:
                if tok[1] == "list":
                    elements[-1][2].append(("list", tok[2], tok[3], tok[4]))
                else:
                    elements[-1][2].append(("scalar", tok[1], tok[2]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError("%s: unsupported PLY format %s" % (path, fmt))
        for _, _, props in elements:
            for p in props:
                for t in p[1:-1]:
                    if t not in _PLY_TYPES:
                        raise ValueError("%s: unsupported PLY property type %s" % (path, t))
        tris: List[Tuple[int, int, int]] = []
        for name, count, props in elements:
            face = name == "face"
            if face:
                lists = [p for p in props if p[0] == "list" and p[3] in ("vertex_indices", "vertex_index")]
                if len(lists) != 1 or lists[0][1] not in ("uchar", "uint8") or lists[0][2] not in ("int", "int32", "uint", "uint32"):
                    raise ValueError("%s: element face needs one `property list uchar int|uint vertex_indices|vertex_index`" % path)
            if fmt == "ascii":
                for _ in range(count):
                    row = f.readline().split()
                    if not face:
                        continue
                    at = 0
                    for p in props:
                        if p[0] == "scalar":
                            at += 1
                            continue
                        n = int(row[at])
                        if p[3] in ("vertex_indices", "vertex_index"):
                            tris += _fan([int(t) for t in row[at + 1:at + 1 + n]])
                        at += 1 + n
                continue
            if all(p[0] == "scalar" for p in props):   # fixed-size rows: skipped (or, never for a face, read) in one step
                f.seek(count * sum(np.dtype(_PLY_TYPES[p[1]]).itemsize for p in props), 1)
                continue
            if face and sum(p[0] == "list" for p in props) == 1:   # all triangles (the common case): one structured read
                dt = np.dtype([("f%d" % i, _PLY_TYPES[p[1]]) if p[0] == "scalar" else ("tri", [("n", _PLY_TYPES[p[1]]), ("i", _PLY_TYPES[p[2]], (3,))])
                               for i, p in enumerate(props)])
                start = f.tell()
                raw = f.read(count * dt.itemsize)
                if len(raw) == count * dt.itemsize:
                    rows = np.frombuffer(raw, dt)["tri"]
                    if (rows["n"] == 3).all():
                        tris += [tuple(r) for r in rows["i"].astype(np.int64).tolist()]
                        continue
                f.seek(start)
            for _ in range(count):
                for p in props:
                    if p[0] == "scalar":
                        f.seek(np.dtype(_PLY_TYPES[p[1]]).itemsize, 1)
                        continue
                    ct, it = np.dtype(_PLY_TYPES[p[1]]), np.dtype(_PLY_TYPES[p[2]])
                    n = int(np.frombuffer(f.read(ct.itemsize), ct)[0])
                    data = f.read(n * it.itemsize)
                    if face and p[3] in ("vertex_indices", "vertex_index"):
                        tris += _fan(np.frombuffer(data, it).astype(np.int64).tolist())
        return np.asarray(tris, np.int32).reshape(-1, 3)


def _bbox_corners(v: np.ndarray) -> np.ndarray:
    lo, hi = v.min(0), v.max(0)
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)


def _shared_random_seed() -> int:
    """A fresh random seed that is the SAME on every replica: rank 0 draws it and broadcasts it when a process group exists."""
    seed = int(np.random.SeedSequence().entropy % (1 << 31))
    try:
        import torch.distributed as dist
    except ImportError:  # no torch.distributed in this interpreter: a single process keeps its own draw
        return seed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        # a failing collective must NOT be swallowed: ranks that kept their own seeds would draw different epoch permutations and their
        # shard slices would no longer partition the global batch (and the other ranks would hang in the broadcast)
        box = [seed]
        dist.broadcast_object_list(box, src=0)
        seed = int(box[0])
    return seed


def load_split(path: str, ratio: float, rng: np.random.Generator) -> List[int]:
    """_split_settings.json (utils/dataset_utils.py:462-497): reuse a stored split with the same ratio, else draw and store one."""
    fp = os.path.join(path, "_split_settings.json")
    if os.path.isfile(fp):
        info = json.load(open(fp))
        if info["split"][0]["ratio"] == ratio:
            return info["split"][0]["values"]
    n = len(glob.glob(path + "/*seg.png"))
    split = np.zeros(n, int)
    split[: int(n * ratio)] = 1
    rng.shuffle(split)
    json.dump({"split": [{"ratio": ratio, "values": split.tolist()}]}, open(fp, "w"))
    return split.tolist()


# ------------------------------------------------------------------------------------------------
class VectorfieldDataset:
    last_instance = None   # weak reference to the dataset built last: names the meshes for pose_estimation/mask_refine.py (CASAPOSE_MASK_REFINE=1)

    def __init__(self, root, path_meshes, no_points=9, color_input=False, normal=(0.5, 0.5), test=False, objectsofinterest=(), save=False, noise=2,
                 data_size=None, random_translation=(25.0, 25.0), random_rotation=15.0, random_crop=True, contrast=0.2, brightness=0.2, hue=0.05,
                 saturation=0.2, use_train_split=False, use_validation_split=False, train_validation_split=0.9, output_folder="", use_imgaug=False,
                 visibility_filter=False, separated_vectorfields=False, wxyz_quaterion_input=False, path_filter_root=None, seed: int = 0):
        if use_imgaug and not color_input:
            raise NotImplementedError("use_imgaug with color_input off (the reference's seq_grayscale) is not part of this build")
        if separated_vectorfields:
            raise NotImplementedError("separated vector fields (modelname pvnet) are not part of this build")
        # `meshes:<folder>[:N]` in place of a tree: the scenes are rendered from the meshes (mesh_scene.py) and this object only hands the
        # caller's image size and object count on to a MeshSceneDataset.  test_casapose.py's folder branch builds this class, so the script
        # takes `--datatest meshes:` as it stands; path_meshes and the augmentation arguments do not apply to such a source.
        self.mesh_spec = str(root) if str(root).startswith("meshes:") else None
        self._mesh_scenes = None
        if self.mesh_spec is not None:
            self.no_points, self.objectsofinterest, self.random_crop, self.use_imgaug = no_points, list(objectsofinterest), random_crop, False
            self.seed = int(_shared_random_seed() if seed is None else seed)
            return
        self.path_meshes, self.no_points, self.color_input, self.normal = path_meshes, no_points, color_input, list(normal)
        self.objectsofinterest = list(objectsofinterest)
        self.noise, self.random_translation, self.random_rotation, self.random_crop = noise, random_translation, random_rotation, random_crop
        self.contrast, self.brightness = contrast, brightness
        self.use_imgaug = bool(use_imgaug)
        self.use_train_split, self.use_validation_split, self.train_validation_split = use_train_split, use_validation_split, train_validation_split
        self.visibility_filter, self.wxyz_quaterion_input = visibility_filter, wxyz_quaterion_input
        if seed is None:
            seed = _shared_random_seed()   # the reference shuffles / augments differently on every run; all replicas must still agree on ONE stream
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)   # re-seeded per image in generate_dataset(): the augmentation of image i of epoch e does
        #                                               not depend on the number of replicas or on which of them reads it
        self.order_rng = np.random.default_rng([self.seed, 1])  # epoch permutations only: identical on every replica
        self.meshes = self.load_meshes(path_meshes)
        self.last_offsets: Optional[np.ndarray] = None   # the offsets of the sample drawn last (draw_geometry)
        VectorfieldDataset.last_instance = weakref.ref(self)
        self.imgs: List[Tuple[str, str, str, str, str]] = []
        self.class_labels: Dict[str, Dict[str, int]] = {}
        self.fixed_transformations: Dict[str, Dict[str, np.ndarray]] = {}
        self.camera_data: Dict[str, np.ndarray] = {}
        for name in sorted(os.listdir(str(root))):
            if path_filter_root is None or name in path_filter_root:
                self._explore(os.path.join(root, name))
        if not self.imgs:
            raise FileNotFoundError("no <name>.png + <name>.seg.png + <name>.json triples under %s" % root)

    def __len__(self):
        return len(self.mesh_scenes()) if self.mesh_spec is not None else len(self.imgs)

    def mesh_scenes(self, imagesize=(448, 448), no_objects=None):
        """the MeshSceneDataset behind a `meshes:<folder>[:N]` root, built on first use with the image size and object count known then (N
        defaults to 32, test_casapose.py's default for `synthetic`)"""
        if self._mesh_scenes is None:
            from .mesh_scene import MeshSceneDataset, parse_spec

            folder, n = parse_spec(self.mesh_spec)
            self._mesh_scenes = MeshSceneDataset(folder, no_objects or len(self.objectsofinterest), tuple(imagesize), self.no_points,
                                                 length=32 if n is None else n, seed=self.seed, random_crop=self.random_crop)
        return self._mesh_scenes

    # ---- discovery ---------------------------------------------------------------------------------
    def load_meshes(self, path) -> Dict[str, dict]:
        meshes = {}
        info_file = os.path.join(path, "models_info.json")
        info = json.load(open(info_file)) if os.path.isfile(info_file) else {}
        for name in sorted(o for o in os.listdir(path) if os.path.isdir(os.path.join(path, o))):
            model = os.path.join(path, name, name + ".obj")
            if not os.path.exists(model):
                model = os.path.join(path, name, name + ".ply")
            kp = os.path.join(path, name, name + "_keypoints.ply")
            if os.path.isfile(model) and os.path.isfile(kp):
                v = read_vertices(model)
                diam = info.get(name, {}).get("diameter")
                if diam is None:  # largest vertex distance (:632-640)
                    sub = v if len(v) <= 4000 else v[np.random.default_rng(0).choice(len(v), 4000, replace=False)]
                    G = sub @ sub.T
                    d2 = np.diag(G)[:, None] + np.diag(G)[None, :] - 2 * G
                    diam = float(np.sqrt(d2.max()))
                meshes[name] = {"keypoints": read_vertices(kp), "vertices": v, "volume": _bbox_corners(v), "diameter": float(diam)}
        return meshes

    def _explore(self, path):
        if not os.path.isdir(path):
            return
        sub = [os.path.join(path, o) for o in sorted(os.listdir(path)) if os.path.isdir(os.path.join(path, o))]
        if sub:
            for s in sub:
                self._explore(s)
            return
        files = sorted(glob.glob(path + "/*seg.png"))
        if not files:
            return
        if self.use_train_split or self.use_validation_split:
            split = np.array(load_split(path, self.train_validation_split, self.rng), bool)
            files = [f for f, s in zip(files, split if self.use_train_split else ~split) if s]
        if path not in self.class_labels:
            data = json.load(open(os.path.join(path, "_object_settings.json")))
            self.class_labels[path] = {o["class"]: o["segmentation_class_id"] for o in data["exported_objects"]}
            self.fixed_transformations[path] = {o["class"]: np.array(o["fixed_model_transform"], np.float32).T for o in data["exported_objects"]}
            cam = json.load(open(os.path.join(path, "_camera_settings.json")))["camera_settings"][0]["intrinsic_settings"]
            self.camera_data[path] = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], np.float64)
        for seg in files:
            for ext in ("png", "bmp", "jpg"):
                img = seg.replace("seg.png", ext)
                js = seg.replace("seg.png", "json")
                if os.path.exists(img) and os.path.exists(js):
                    self.imgs.append((img, os.path.basename(img), js, seg, path))
                    break

    def load_json_minimal(self, path) -> dict:
        data = json.load(open(path))
        out = {"keypoints2d": [], "objectClasses": {}, "poses_quaternions": [], "poses_loc": [], "px_count_all": []}
        idx = 0
        for info in data["objects"]:
            if self.visibility_filter and not info["visibility"] > 0.10:
                continue
            out["objectClasses"].setdefault(info["class"], []).append(idx)
            out["px_count_all"].append(int(info.get("px_count_all", 0)))
            out["keypoints2d"].append([(p[0], p[1]) for p in info["keypoints_2d"]])
            out["poses_quaternions"].append(np.array(info["quaternion_xyzw"], np.float32))
            out["poses_loc"].append(np.array(info["location"], np.float32))
            idx += 1
        return out

    # ---- one sample ----------------------------------------------------------------------------------
    def draw_geometry(self, width, height, imagesize, cropratio) -> dict:
        """The crop / translation / rotation draws of one image (in this order, from self.rng) and the maps they define."""
        crop_h = round(float(height) * cropratio)
        crop_w = crop_h * (float(imagesize[1]) / float(imagesize[0]))
        out_h, out_w = int(crop_h), int(crop_w)
        scale = imagesize[0] / out_h
        if self.random_crop:
            w_crop = int(self.rng.integers(0, width - out_w + 1))
            h_crop = int(self.rng.integers(0, height - out_h + 1))
        else:
            w_crop, h_crop = int((width - out_w) / 2), int((height - out_h) / 2)
        dx = round(self.rng.normal(0, 2) * float(self.random_translation[0]))
        dy = round(self.rng.normal(0, 2) * float(self.random_translation[1]))
        angle = round(self.rng.normal(0, 1) * float(self.random_rotation))
        offsets = np.array([h_crop, w_crop, out_h, out_w, dx, dy, angle, scale, width, height], np.float32)
        self.last_offsets = offsets
        tm = np.array([[1, 0, dx], [0, 1, dy]], np.float64)
        rm = get_rotation_matrix_2D((width / 2, height / 2), angle)
        # output -> input map of the image warp (tfa.image.transform convention == PIL AFFINE)
        ar, at = np.identity(3), np.identity(3)
        ar[:2] = get_rotation_matrix_2D((width / 2, height / 2), -angle)
        at[:2] = [[1, 0, -dx], [0, 1, -dy]]
        affine = (ar @ at).flatten()[:6]
        return dict(out_h=out_h, out_w=out_w, scale=scale, w_crop=w_crop, h_crop=h_crop, dx=dx, dy=dy, angle=angle, offsets=offsets, tm=tm, rm=rm,
                    affine=affine, width=width, height=height)

    def annotations(self, data, path_raw, geo) -> Tuple[dict, Dict[int, int]]:
        """Keypoints / poses / counts of one image under the drawn geometry, and the segmentation id -> label map (1..oc in the order of
        objectsofinterest; later objects win, like the reference's successive masks)."""
        labels, fixed, cam = self.class_labels[path_raw], self.fixed_transformations[path_raw], self.camera_data[path_raw]
        oc, kp = len(self.objectsofinterest), self.no_points
        kp2 = np.full((oc, 1, kp, 2), -1000.0, np.float32)
        kp3 = np.zeros((oc, 1, kp, 3), np.float32)
        cub = np.zeros((oc, 1, 8, 3), np.float32)
        poses = np.zeros((oc, 1, 3, 4), np.float32)
        pxc = np.zeros((oc, 1, 1), np.float32)
        diam = np.full((oc, 1, 1), -1.0, np.float32)
        remap: Dict[int, int] = {}
        rm, tm, scale, w_crop, h_crop = geo["rm"], geo["tm"], geo["scale"], geo["w_crop"], geo["h_crop"]
        for o, obj in enumerate(self.objectsofinterest):
            mesh = self.meshes[obj]
            if obj in fixed:
                kp3[o, 0] = transform_points(mesh["keypoints"], fixed[obj])[:kp]
                cub[o, 0] = transform_points(mesh["volume"], fixed[obj])
            else:
                kp3[o, 0], cub[o, 0] = np.asarray(mesh["keypoints"])[:kp], mesh["volume"]
            for cls, ids in data["objectClasses"].items():
                if obj in cls:  # substring match like the reference (:379)
                    i = ids[0]
                    pts = np.asarray(data["keypoints2d"][i], np.float64)[:kp]
                    h1 = np.c_[pts, np.ones(len(pts))]
                    r3, t3 = np.identity(3), np.identity(3)
                    r3[:2], t3[:2] = rm, tm
                    p = (t3 @ (r3 @ h1.T))[:2].T - np.array([w_crop, h_crop])      # reproject (geometry_utils.py:7-19)
                    kp2[o, 0] = (p * scale)[:, ::-1]                                # stored (y,x) (:483)
                    poses[o, 0] = quaternion_matrix(data["poses_quaternions"][i], data["poses_loc"][i], wxyz_input=self.wxyz_quaterion_input)
                    pxc[o, 0, 0] = int(float(data["px_count_all"][i]) * scale + 0.5)
                    diam[o, 0, 0] = mesh["diameter"] * (np.linalg.norm(fixed[obj][:, 0]) if obj in fixed else 1.0)
                    remap[int(labels[obj])] = o + 1
                    break
        p = os.path.normpath(path_raw.replace("\\", "/")).split(os.sep)
        name = os.path.basename(data.get("_img_path", ""))
        return dict(target_vert=kp2, keypoints3d=kp3, cam_mat=cam.astype(np.float32), diameters=diam, offsets=geo["offsets"], cuboid3d=cub,
                    poses_gt=poses, pixel_gt_count=pxc, image_id=p[-2] + "_" + p[-1] + "_" + os.path.splitext(name)[0]), remap

    def draw_photometric(self) -> Tuple[float, float, float]:
        """(brightness offset, contrast factor, noise sigma) of image_augmentation (:259-272), drawn in this order; 0 / 1 / 0 when off."""
        b = float(self.rng.uniform(-self.brightness, self.brightness)) if self.brightness else 0.0
        f = float(self.rng.uniform(1 - self.contrast, 1 + self.contrast)) if self.contrast else 1.0
        sigma = float(self.rng.uniform(0, self.noise)) if self.noise else 0.0
        return b, f, sigma

    # ---- one sample ----------------------------------------------------------------------------------
    def apply_preprocessing(self, item, imagesize, cropratio) -> dict:
        from PIL import Image

        img_path, name, js, seg_path, path_raw = item
        data = self.load_json_minimal(js)
        data["_img_path"] = name
        img = Image.open(img_path)
        img = img.convert("RGB") if self.color_input else img.convert("L")
        seg = Image.open(seg_path).convert("L")
        width, height = img.size
        geo = self.draw_geometry(width, height, imagesize, cropratio)
        out_h, out_w, w_crop, h_crop, affine = geo["out_h"], geo["out_w"], geo["w_crop"], geo["h_crop"], geo["affine"]
        if geo["dx"] or geo["dy"] or geo["angle"]:
            img = img.transform(img.size, Image.AFFINE, data=tuple(affine), resample=Image.BILINEAR)
            seg = seg.transform(seg.size, Image.AFFINE, data=tuple(affine), resample=Image.NEAREST)
        box = (w_crop, h_crop, w_crop + out_w, h_crop + out_h)
        img = img.crop(box).resize((imagesize[1], imagesize[0]), Image.BILINEAR)
        seg = seg.crop(box).resize((imagesize[1], imagesize[0]), Image.NEAREST)
        img = np.asarray(img, np.float32)
        img = img[..., None] if img.ndim == 2 else img
        seg = np.asarray(seg, np.uint8)
        ann, remap = self.annotations(data, path_raw, geo)
        new_seg = np.zeros_like(seg)
        for sid, lab in remap.items():
            new_seg[seg == sid] = lab
        # photometric part of image_augmentation (:259-272)
        if self.brightness:
            img = img + self.rng.uniform(-self.brightness, self.brightness)
        if self.contrast:
            f = self.rng.uniform(1 - self.contrast, 1 + self.contrast)
            m = img.mean(axis=(0, 1), keepdims=True)
            img = (img - m) * f + m
        img = ((img / 255.0) - self.normal[0]) / self.normal[1]
        if self.noise:
            img = img + self.rng.normal(0.0, self.rng.uniform(0, self.noise), img.shape)
        img = np.clip(img, -1, 1).astype(np.float32)
        if img.shape[2] == 1:
            img = np.repeat(img, 3, axis=2)
        return dict(img=img, label=new_seg, **ann)

    # ---- batches ---------------------------------------------------------------------------------------
    def generate_dataset(self, batchsize, epochs, prefetch=0, imagesize=(448, 448), cropratio=1.0, worker=1, no_objects=None, shuffle=True,
                         mirrored_strategy=None, shard: Tuple[int, int] = (0, 1), device=None) -> Tuple[Iterator[Dict[str, torch.Tensor]], int]:
        """`batchsize` is the GLOBAL batch (vectorfield_dataset.py:923; `experimental_distribute_dataset` splits it, :1000-1002).  Here every
        replica owns a process: shard = (rank, world) makes it read, decode and augment only its contiguous slice of each global batch
        (the epoch permutation comes from a generator of its own, seeded alike on all replicas, so the slices partition the batch).
        device: None = this host path; a GPU = the device path (device_pipeline.py: decode on `worker` threads, every per-pixel step on the
        GPU, up to max(prefetch, 1) batches in flight), the only path that runs use_imgaug."""
        from ..parallel import shard_range

        if self.mesh_spec is not None:
            return self.mesh_scenes(imagesize, no_objects).generate_dataset(batchsize, epochs, prefetch, shard=shard, device=device)
        if device is not None:
            from .device_pipeline import device_batches

            return device_batches(self, device, batchsize, epochs, prefetch, imagesize, cropratio, worker, shard, shuffle)
        if self.use_imgaug:
            raise ValueError("use_imgaug runs on the device input pipeline only: call generate_dataset(..., device=<GPU>)")

        data_size = len(self.imgs) - (len(self.imgs) % batchsize)
        epoch_batches = data_size // batchsize
        oc = len(self.objectsofinterest)
        begin, end = shard_range(batchsize, shard[0], shard[1])

        def sample(epoch, i):
            self.rng = np.random.default_rng([self.seed, 2, epoch, int(i)])   # crop / rotation / colour draws of THIS image in THIS epoch
            return self.apply_preprocessing(self.imgs[i], imagesize, cropratio)

        def it():
            for epoch in range(max(int(epochs), 1)):
                order = self.order_rng.permutation(data_size) if shuffle else np.arange(data_size)
                for b in range(epoch_batches):
                    items = [sample(epoch, i) for i in order[b * batchsize + begin:b * batchsize + end]]
                    lab = np.stack([x["label"] for x in items])
                    st = lambda k: torch.from_numpy(np.stack([x[k] for x in items]))  # noqa: E731
                    yield dict(img=st("img"), target_seg=torch.from_numpy(np.eye(oc + 1, dtype=np.float32)[lab]), target_vert=st("target_vert"),
                               keypoints3d=st("keypoints3d"), cam_mat=st("cam_mat"), diameters=st("diameters"), offsets=st("offsets"),
                               filtered_seg=torch.from_numpy(lab[..., None].astype(np.int32)), cuboid3d=st("cuboid3d"), poses_gt=st("poses_gt"),
                               pixel_gt_count=st("pixel_gt_count"), image_id=[x["image_id"] for x in items])

        return it(), epoch_batches

    def generate_object_vertex_array(self):
        """(vertex_array [oc, Vmax, 3] in the fixed-transform frame, vertex_count [oc,1]) for ADD / ADD-S (:1047-1074)."""
        if self.mesh_spec is not None:
            return self.mesh_scenes().generate_object_vertex_array()
        oc = len(self.objectsofinterest)
        count = np.zeros((oc, 1), np.int32)
        for i, o in enumerate(self.objectsofinterest):
            if o in self.meshes:
                count[i, 0] = len(self.meshes[o]["vertices"])
        arr = np.zeros((oc, int(count.max()), 3), np.float32)
        for i, o in enumerate(self.objectsofinterest):
            for fixed in self.fixed_transformations.values():
                if o in fixed and o in self.meshes:
                    arr[i, :count[i, 0]] = transform_points(self.meshes[o]["vertices"], fixed[o])
                    break
        return arr, count


# ------------------------------------------------------------------------------------------------
# exporter: the synthetic scene in the on-disk format above (round-trip tests; a sample dataset for the drivers)
# ------------------------------------------------------------------------------------------------
def write_ndds_scene(root: str, meshes_dir: str, scene, count: int, names: Sequence[str], scene_name: str = "000000"):
    """Render `count` images of a SyntheticSceneDataset (built for the full 480x640 frame) into <root>/<scene_name>/ and its
    object models into <meshes_dir>/ in the layout VectorfieldDataset reads."""
    from PIL import Image

    from .synthetic_scene import CAMERA, FULL_H, FULL_W

    assert scene.size == (FULL_H, FULL_W) and len(names) == scene.oc
    d = os.path.join(root, scene_name)
    os.makedirs(d, exist_ok=True)
    os.makedirs(meshes_dir, exist_ok=True)

    def write_ply(path, v):
        with open(path, "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(v))
            for p in v:
                f.write("%.6f %.6f %.6f\n" % tuple(p))

    info = {}
    for o, name in enumerate(names):
        os.makedirs(os.path.join(meshes_dir, name), exist_ok=True)
        write_ply(os.path.join(meshes_dir, name, name + ".ply"), scene.mesh_vertex_array[o])
        write_ply(os.path.join(meshes_dir, name, name + "_keypoints.ply"), scene.keypoints3d[o])
        info[name] = {"diameter": float(scene.diameters[o])}
    json.dump(info, open(os.path.join(meshes_dir, "models_info.json"), "w"))
    json.dump({"exported_objects": [{"class": n, "segmentation_class_id": 10 * (o + 1), "fixed_model_transform": np.identity(4).tolist()}
                                    for o, n in enumerate(names)]}, open(os.path.join(d, "_object_settings.json"), "w"))
    json.dump({"camera_settings": [{"intrinsic_settings": {"fx": CAMERA[0, 0], "fy": CAMERA[1, 1], "cx": CAMERA[0, 2], "cy": CAMERA[1, 2]}}]},
              open(os.path.join(d, "_camera_settings.json"), "w"))
    for i in range(count):
        it = scene._render(np.random.default_rng([scene.seed, i]))
        img = np.clip((it["img"] * 0.5 + 0.5) * 255.0 + 0.5, 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(d, "%06d.png" % i))
        Image.fromarray((it["label"].astype(np.uint8) * 10)).save(os.path.join(d, "%06d.seg.png" % i))
        objs = []
        for o, name in enumerate(names):
            P = it["poses"][o]
            objs.append({"class": name, "visibility": 1.0, "px_count_all": int(it["counts"][o]), "location": P[:, 3].tolist(),
                         "quaternion_xyzw": matrix_to_quaternion_xyzw(P[:, :3]).tolist(),
                         "keypoints_2d": it["kp2"][o][:, ::-1].tolist(), "keypoints_3d": scene.keypoints3d[o].tolist()})
        json.dump({"objects": objs}, open(os.path.join(d, "%06d.json" % i), "w"))
