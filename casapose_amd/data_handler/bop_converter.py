"""BOP datasets (scene_gt.json, scene_camera.json, scene_gt_info.json, rgb/, mask_visib/, models*/) converted to the layout VectorfieldDataset
reads -- the counterpart of util_scripts/dataset_converter.py:51-482 without pyrender, trimesh or cv2: PIL for images, NumPy for geometry and
csrc/masks.hip for the one compute step, the segmentation mask rendered from the meshes (`settings["mask"] = "render"`, the reference's
create_ndds_mask :64-95).

    generate_data(dataset_path, dataset_path_out, settings, model_folder, model_folder_out, image_folder)

`settings` keeps the reference's keys: near, far, width, height, filetype_in, mask ("reuse" builds NNNNNN.seg.png from mask_visib/, "render"
renders it, anything else writes none), copy_meshes, draw_debug_image (refused: visualisation is not part of this build).  Six keys are new and
default to the reference's behaviour:
    mask_sample_offset  0.5: where a pixel is sampled, in pixels from its integer coordinate.  0.5 is the reference (pyrender's GL window puts the
                        centre of pixel j at u = j + 0.5 while cx, cy are handed over unchanged); 0.0 is BOP's convention, centres at integers
    gt_info             "file": visibility, pixel counts and boxes from scene_gt_info.json when it exists, else `visibility 1` and no counts;
                        "render": px_count_all, px_count_visib, visibility (= visib / all, 0 when all = 0), bounding_box and
                        bounding_box_visible from the renderer's records (px_count_valid is omitted); works with mask = "reuse" too
    renderer            "device" (default; needs a GPU, there is no fall-back) or "host", the kernel's serial twin
    keypoints           "file": obj_NNNNNN_keypoints.ply beside each mesh, as the reference ships them for LM and HomebrewedDB;
                        "generate": the box centre and farthest-point samples of the mesh vertices (model_prep.py, csrc/models.hip), so that any
                        BOP dataset or folder of meshes converts; they feed the frame JSONs and, with copy_meshes, are written as
                        <out>/<name>/<name>_keypoints.ply
    models_info         "file": <models>/models_info.json must exist and is copied; "generate": diameter, min_* and size_* computed from the
                        vertices and written, with copy_meshes, as <out>/models_info.json keyed by the mesh's name (what the reader looks up);
                        an existing entry's other fields (symmetries) are carried over
    no_points           9: keypoints per object in "generate" mode, the centre included

Differences from the reference, all stated: `cuboid` / `projected_cuboid` come from the axis-aligned box of the mesh vertices (trimesh's
bounding_box_oriented is not reproducible without trimesh; the reader does not read them); without scene_gt_info.json the reference's
create_ndds_json raises KeyError 'bb', here the box is BOP's empty box (-1, -1, -1, -1); a triangle with a vertex in front of the near plane
is dropped whole where the reference's renderer clips it, and each frame where that happens is reported by frame and object.

Host I/O (PNG reading and writing, JSON writing, copyfile) runs on a small thread pool; the renderer works one chunk of frames ahead on a
side stream with an event, the convention of device_pipeline.py."""
from __future__ import annotations

import glob
import json
import os
import re
from concurrent.futures import ThreadPoolExecutor
from shutil import copyfile
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib, twin
from ..utils.io_utils import to_json
from .vectorfield_dataset import _bbox_corners, read_faces, read_vertices

RECORD = 11   # cp_mask::RECORD of csrc/mask_math.h: px_count_all, px_count_visib, bbox_obj[4], bbox_visib[4], dropped_triangles
R_ALL, R_VISIB, R_BOX_OBJ, R_BOX_VISIB, R_DROPPED = 0, 1, 2, 6, 10
MAX_INSTANCES = 256
DEFAULT_WORKSPACE_CAP = 1 << 30


# ------------------------------------------------------------------------------------------------
# the reference's small geometry (utils/geometry_utils.py)
# ------------------------------------------------------------------------------------------------
def project(xyz, K, RT):
    """geometry_utils.py:60-69: (pixels [N, 2], camera points [N, 3]) of model points [N, 3] under K [3, 3] and RT [3, 4]"""
    cam = np.dot(xyz, RT[:, :3].T) + RT[:, 3:].T
    hom = np.dot(cam, K.T)
    return hom[:, :2] / hom[:, 2:], cam


def matrix_to_quaternion(M):
    """geometry_utils.py:73-97: xyzw with w >= 0, the eigenvector of the largest eigenvalue of the symmetric 4x4 built from the rotation (its
    lower triangle is all `eigh` reads)"""
    m = np.asarray(M, np.float64).reshape(3, 3)
    K = np.zeros((4, 4))
    K[0, 0], K[1, 1], K[2, 2] = m[0, 0] - m[1, 1] - m[2, 2], m[1, 1] - m[0, 0] - m[2, 2], m[2, 2] - m[0, 0] - m[1, 1]
    K[1, 0], K[2, 0], K[2, 1] = m[0, 1] + m[1, 0], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1]
    K[3, 0], K[3, 1], K[3, 2] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]
    K[3, 3] = m[0, 0] + m[1, 1] + m[2, 2]
    vals, vecs = np.linalg.eigh(K / 3.0)
    q = vecs[:, np.argmax(vals)].copy()
    return -q if q[3] < 0 else q


def get_horizontal_width_angle(width, height, fx, fy):
    """geometry_utils.py:100-102: the horizontal field of view in degrees"""
    fy_rel = fy / height
    return np.rad2deg(2.0 * np.arctan((width / fx * fy_rel) * (0.5 / fy_rel)))


def create_transformation_matrix(R, t):
    """geometry_utils.py:105-113: the 4x4 [R t; 0 1]"""
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = np.asarray(R, np.float64), np.asarray(t, np.float64)
    return M


# ------------------------------------------------------------------------------------------------
# the mask renderer
# ------------------------------------------------------------------------------------------------
class MaskRenderer:
    """Meshes uploaded once; frames rendered in chunks.

    meshes: {object id: (vertices [V, 3], faces [T, 3])}.  A frame is a dict with `cam` = (fx, fy, cx, cy) and `instances` = a list of
    (object id, label 0..255, pose [3, 4]).  render / render_host return (labels uint8 [frames, H, W], records int32 [frames, instances_max, 11])
    as NumPy arrays, instances_max = the largest instance count among the frames (at least 1); record fields in the order of `RECORD`'s comment.
    device = None builds a renderer that can only run the host twin."""

    def __init__(self, device, meshes: Dict[int, Tuple[np.ndarray, np.ndarray]], workspace_cap: int = DEFAULT_WORKSPACE_CAP):
        import torch

        self.lib = _lib.load()
        self.ids = sorted(meshes)
        if not self.ids:
            raise ValueError("MaskRenderer needs at least one mesh")
        self.index = {obj: i for i, obj in enumerate(self.ids)}
        for obj in self.ids:
            v, f = np.asarray(meshes[obj][0]), np.asarray(meshes[obj][1])
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or len(v) == 0 or len(f) == 0:
                raise ValueError("object %s: a mesh is vertices [V, 3] and faces [T, 3], both non-empty (got %s, %s)" % (obj, v.shape, f.shape))
            if f.min() < 0 or f.max() >= len(v):
                raise ValueError("object %s: face indices must lie in [0, %d)" % (obj, len(v)))
        self.vmax = max(len(meshes[o][0]) for o in self.ids)
        self.tmax = max(len(meshes[o][1]) for o in self.ids)
        self.verts = np.zeros((len(self.ids), self.vmax, 3), np.float32)
        self.faces = np.zeros((len(self.ids), self.tmax, 3), np.int32)
        self.vert_counts = np.zeros(len(self.ids), np.int32)
        self.face_counts = np.zeros(len(self.ids), np.int32)
        for i, obj in enumerate(self.ids):
            v, f = np.asarray(meshes[obj][0], np.float32), np.asarray(meshes[obj][1], np.int32)
            self.verts[i, :len(v)], self.faces[i, :len(f)] = v, f
            self.vert_counts[i], self.face_counts[i] = len(v), len(f)
        self.workspace_cap = int(workspace_cap)
        self.device = None if device is None else torch.device(device)
        self.stream = None
        if self.device is not None:
            if not torch.cuda.is_available():
                raise _lib.CasaposeHipError("MaskRenderer(device=%s) needs a ROCm GPU; the host twin is render_host" % (device,))
            self.d_mesh = [torch.from_numpy(a).to(self.device) for a in (self.verts, self.vert_counts, self.faces, self.face_counts)]

    # ---- packing ----------------------------------------------------------------------------------
    def pack(self, frames: Sequence[dict], instances_max: Optional[int] = None) -> Dict[str, np.ndarray]:
        imax = max([1] + [len(fr["instances"]) for fr in frames]) if instances_max is None else int(instances_max)
        if imax > MAX_INSTANCES:
            raise ValueError("a frame has %d instances, the renderer takes at most %d" % (imax, MAX_INSTANCES))
        n = len(frames)
        out = dict(cams=np.zeros((n, 4), np.float64), inst_counts=np.zeros(n, np.int32), inst_obj=np.zeros((n, imax), np.int32),
                   inst_label=np.zeros((n, imax), np.int32), poses=np.zeros((n, imax, 12), np.float64))
        for i, fr in enumerate(frames):
            out["cams"][i] = np.asarray(fr["cam"], np.float64).reshape(4)
            out["inst_counts"][i] = len(fr["instances"])
            for k, (obj, label, pose) in enumerate(fr["instances"]):
                if obj not in self.index:
                    raise KeyError("frame %d names object %s, which has no mesh" % (i, obj))
                if not 0 <= int(label) <= 255:
                    raise ValueError("frame %d, object %s: label %d does not fit the uint8 mask" % (i, obj, label))
                out["inst_obj"][i, k], out["inst_label"][i, k] = self.index[obj], int(label)
                out["poses"][i, k] = np.asarray(pose, np.float64).reshape(12)
        return out

    def chunk_frames(self, n: int, instances_max: int, H: int, W: int, workspace_cap: Optional[int] = None) -> int:
        """frames per launch under the workspace cap; a single frame above the cap is an error"""
        cap = self.workspace_cap if workspace_cap is None else int(workspace_cap)
        one = int(self.lib.cp_render_masks_workspace_bytes(1, instances_max, H, W))
        if one == 0:
            raise ValueError("the renderer takes H, W in [1, 16384] and at most %d instances per frame (got %d x %d, %d)" % (MAX_INSTANCES, H, W, instances_max))
        if one > cap:
            raise ValueError("one %d x %d frame with %d instances needs %d bytes of depth planes, the workspace cap is %d" % (H, W, instances_max, one, cap))
        return max(1, min(n, cap // one, 65535))

    # ---- the library call, host twin or device ---------------------------------------------------------
    def _render(self, mesh, p, n: int, H: int, W: int, near: float, far: float, sample_offset: float, workspace, workspace_bytes: int, device, stream):
        """cp_render_masks_u8 on `stream` over device tensors, or (device None) its host twin over NumPy arrays: `mesh` = verts, vert_counts,
        faces, face_counts and `p` = n packed frames, where the call runs -> (labels, records) there"""
        imax = p["inst_obj"].shape[1]
        out = twin.alloc(dict(labels=((n, H, W), np.uint8), records=((n, imax, RECORD), np.int32)), device)
        twin.call("cp_render_masks_u8", mesh[0], mesh[1], self.vmax, mesh[2], mesh[3], self.tmax, len(self.ids), p["cams"], p["inst_counts"],
                  p["inst_obj"], p["inst_label"], p["poses"], n, imax, H, W, float(near), float(far), float(sample_offset), out["labels"],
                  out["records"], workspace, workspace_bytes, host=device is None, stream=stream)
        return out["labels"], out["records"]

    def render_host(self, frames: Sequence[dict], height: int, width: int, near: float, far: float, sample_offset: float = 0.5,
                    instances_max: Optional[int] = None):
        p = self.pack(frames, instances_max)
        n, imax = len(frames), p["inst_obj"].shape[1]
        if n == 0:
            return np.empty((n, height, width), np.uint8), np.empty((n, imax, RECORD), np.int32)
        size = int(self.lib.cp_render_masks_workspace_bytes(n, imax, height, width))
        return self._render((self.verts, self.vert_counts, self.faces, self.face_counts), p, n, height, width, near, far, sample_offset,
                            np.empty(max(size // 4, 1), np.uint32), size, None, None)

    def _launch(self, p: Dict[str, np.ndarray], lo: int, hi: int, H: int, W: int, near: float, far: float, sample_offset: float, workspace):
        """frames [lo, hi) of the packed arrays on the side stream -> (pinned labels, pinned records, event)"""
        import torch

        dev, st = self.device, self.stream
        with torch.cuda.stream(st):
            d = {k: torch.from_numpy(np.ascontiguousarray(a[lo:hi])).pin_memory().to(dev, non_blocking=True) for k, a in p.items()}
            labels, records = self._render(self.d_mesh, d, hi - lo, H, W, near, far, sample_offset, workspace, workspace.numel(), dev, st.cuda_stream)
            h_labels = torch.empty(labels.shape, dtype=torch.uint8, pin_memory=True)
            h_records = torch.empty(records.shape, dtype=torch.int32, pin_memory=True)
            h_labels.copy_(labels, non_blocking=True)
            h_records.copy_(records, non_blocking=True)
            done = torch.cuda.Event()
            done.record(st)
        return h_labels, h_records, done, (d, labels, records)

    def render_chunks(self, frames: Sequence[dict], height: int, width: int, near: float, far: float, sample_offset: float = 0.5,
                      workspace_cap: Optional[int] = None, renderer: str = "device") -> Iterator[Tuple[int, np.ndarray, np.ndarray]]:
        """(first frame, labels, records) per chunk of frames, in order.  On the device chunk c + 1 is launched before chunk c is waited for, so
        the consumer's work on a chunk (PNG encoding) overlaps the next one's rendering; all chunks share one workspace, in stream order."""
        if renderer not in ("device", "host"):
            raise ValueError("renderer must be 'device' or 'host' (got %r)" % (renderer,))
        n = len(frames)
        if n == 0:
            return
        p = self.pack(frames)
        imax = p["inst_obj"].shape[1]
        step = self.chunk_frames(n, imax, height, width, workspace_cap)
        bounds = [(lo, min(lo + step, n)) for lo in range(0, n, step)]
        if renderer == "host":
            for lo, hi in bounds:
                labels, records = self.render_host(frames[lo:hi], height, width, near, far, sample_offset, imax)
                yield lo, labels, records
            return
        if self.device is None:
            raise _lib.CasaposeHipError("this MaskRenderer was built without a device; there is no fall-back to the host twin (ask for renderer='host')")
        import torch

        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        size = int(self.lib.cp_render_masks_workspace_bytes(step, imax, height, width))
        with torch.cuda.stream(self.stream):
            workspace = torch.empty(size, dtype=torch.uint8, device=self.device)
        flight = self._launch(p, *bounds[0], height, width, near, far, sample_offset, workspace)
        for c, (lo, hi) in enumerate(bounds):
            ahead = self._launch(p, *bounds[c + 1], height, width, near, far, sample_offset, workspace) if c + 1 < len(bounds) else None
            flight[2].synchronize()
            yield lo, flight[0].numpy(), flight[1].numpy()
            flight = ahead

    def render(self, frames: Sequence[dict], height: int, width: int, near: float, far: float, sample_offset: float = 0.5,
               workspace_cap: Optional[int] = None, renderer: str = "device"):
        parts = list(self.render_chunks(frames, height, width, near, far, sample_offset, workspace_cap, renderer))
        if not parts:
            return np.empty((0, height, width), np.uint8), np.empty((0, 1, RECORD), np.int32)
        return np.concatenate([np.array(l) for _, l, _ in parts]), np.concatenate([np.array(r) for _, _, r in parts])


# ------------------------------------------------------------------------------------------------
# files written per frame
# ------------------------------------------------------------------------------------------------
def create_bop_mask(path, path_out, gt, digits, width, height, filetypet):
    """dataset_converter.py:51-61: the NDDS mask from BOP's mask_visib/<digits>_<instance>.png, a later instance over an earlier one"""
    from PIL import Image

    mask = np.zeros([height, width], dtype=np.uint8)
    path = path.replace("rgb", "mask_visib")
    for idx, mesh_gt in enumerate(gt):
        part = np.array(Image.open(path.replace(digits + "." + filetypet, digits + "_" + str(idx).zfill(6) + ".png")))
        mask[part == 255] = mesh_gt["id"]
    Image.fromarray(mask).save(path_out)


def write_camera_setting(path, name, camera_matrix, width, height):
    """dataset_converter.py:98-124"""
    fx, fy = camera_matrix[0][0], camera_matrix[1][1]
    intrinsics = {"resX": width, "resY": height, "fx": fx, "fy": fy, "cx": camera_matrix[0][2], "cy": camera_matrix[1][2], "s": 0}
    camera = {"name": name, "horizontal_fov": get_horizontal_width_angle(width, height, fx, fy), "intrinsic_settings": intrinsics,
              "captured_image_size": {"width": width, "height": height}}
    with open(path, "w") as outfile:
        outfile.write(to_json({"camera_settings": [camera]}))


def write_object_settings(path, meshes):
    """dataset_converter.py:127-144: the objects that occurred in this scene"""
    classes, objects = [], []
    for mesh in meshes:
        if meshes[mesh]["counter"] > 0:
            classes.append(meshes[mesh]["name"])
            objects.append({"class": meshes[mesh]["name"], "segmentation_class_id": meshes[mesh]["id"], "segmentation_instance_id": 0,
                            "fixed_model_transform": meshes[mesh]["fixed_model_transform"].tolist(), "cuboid_dimensions": meshes[mesh]["volume_size"]})
    with open(path, "w") as outfile:
        outfile.write(to_json({"exported_object_classes": classes, "exported_objects": objects}))


def ndds_json_data(camera_matrix, gt, meshes) -> dict:
    """The frame's annotation (dataset_converter.py:150-204) as a dict; counts the objects it names in meshes[...]["counter"]."""
    objects = []
    for mesh_gt in gt:
        object_id, t, R = mesh_gt["id"], mesh_gt["t"], mesh_gt["R"]
        bb = mesh_gt.get("bb", [-1, -1, -1, -1])   # the reference raises KeyError here when there is no scene_gt_info.json
        pose = create_transformation_matrix(R, t)
        mesh = meshes[object_id]
        mesh["counter"] = mesh["counter"] + 1
        info = {"class": mesh["name"], "instance_id": 0}
        info["visibility"] = mesh_gt["visib_fract"] if "visib_fract" in mesh_gt else 1
        for key in ("px_count_all", "px_count_valid", "px_count_visib"):
            if key in mesh_gt:
                info[key] = mesh_gt[key]
        info["location"] = t
        info["quaternion_xyzw"] = matrix_to_quaternion(R)
        info["pose_transform"] = np.transpose(pose).tolist()
        center_2d, center_3d = project(np.array(np.expand_dims(mesh["center"], 0)), camera_matrix, pose[0:3])
        info["cuboid_centroid"] = center_3d[0]
        info["projected_cuboid_centroid"] = center_2d[0]
        info["bounding_box"] = {"top_left": [bb[0], bb[1]], "bottom_right": [bb[0] + bb[2], bb[1] + bb[3]]}
        if "bb_visib" in mesh_gt:
            bv = mesh_gt["bb_visib"]
            info["bounding_box_visible"] = {"top_left": [bv[0], bv[1]], "bottom_right": [bv[0] + bv[2], bv[1] + bv[3]]}
        cuboid_2d, cuboid_3d = project(mesh["volume"], camera_matrix, pose[0:3])
        info["cuboid"] = cuboid_3d.tolist()
        info["projected_cuboid"] = cuboid_2d.tolist()
        keypoints_2d, keypoints_3d = project(mesh["keypoints"], camera_matrix, pose[0:3])
        info["keypoints_2d"] = keypoints_2d.tolist()
        info["keypoints_3d"] = keypoints_3d.tolist()
        objects.append(info)
    return {"camera_data": {"location_worldframe": [0.0, 0.0, 0.0], "quaternion_xyzw_worldframe": [0.0, 0.0, 0.0, 1.0]}, "objects": objects}


def create_ndds_json(path, camera_matrix, gt, meshes, debug_image=None):
    """dataset_converter.py:147-212; returns meshes with the updated counters"""
    if debug_image is not None:
        raise NotImplementedError("draw_debug_image: visualisation is not part of this build")
    data = ndds_json_data(camera_matrix, gt, meshes)
    with open(path, "w") as outfile:
        outfile.write(to_json(data))
    return meshes


# ------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------
def load_object(path_keypoints, path_mesh, index, name, meshes, fixed_transform=None):
    """dataset_converter.py:215-241 without trimesh: vertices and faces through read_vertices / read_faces; `volume` is the axis-aligned box
    of the mesh vertices (the stated difference from bounding_box_oriented)."""
    keypoints, vertices = read_vertices(path_keypoints), read_vertices(path_mesh)
    meshes[index] = {"name": name, "keypoints": keypoints, "volume": _bbox_corners(vertices),
                     "volume_size": np.max(keypoints, 0) - np.min(keypoints, 0), "center": (np.max(keypoints, 0) + np.min(keypoints, 0)) / 2.0,
                     "counter": 0, "fixed_model_transform": np.eye(4), "id": index,
                     "mesh": {"vertices": vertices, "faces": read_faces(path_mesh), "path": path_mesh}}
    return meshes


def load_model_infos(files):
    """dataset_converter.py:262-275"""
    model_info, model_info_file = {}, ""
    for file in files:
        if os.path.basename(file) == "models_info.json":
            model_info_file = file
            with open(file) as f:
                model_info = json.load(f)
        else:
            print("unknown file: {}".format(os.path.basename(file)))
    return model_info, model_info_file


def _generate_models_bop(path, path_root_out, copy_meshes, settings):
    """load_models_bop with settings["keypoints"] or settings["models_info"] = "generate": meshes and keypoint files are paired by name, never by
    sorted position; what is generated comes from ModelPrep on settings["renderer"] and needs no file; nothing is written under `path`."""
    from .model_prep import model_prep_for, write_keypoints_ply, write_models_info

    kp_mode, info_mode = settings.get("keypoints", "file"), settings.get("models_info", "file")
    for key, mode in (("keypoints", kp_mode), ("models_info", info_mode)):
        if mode not in ("file", "generate"):
            raise ValueError("settings[%r] must be 'file' or 'generate' (got %r)" % (key, mode))
    info_file = os.path.join(path, "models_info.json")
    existing = None
    if os.path.isfile(info_file):
        with open(info_file) as f:
            existing = json.load(f)
    if info_mode == "file" and not existing:
        return None
    files = [a for a in sorted(glob.glob(path + "/*.ply")) if not a.endswith("keypoints.ply")] or sorted(glob.glob(path + "/*.obj"))
    model_files = {os.path.splitext(os.path.basename(a))[0]: a for a in files}
    vertices, ids = {}, {}
    for name, file in model_files.items():
        digits = re.findall(r"\d+", name)
        if len(digits) == 0:
            print("no object id in the name: {}".format(os.path.basename(file)))
            continue
        ids[name], vertices[name] = int(digits[0]), read_vertices(file)
    prepared = model_prep_for(settings.get("renderer", "device")).run(vertices, settings.get("no_points", 9), settings.get("renderer", "device"))
    meshes = {}
    for name in ids:
        print(name)
        file, v = model_files[name], vertices[name]
        if kp_mode == "generate":
            keypoints = prepared[name]["keypoints"].astype(np.float64)
        else:
            kp_file = os.path.join(os.path.dirname(file), name + "_keypoints.ply")
            if not os.path.isfile(kp_file):
                raise FileNotFoundError("%s: no keypoint file (settings['keypoints'] = 'generate' makes the keypoints from the mesh)" % kp_file)
            keypoints = read_vertices(kp_file)
        meshes[ids[name]] = {"name": name, "keypoints": keypoints, "volume": _bbox_corners(v), "volume_size": np.max(keypoints, 0) - np.min(keypoints, 0),
                             "center": (np.max(keypoints, 0) + np.min(keypoints, 0)) / 2.0, "counter": 0, "fixed_model_transform": np.eye(4),
                             "id": ids[name], "mesh": {"vertices": v, "faces": read_faces(file), "path": file}}
        if copy_meshes:
            path_out = os.path.join(path_root_out, name)
            os.makedirs(path_out, exist_ok=True)
            copyfile(file, os.path.join(path_out, name + os.path.splitext(file)[1].lower()))
            write_keypoints_ply(os.path.join(path_out, name + "_keypoints.ply"), keypoints)
    if copy_meshes:
        out_file = os.path.join(path_root_out, "models_info.json")
        if info_mode == "generate":
            write_models_info(out_file, {name: prepared[name] for name in ids}, existing)
        else:
            print("Copy: " + info_file)
            copyfile(info_file, out_file)
    return meshes


def load_models_bop(path, path_root_out, copy_meshes=False, settings=None):
    """dataset_converter.py:424-463: {object id: mesh record} of <path>/obj_NNNNNN.ply (else .obj) paired with obj_NNNNNN_keypoints.ply by
    sorted position; with copy_meshes the reader's <out>/<name>/<name>.ply layout and models_info.json are written.  With
    settings["keypoints"] or settings["models_info"] = "generate" the missing files are computed from the meshes (_generate_models_bop)."""
    if not os.path.exists(path_root_out):
        os.mkdir(path_root_out)
    if settings is not None and (settings.get("keypoints", "file") != "file" or settings.get("models_info", "file") != "file"):
        return _generate_models_bop(path, path_root_out, copy_meshes, settings)
    model_infos, model_info_file = load_model_infos(sorted(glob.glob(path + "/*" + ".json")))
    if len(model_infos) == 0:
        return
    model_keypoint_files = sorted(glob.glob(path + "/*" + "keypoints.ply"))
    model_files = [a for a in sorted(glob.glob(path + "/*" + ".ply")) if a not in model_keypoint_files]
    if len(model_files) == 0:
        model_files = sorted(glob.glob(path + "/*" + ".obj"))
    meshes = {}
    for i in range(len(model_files)):
        name = os.path.splitext(os.path.basename(model_files[i]))[0]
        print(name)
        digits_model = re.findall(r"\d+", name)
        digits_keypoints = re.findall(r"\d+", os.path.basename(model_keypoint_files[i]))
        if len(digits_model) > 0 and len(digits_keypoints) > 0 and int(digits_keypoints[0]) == int(digits_model[0]):
            meshes = load_object(model_keypoint_files[i], model_files[i], int(digits_model[0]), name, meshes)
        if copy_meshes:
            path_out = path_root_out + "/" + name
            if not os.path.exists(path_out):
                os.mkdir(path_out)
            copyfile(model_files[i], path_out + "/" + name + ".ply")
            copyfile(model_keypoint_files[i], path_out + "/" + name + "_keypoints.ply")
    if copy_meshes:
        print("Copy: " + model_info_file)
        copyfile(model_info_file, path_root_out + "/models_info.json")
    return meshes


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def get_cam_matrix_bop(info):
    """dataset_converter.py:244-250"""
    cam = np.eye(3)
    cam[0][0], cam[1][1], cam[0][2], cam[1][2] = info["cam_K"][0], info["cam_K"][4], info["cam_K"][2], info["cam_K"][5]
    return cam


def load_json_info(files):
    """dataset_converter.py:278-326: ({image: {"cam_mat"}}, {image: [{"id", "t", "R", and from scene_gt_info.json "bb", "bb_visib",
    "px_count_all", "px_count_valid", "px_count_visib", "visib_fract"}]})"""
    cameras, gts, gt_infos = {}, {}, {}
    for file in files:
        name = os.path.basename(file)
        if name in ("scene_gt.json", "scene_camera.json", "scene_gt_info.json"):
            with open(file) as f:
                loaded = json.load(f)
            if name == "scene_gt.json":
                gts = loaded
            elif name == "scene_camera.json":
                cameras = loaded
            else:
                gt_infos = loaded
        else:
            print("unknown json file: {}".format(name))
    cameras_out = {int(c): {"cam_mat": get_cam_matrix_bop(cameras[c])} for c in cameras}
    gts_out = {}
    for gt in gts:
        gts_out[int(gt)] = [{"id": o["obj_id"], "t": o["cam_t_m2c"], "R": np.array(o["cam_R_m2c"]).reshape(3, 3)} for o in gts[gt]]
    for image in gt_infos:
        for i, o in enumerate(gt_infos[image]):
            entry = gts_out[int(image)][i]
            entry["bb"], entry["bb_visib"] = o["bbox_obj"], o["bbox_visib"]
            for key in ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract"):
                entry[key] = o[key]
    return cameras_out, gts_out


def apply_render_records(gt: List[dict], records: np.ndarray):
    """gt_info = "render": the frame's counts, visibility and boxes from the renderer's records, one per instance in gt's order"""
    for k, mesh_gt in enumerate(gt):
        r = [int(x) for x in records[k]]
        mesh_gt["px_count_all"], mesh_gt["px_count_visib"] = r[R_ALL], r[R_VISIB]
        mesh_gt["visib_fract"] = r[R_VISIB] / r[R_ALL] if r[R_ALL] > 0 else 0.0
        mesh_gt["bb"], mesh_gt["bb_visib"] = r[R_BOX_OBJ:R_BOX_OBJ + 4], r[R_BOX_VISIB:R_BOX_VISIB + 4]
        mesh_gt.pop("px_count_valid", None)


def _renderer_for(meshes, settings) -> MaskRenderer:
    """the scene's renderer, built once per conversion and kept in the settings dict's private slot"""
    if settings.get("_mask_renderer") is None:
        for obj in sorted(meshes):
            if int(obj) > 255:
                raise ValueError("obj_id %d does not fit the uint8 segmentation mask (ids 0..255)" % obj)
            if len(meshes[obj]["mesh"]["faces"]) == 0:
                raise ValueError("%s has no faces: a mask cannot be rendered from it" % meshes[obj]["mesh"]["path"])
        which = settings.get("renderer", "device")
        if which not in ("device", "host"):
            raise ValueError("settings['renderer'] must be 'device' or 'host' (got %r)" % (which,))
        device = None
        if which == "device":
            import torch

            if not torch.cuda.is_available():
                raise _lib.CasaposeHipError("rendering masks (mask='render' or gt_info='render') needs a ROCm GPU; settings['renderer'] = 'host' "
                                            "asks for the serial host twin instead")
            device = torch.device("cuda", torch.cuda.current_device())
        settings["_mask_renderer"] = MaskRenderer(device, {obj: (m["mesh"]["vertices"], m["mesh"]["faces"]) for obj, m in meshes.items()},
                                                  settings.get("workspace_cap", DEFAULT_WORKSPACE_CAP))
    return settings["_mask_renderer"]


def parse_bop(root, root_out, meshes, settings):
    """dataset_converter.py:329-421: every folder under `root` that holds rgb/ is one scene: its camera, its frames (image copied, NNNNNN.json,
    NNNNNN.seg.png) and its object list go to the same place under `root_out`."""
    from PIL import Image

    if settings.get("draw_debug_image"):
        raise NotImplementedError("draw_debug_image: visualisation is not part of this build")
    mask_mode, gt_mode = settings.get("mask"), settings.get("gt_info", "file")
    if gt_mode not in ("file", "render"):
        raise ValueError("settings['gt_info'] must be 'file' or 'render' (got %r)" % (gt_mode,))
    width, height = settings["width"], settings["height"]
    workers = int(settings.get("io_threads") or min(16, os.cpu_count() or 1))

    def write_text(path, text):
        with open(path, "w") as outfile:
            outfile.write(text)

    def save_mask(path, mask):
        Image.fromarray(mask).save(path)

    def update_bop_files(path, info, gt, meshes, pool):
        filetype = "." + settings["filetype_in"]
        files = sorted(glob.glob(path + "/[0-9][0-9][0-9][0-9][0-9][0-9]" + filetype))   # six digits
        if len(files) > 0:
            path_out = path.replace(root, root_out)
            if not os.path.exists(path_out):
                os.mkdir(path_out)
        jobs, work = [], []   # work: (image index, file, file out, digits)
        for filepath in files:
            digits = re.findall(r"\d+", os.path.basename(filepath))
            if len(digits) > 0:
                filepath_out = filepath.replace(root, root_out)
                if filepath_out != filepath:
                    jobs.append(pool.submit(copyfile, filepath, filepath_out))
                work.append((int(digits[0]), filepath, filepath_out, digits[0]))
        for obj_gt in (g for idx, _, _, _ in work for g in gt[idx]):
            if int(obj_gt["id"]) > 255:
                raise ValueError("obj_id %d does not fit the uint8 segmentation mask (ids 0..255)" % obj_gt["id"])

        def finish(idx, filepath, filepath_out, digits, labels, records):
            if gt_mode == "render":
                apply_render_records(gt[idx], records)
            data = ndds_json_data(info[idx]["cam_mat"], gt[idx], meshes)   # in this thread: it counts the objects
            jobs.append(pool.submit(lambda: write_text(filepath_out.replace(filetype, ".json"), to_json(data))))
            if mask_mode == "reuse":
                jobs.append(pool.submit(create_bop_mask, filepath, filepath_out.replace(filetype, ".seg.png"), gt[idx], digits, width, height,
                                        settings["filetype_in"]))
            elif mask_mode == "render":
                jobs.append(pool.submit(save_mask, filepath_out.replace(filetype, ".seg.png"), np.array(labels)))

        if mask_mode == "render" or gt_mode == "render":
            renderer = _renderer_for(meshes, settings)
            frames = []
            for idx, _, _, _ in work:
                K = info[idx]["cam_mat"]
                frames.append(dict(cam=(K[0][0], K[1][1], K[0][2], K[1][2]),
                                   instances=[(g["id"], g["id"], create_transformation_matrix(g["R"], g["t"])[0:3]) for g in gt[idx]]))
            for lo, labels, records in renderer.render_chunks(frames, height, width, settings["near"], settings["far"],
                                                              settings.get("mask_sample_offset", 0.5), settings.get("workspace_cap"),
                                                              settings.get("renderer", "device")):
                for c in range(len(labels)):
                    idx, filepath, filepath_out, digits = work[lo + c]
                    for k, g in enumerate(gt[idx]):
                        if records[c, k, R_DROPPED] > 0:
                            print("warning: %s: object %d (instance %d) lost %d triangles to the near plane; its mask and counts are incomplete"
                                  % (filepath, g["id"], k, int(records[c, k, R_DROPPED])))
                    finish(idx, filepath, filepath_out, digits, labels[c], np.array(records[c]))
        else:
            for idx, filepath, filepath_out, digits in work:
                finish(idx, filepath, filepath_out, digits, None, None)
        for job in jobs:
            job.result()
        return meshes

    def explore(path, meshes, pool):
        if not os.path.isdir(path):
            return
        names = sorted(o for o in os.listdir(path) if os.path.isdir(os.path.join(path, o)))
        folders = [os.path.join(path, o) for o in names]
        if "rgb" in names:
            print(path)
            path_out = path.replace(root, root_out)
            for d in (path_out, path_out + "/rgb"):
                if not os.path.exists(d):
                    os.makedirs(d)
            for mesh in meshes:
                meshes[mesh]["counter"] = 0
            info, gt = load_json_info(sorted(glob.glob(path + "/*" + ".json")))
            camera_matrix = next(iter(info.values()))["cam_mat"]
            print(camera_matrix)
            write_camera_setting(path_out + "/rgb/_camera_settings.json", "Viewpoint", camera_matrix, width, height)
            meshes = update_bop_files(folders[names.index("rgb")], info, gt, meshes, pool)
            write_object_settings(path_out + "/rgb/_object_settings.json", meshes)
        else:
            for folder in folders:
                explore(folder, meshes, pool)

    with ThreadPoolExecutor(max_workers=max(workers, 1)) as pool:
        explore(root, meshes, pool)


def update_data(path, path_out, meshes, settings):
    """dataset_converter.py:253-259"""
    if not os.path.exists(path_out):
        os.makedirs(path_out)
    for name in sorted(os.listdir(str(path))):
        parse_bop(path + "/" + name, path_out + "/" + name, meshes, settings)


def generate_data(dataset_path, dataset_path_out, settings, model_folder="models", model_folder_out="models", image_folder="train_pbr"):
    """dataset_converter.py:467-482"""
    if settings.get("draw_debug_image"):
        raise NotImplementedError("draw_debug_image: visualisation is not part of this build")
    if not os.path.exists(dataset_path_out):
        os.makedirs(dataset_path_out)
    meshes = load_models_bop(os.path.join(dataset_path, model_folder), os.path.join(dataset_path_out, model_folder_out), settings["copy_meshes"],
                             settings)
    if meshes is None:
        raise FileNotFoundError("no models_info.json under %s" % os.path.join(dataset_path, model_folder))
    settings = dict(settings, _mask_renderer=None)
    update_data(os.path.join(dataset_path, image_folder), os.path.join(dataset_path_out, image_folder), meshes, settings)


__all__ = ["MaskRenderer", "generate_data", "update_data", "parse_bop", "load_models_bop", "load_object", "load_json_info", "get_cam_matrix_bop",
           "create_ndds_json", "write_camera_setting", "write_object_settings", "create_bop_mask", "read_faces"]
