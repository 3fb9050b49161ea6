"""Training and evaluation scenes rendered from any folder of meshes: what `--data meshes:<folder>[:N]` / `--datatest meshes:<folder>[:N]`
select in train_casapose.py and, through VectorfieldDataset, in test_casapose.py.  It delivers the batch dictionary of SyntheticSceneDataset (synthetic_scene.py), the instance axis included, with triangle
meshes in place of ellipsoids: shaded pictures from cp_render_shaded_f32 (csrc/shade.hip; the rules are listed in csrc/shade_math.h) or, without
a device, from its host twin.

The folder is a model folder in BOP's flat layout or the reader's (model_prep.find_meshes), prepared by util_scripts/make_keypoints.py: every
mesh has its `<stem>_keypoints.ply` and a diameter in `models_info.json`.  Units are millimetres.  The first `no_objects` meshes in sorted order
are object 0, 1, ...; PLY vertex colours are used where a file has them, the other objects get a flat colour drawn from the seed.

The draws of image i come from default_rng([seed, i]) in this order: everything SyntheticSceneDataset._draw / _draw_instances draws (the crop
origin; per object [its count]; per instance z from `distance`, u, v and the rotation); the light (a direction uniform on the hemisphere
l_z < 0, ambient U(0.25, 0.5), diffuse U(0.5, 0.9)); with `backgrounds` the picture's index and its crop (two uniforms); the 63-bit noise seed.
Image i is therefore the same picture alone, inside any batch and from any shard.  Ground truth is exact by construction: the label map is
cp_render_masks_u8's byte for byte, the 2-D keypoints are projected in fp64 on the host.

ShadedRenderer is the thin layer over the entry point (meshes packed once, frames per call), MeshSceneDataset the source, MeshDeviceScenes its
device half: DeviceScenes' side stream, event and prefetch queue around another launch."""
from __future__ import annotations

import functools
import json
import os
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .. import twin as _twin
from .bop_converter import MaskRenderer
from .device_scenes import DeviceScenes, from_environment
from .model_prep import _existing_entry, find_meshes
from .synthetic_scene import CAMERA, SyntheticSceneDataset
from .vectorfield_dataset import read_faces, read_vertex_colors, read_vertices

FRAME_WORDS = 8   # cp_shade::FRAME_WORDS of csrc/shade_math.h: light (3), ambient, diffuse, seed, crop row, crop column
NEAR, FAR = 10.0, 1.0e5   # mm


def frame_record(light, ambient: float, diffuse: float, seed: int, crop_row: float = 0.0, crop_col: float = 0.0) -> np.ndarray:
    rec = np.zeros(FRAME_WORDS, np.float64)
    rec[0:3], rec[3], rec[4], rec[6], rec[7] = light, ambient, diffuse, crop_row, crop_col
    rec[5:6].view(np.uint64)[0] = int(seed)
    return rec


class ShadedRenderer:
    """meshes: {object id: (vertices [V, 3], faces [T, 3])}; colors: {object id: uint8 [V, 3]} for the objects that have vertex colours;
    flat_colors: {object id: (r, g, b) in [0, 1]}.  When some objects have vertex colours and others none, the others' vertices all take
    their flat colour rounded to uint8.  Frames are MaskRenderer's: dict(cam=(fx, fy, cx, cy), instances=[(object id, label, pose [3, 4])])."""

    def __init__(self, device, meshes, colors: Optional[dict] = None, flat_colors: Optional[dict] = None):
        self.masks = MaskRenderer(device, meshes)
        m = self.masks
        self.device, self.lib = m.device, m.lib
        colors = {k: v for k, v in (colors or {}).items() if v is not None}
        self.flat = np.full((len(m.ids), 3), 0.5, np.float32)
        for obj, c in (flat_colors or {}).items():
            self.flat[m.index[obj]] = np.asarray(c, np.float32)
        self.colors = None
        if colors:
            self.colors = np.zeros((len(m.ids), m.vmax, 3), np.uint8)
            for i, obj in enumerate(m.ids):
                n = int(m.vert_counts[i])
                if obj in colors:
                    c = np.asarray(colors[obj], np.uint8)
                    if c.shape != (n, 3):
                        raise ValueError("object %s: %d vertices, colours %s" % (obj, n, c.shape))
                    self.colors[i, :n] = c
                else:
                    self.colors[i, :n] = np.rint(np.clip(self.flat[i], 0, 1) * 255.0).astype(np.uint8)
        if self.device is not None:
            self.d_colors = None if self.colors is None else torch.from_numpy(self.colors).to(self.device)
            self.d_flat = torch.from_numpy(self.flat).to(self.device)

    def workspace_bytes(self, n: int, H: int, W: int) -> int:
        size = int(self.lib.cp_render_shaded_workspace_bytes(n, H, W))
        if size == 0:
            raise ValueError("the renderer takes 1..65535 frames of H, W in [1, 16384] (got %d of %d x %d)" % (n, H, W))
        return size

    def call(self, mesh, colors, flat, p, lights, background, noise: bool, n: int, H: int, W: int, near: float, far: float, sample_offset: float,
             depth: bool, workspace, device, stream) -> dict:
        """cp_render_shaded_f32 on `stream` over device tensors, or (device None) its host twin over NumPy arrays -> img, label, depth (or None),
        dropped and keys (the workspace as one 64-bit word per pixel) where the call ran"""
        m = self.masks
        out = _twin.alloc(dict(img=((n, H, W, 3), np.float32), label=((n, H, W), np.uint8), dropped=((n,), np.int32)), device)
        out["depth"] = _twin.alloc(dict(depth=((n, H, W), np.float32)), device)["depth"] if depth else None
        size = self.workspace_bytes(n, H, W)
        _twin.call("cp_render_shaded_f32", mesh[0], mesh[1], m.vmax, mesh[2], mesh[3], m.tmax, len(m.ids), p["cams"], p["inst_counts"], p["inst_obj"],
                   p["inst_label"], p["poses"], n, p["inst_obj"].shape[1], H, W, float(near), float(far), float(sample_offset), colors, flat, lights,
                   background, int(bool(noise)), out["img"], out["label"], out["depth"], out["dropped"], workspace, size, host=device is None,
                   stream=stream)
        out["keys"] = workspace[:size // 8].reshape(n, H, W)
        return out

    def render_host(self, frames: Sequence[dict], lights, H: int, W: int, near: float = NEAR, far: float = FAR, sample_offset: float = 0.5,
                    background=None, noise: bool = False, depth: bool = True, colors: bool = True, instances_max: Optional[int] = None) -> dict:
        m = self.masks
        p = m.pack(frames, instances_max)
        n = len(frames)
        lights = np.ascontiguousarray(lights, np.float64).reshape(n, FRAME_WORDS)
        bg = None if background is None else np.ascontiguousarray(background, np.uint8).reshape(n, H, W, 3)
        return self.call((m.verts, m.vert_counts, m.faces, m.face_counts), self.colors if colors else None, self.flat, p, lights, bg, noise, n, H, W,
                         near, far, sample_offset, depth, np.empty(self.workspace_bytes(n, H, W) // 8, np.uint64), None, None)

    def render(self, frames: Sequence[dict], lights, H: int, W: int, near: float = NEAR, far: float = FAR, sample_offset: float = 0.5,
               background=None, noise: bool = False, depth: bool = True, colors: bool = True, instances_max: Optional[int] = None, stream=None) -> dict:
        """the same on the device (device tensors come back; keys as int64: the same bits)"""
        m, dev = self.masks, self.device
        p = {k: torch.from_numpy(a).to(dev) for k, a in m.pack(frames, instances_max).items()}
        n = len(frames)
        lights = torch.from_numpy(np.ascontiguousarray(lights, np.float64).reshape(n, FRAME_WORDS)).to(dev)
        bg = None if background is None else torch.from_numpy(np.ascontiguousarray(background, np.uint8).reshape(n, H, W, 3)).to(dev)
        ws = torch.empty(self.workspace_bytes(n, H, W) // 8, dtype=torch.int64, device=dev)
        return self.call(m.d_mesh, self.d_colors if colors else None, self.d_flat, p, lights, bg, noise, n, H, W, near, far, sample_offset, depth, ws, dev,
                         torch.cuda.current_stream(dev).cuda_stream if stream is None else stream)


def parse_spec(spec: str) -> Tuple[str, Optional[int]]:
    """`meshes:<folder>[:N]` -> (folder, N or None)"""
    body = spec[len("meshes:"):]
    head, sep, tail = body.rpartition(":")
    if sep and tail.isdigit() and head:
        return head, int(tail)
    return body, None


def is_spec(spec: str) -> bool:
    return spec.startswith("meshes:")


@functools.lru_cache(maxsize=64)
def _load_picture(path: str) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))


class MeshSceneDataset(SyntheticSceneDataset):
    def __init__(self, mesh_folder: str, no_objects: int, image_size: Tuple[int, int] = (448, 448), no_points: int = 9, length: int = 64, seed: int = 0,
                 random_crop: bool = True, instances: int = 1, backgrounds: Optional[str] = None, distance: Tuple[float, float] = (650.0, 1100.0)):
        if not 1 <= int(instances) <= 16 or no_objects * int(instances) > 254:
            raise ValueError("instances must lie in 1..16 with no_objects * instances <= 254 (got %d objects, %r instances)" % (no_objects, instances))
        self.folder, self.instances = mesh_folder, int(instances)
        self.oc, self.size, self.kp, self.length, self.seed = no_objects, tuple(image_size), no_points, length, seed
        self.random_crop, self.distance = random_crop, (float(distance[0]), float(distance[1]))
        found = find_meshes(mesh_folder)
        if len(found) < no_objects:
            raise ValueError("%s holds %d meshes, %d objects were asked for" % (mesh_folder, len(found), no_objects))
        self.names = sorted(found)[:no_objects]
        info_file = os.path.join(mesh_folder, "models_info.json")
        info = json.load(open(info_file)) if os.path.isfile(info_file) else None
        command = "python util_scripts/make_keypoints.py --model_folder %s --no_points %d" % (mesh_folder, no_points)
        meshes, colors, kps, diameters = {}, {}, [], []
        for o, stem in enumerate(self.names):
            path = found[stem]
            v, f = read_vertices(path), read_faces(path)
            if len(f) == 0:
                raise ValueError("%s has no faces: a picture needs triangles" % os.path.basename(path))
            kp_file = next((c for c in (os.path.join(mesh_folder, stem, stem + "_keypoints.ply"), os.path.join(os.path.dirname(path), stem + "_keypoints.ply"))
                            if os.path.isfile(c)), None)
            diameter = _existing_entry(info, stem).get("diameter")
            if kp_file is None or diameter is None:
                raise ValueError("%s: %s is missing for %s; write it with `%s`"
                                 % (mesh_folder, stem + "_keypoints.ply" if kp_file is None else "the diameter in models_info.json", stem, command))
            kp = read_vertices(kp_file)
            if len(kp) != no_points:
                raise ValueError("%s holds %d keypoints, no_points is %d; write them again with `%s`" % (os.path.basename(kp_file), len(kp), no_points, command))
            meshes[o], colors[o] = (v, f), read_vertex_colors(path)
            kps.append(kp)
            diameters.append(float(diameter))
        print("meshes: " + ", ".join("object %d = %s (%d triangles, %s)" % (o, s, len(meshes[o][1]), "vertex colours" if colors[o] is not None else "flat colour")
                                     for o, s in enumerate(self.names)))
        rng = np.random.default_rng(seed)
        rng.uniform(35.0, 70.0, (no_objects, 3))                      # SyntheticSceneDataset's stream: its semi-axes come first
        self.colors = rng.uniform(0.15, 0.95, (no_objects, 3))       # the flat colours, as SyntheticSceneDataset.colors
        self.meshes, self.vertex_colors = meshes, colors
        self.keypoints3d = np.stack(kps).astype(np.float64)          # [oc,kp,3]
        self.diameters = np.asarray(diameters, np.float64)
        vmax = max(len(meshes[o][0]) for o in meshes)
        self.mesh_vertex_array = np.zeros((no_objects, vmax, 3))
        for o in meshes:
            self.mesh_vertex_array[o, :len(meshes[o][0])] = meshes[o][0]
        self.mesh_vertex_count = np.array([[len(meshes[o][0])] for o in range(no_objects)], np.int32)
        self.background_files = None
        if backgrounds is not None:
            self.background_files = sorted(os.path.join(backgrounds, n) for n in os.listdir(backgrounds)
                                           if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
            if not self.background_files:
                raise ValueError("%s holds no background pictures (.png, .jpg, .bmp)" % backgrounds)
        self._renderers: Dict[str, ShadedRenderer] = {}
        self._device_scenes: Dict[str, object] = {}

    # ---- one image -----------------------------------------------------------------------------------
    def renderer(self, device=None) -> ShadedRenderer:
        key = "host" if device is None else str(torch.device(device))
        if key not in self._renderers:
            self._renderers[key] = ShadedRenderer(device, self.meshes, self.vertex_colors, {o: self.colors[o] for o in range(self.oc)})
        return self._renderers[key]

    def _background(self, rng) -> np.ndarray:
        """the picture's index, then two uniforms for its crop: resized to cover H x W, cropped there -> uint8 [H, W, 3]"""
        from PIL import Image

        H, W = self.size
        pic = _load_picture(self.background_files[int(rng.integers(0, len(self.background_files)))])
        fy, fx = float(rng.uniform()), float(rng.uniform())
        scale = max(H / pic.shape[0], W / pic.shape[1])
        h, w = max(H, int(round(pic.shape[0] * scale))), max(W, int(round(pic.shape[1] * scale)))
        if (h, w) != pic.shape[:2]:
            pic = np.asarray(Image.fromarray(pic).resize((w, h), Image.BILINEAR))
        y, x = int(fy * (h - H + 1)), int(fx * (w - W + 1))
        return np.ascontiguousarray(pic[min(y, h - H):min(y, h - H) + H, min(x, w - W):min(x, w - W) + W])

    def describe(self, image: int) -> dict:
        """Everything about stream image `image` but its pixels: the draws, the frame for the renderer and the small per-image arrays"""
        oc, I = self.oc, self.instances
        rng = np.random.default_rng([self.seed, int(image)])
        if I > 1:
            hc, wc, inst, poses = self._draw_instances(rng)
            kp2, offsets = self._keypoints_instances(hc, wc, inst, poses)
            small = dict(poses=poses, kp2=kp2, offsets=offsets, instance_count=inst)
        else:
            hc, wc, poses1 = self._draw(rng)
            inst, poses = np.ones(oc, np.int32), poses1[:, None]
            kp2, offsets = self._keypoints(hc, wc, poses1)
            small = dict(poses=poses1, kp2=kp2, offsets=offsets)
        g = rng.normal(size=3)
        light = g / np.linalg.norm(g)
        light[2] = -abs(light[2])
        ambient, diffuse = float(rng.uniform(0.25, 0.5)), float(rng.uniform(0.5, 0.9))
        background = self._background(rng) if self.background_files else None
        seed = int(rng.integers(0, 1 << 63, dtype=np.int64))
        cam = (CAMERA[0, 0], CAMERA[1, 1], CAMERA[0, 2] - wc, CAMERA[1, 2] - hc)   # the camera of the crop
        frame = dict(cam=cam, instances=[(o, o * I + r + 1, poses[o, r]) for o in range(oc) for r in range(int(inst[o]))])
        return dict(frame=frame, light=frame_record(light, ambient, diffuse, seed, hc, wc), background=background, small=small)

    def pack(self, images: Iterable[int]) -> dict:
        """the host half of a batch: MaskRenderer's packed frames, the frame records, the backgrounds and the small arrays"""
        parts = [self.describe(i) for i in images]
        packed = self.renderer(None).masks.pack([p["frame"] for p in parts], self.oc * self.instances)
        background = np.stack([p["background"] for p in parts]) if self.background_files else None
        return dict(packed=packed, lights=np.stack([p["light"] for p in parts]), background=background, small=self._small_arrays([p["small"] for p in parts]))

    def render_twin(self, images: Iterable[int], noise: bool = True, depth: bool = False) -> dict:
        """these stream images through the host twin -> NumPy img, slots (the label map o * I + r + 1), depth, dropped, keys and the host half"""
        H, W = self.size
        host = self.pack(images)
        r, m = self.renderer(None), self.renderer(None).masks
        n = len(host["lights"])
        out = r.call((m.verts, m.vert_counts, m.faces, m.face_counts), r.colors, r.flat, host["packed"], host["lights"], host["background"], noise, n, H, W,
                     NEAR, FAR, 0.5, depth, np.empty(r.workspace_bytes(n, H, W) // 8, np.uint64), None, None)
        return dict(out, slots=out["label"], host=host)

    def batch(self, index: int, batchsize: int, shard: Tuple[int, int] = (0, 1), device=None, noise: bool = True) -> Dict[str, torch.Tensor]:
        """SyntheticSceneDataset.batch over meshes: device=None renders with the host twin (slow, but it needs no GPU), a device with the kernel.
        Both give the same labels, instance_seg, counts, keypoints and poses, and draw the same noise words."""
        from ..parallel import shard_range

        begin, end = shard_range(batchsize, shard[0], shard[1])
        images = range(index * batchsize + begin, index * batchsize + end)
        if device is not None:
            return self.device_scenes(device).render(images, noise)
        out = self.render_twin(images, noise)
        label, iseg = self.split_slots(out["slots"])
        small = out["host"]["small"]
        counts = np.stack([(label == o + 1).reshape(len(label), -1).sum(1) for o in range(self.oc)], 1).astype(np.float32)
        extra = {}
        if self.instances > 1:
            extra = dict(instance_count=small["instance_count"], instance_seg=torch.from_numpy(iseg))
        return dict(
            img=torch.from_numpy(out["img"]),
            target_seg=torch.from_numpy(np.eye(self.oc + 1, dtype=np.float32)[label]),
            keypoints3d=small["keypoints3d"],
            target_vert=small["target_vert"],
            cam_mat=small["cam_mat"],
            diameters=small["diameters"],
            offsets=small["offsets"],
            filtered_seg=torch.from_numpy(label[..., None].astype(np.int32)),
            poses_gt=small["poses_gt"],
            pixel_gt_count=torch.from_numpy(counts[:, :, None, None]),
            **extra,
        )

    def device_scenes(self, device, prefetch: int = 1):
        key = str(torch.device(device))
        if key not in self._device_scenes:
            self._device_scenes[key] = MeshDeviceScenes(self, device, prefetch)
        return self._device_scenes[key]

    def generate_dataset(self, batchsize: int, epochs: int = 1, prefetch: int = 0, *unused, shard: Tuple[int, int] = (0, 1), device=None, **unused_kw):
        """SyntheticSceneDataset.generate_dataset; one line says which source and which renderer serve it.  Without a device the host twin
        renders, unless CASAPOSE_DEVICE_SCENES=1 selects the current GPU."""
        if device is None and from_environment():
            if not torch.cuda.is_available():
                raise RuntimeError("CASAPOSE_DEVICE_SCENES=1 needs a ROCm GPU (unset it for the host twin)")
            device = torch.device("cuda", torch.cuda.current_device())
        print("input: meshes:%s (%d objects, up to %d instances each) rendered by %s"
              % (self.folder, self.oc, self.instances, "the host twin (cp_render_shaded_host_f32)" if device is None else "the device (cp_render_shaded_f32)"))
        if device is None:   # the parent's host loop, without its look at the environment
            n = self.length // batchsize
            return (self.batch(i, batchsize, shard) for _ in range(max(epochs, 1) + 1) for i in range(n)), n
        return super().generate_dataset(batchsize, epochs, prefetch, shard=shard, device=device)


class MeshDeviceScenes(DeviceScenes):
    """DeviceScenes for a MeshSceneDataset: the same side stream, event, prefetch queue and hand-over (batches, render, _launch, _finish); the host
    half packs frames instead of ellipsoid records, and the launch is cp_render_shaded_f32 followed by cp_slot_labels_u8."""

    def __init__(self, ds: MeshSceneDataset, device, prefetch: int = 1):
        self.ds, self.device = ds, torch.device(device)
        self.depth = max(int(prefetch), 1)
        self.stream = None
        self.lib = _lib.load()
        self.instances = ds.instances
        self.slots = ds.oc * ds.instances
        self.renderer = ds.renderer(self.device)
        self.workspace = None   # shared by the launches of the side stream, in stream order

    def host_half(self, images: Iterable[int]) -> dict:
        host = self.ds.pack(images)
        records = {k: torch.from_numpy(a) for k, a in host["packed"].items()}
        records["lights"] = torch.from_numpy(host["lights"])
        if host["background"] is not None:
            records["background"] = torch.from_numpy(host["background"])
        if torch.cuda.is_available():
            records = {k: a.pin_memory() for k, a in records.items()}
        return dict(records=records, small=host["small"])

    def launch_records(self, records: dict, noise: bool = True):
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        dev, st, r, ds = self.device, self.stream, self.renderer, self.ds
        H, W = ds.size
        with torch.cuda.stream(st):
            d = {k: a.to(dev, non_blocking=True) for k, a in records.items()}
            b = d["lights"].shape[0]
            words = r.workspace_bytes(b, H, W) // 8
            if self.workspace is None or self.workspace.numel() < words:
                self.workspace = torch.empty(words, dtype=torch.int64, device=dev)
            raw = r.call(r.masks.d_mesh, r.d_colors, r.d_flat, d, d["lights"], d.get("background"), noise, b, H, W, NEAR, FAR, 0.5, False, self.workspace, dev,
                         st.cuda_stream)
            out = _twin.alloc(dict(label=((b, H, W), np.uint8), instance_seg=((b, H, W), np.uint8), target_seg=((b, H, W, ds.oc + 1), np.float32),
                                   counts=((b, ds.oc), np.int32)), dev)
            _lib.check(self.lib.cp_slot_labels_u8(raw["label"].data_ptr(), b, ds.oc, self.instances, H * W, out["label"].data_ptr(),
                                                  out["instance_seg"].data_ptr(), out["target_seg"].data_ptr(), out["counts"].data_ptr(), st.cuda_stream),
                       "cp_slot_labels_u8")
            counts_host = torch.empty(out["counts"].shape, dtype=torch.int32, pin_memory=True)
            counts_host.copy_(out["counts"], non_blocking=True)
            filtered = out["label"].to(torch.int32).unsqueeze(-1)
            done = torch.cuda.Event()
            done.record(st)
        return dict(out, img=raw["img"], slots=raw["label"], dropped=raw["dropped"], filtered_seg=filtered, counts_host=counts_host, records=d), done


__all__ = ["ShadedRenderer", "MeshSceneDataset", "MeshDeviceScenes", "frame_record", "parse_spec", "is_spec", "FRAME_WORDS", "NEAR", "FAR"]
