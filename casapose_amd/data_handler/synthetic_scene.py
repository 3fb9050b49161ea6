"""A self-contained stand-in for the NDDS/BOP image source of the reference (VectorfieldDataset,
casapose/data_handler/vectorfield_dataset.py): ray-cast scenes of textured ellipsoids with analytic ground truth,
delivered as the SAME batch tuple the training / evaluation steps consume (train_casapose.py:496-507):

    img [B,H,W,3] in [-1,1], target_seg [B,H,W,K] one-hot, keypoints3d [B,oc,1,kp,3], target_vert [B,oc,1,kp,2] 2-D
    keypoints (y,x) in crop pixels, cam_mat [B,3,3], diameters [B,oc,1], offsets [B,10], filtered_seg [B,H,W,1] label
    map, poses_gt [B,oc,1,3,4], pixel_gt_count [B,oc]

There is no dataset on this machine (no network); this generator is what `--data synthetic[:N]` selects in
train_casapose.py / test_casapose.py so that the whole config-driven pipeline (losses, voting, PnP, ADD metrics, CSV
logs) runs end to end with ground truth that is exact by construction.  The NDDS reader itself is the next row of
SURVEY 8(f).

Geometry: object o is the ellipsoid x^2/a^2 + y^2/b^2 + z^2/c^2 = 1 in its own frame; its 9 keypoints are the centre and
the 8 corners of its bounding box (the reference's farthest-point keypoints are likewise spread over the object); the
evaluation mesh is a Fibonacci sampling of the surface.  A camera with the LINEMOD intrinsics renders 480x640; crops
follow the reference's offsets convention [h_crop, w_crop, -, -, dx, dy, angle, scale, 640, 480].

The pictures are ray-cast here in NumPy fp64, one image at a time; `batch(..., device=)` / `generate_dataset(..., device=)` hand the per-pixel part
to the GPU instead (device_scenes.py, csrc/scenes.hip): the same draws, labels, poses and keypoints, other noise samples of the same distribution.

Several instances of one object (`instances=I`, 2..16; the reference's max_instance_count, vectorfield_dataset.py:378-410,452-479): per image and
object a count n in 1..I is drawn and n ellipsoids of that object -- the same semi-axes and colour -- are posed and rendered; the nearest hit
wins, as between objects.  The draws of one image, in order: the crop origin; then per object its count n, then per present instance z, u, v and
the rotation (a stream of its own: it does not relate to the stream of instances=1).  The batch then carries the reference's instance axis:
target_vert [B,oc,I,kp,2], keypoints3d [B,oc,I,kp,3], poses_gt [B,oc,I,3,4], diameters [B,oc,I], absent instances padded as the reference's reader
pads them (keypoints -1000, pose 0, diameter -1; :458-470), and two fields more: instance_count int32 [B,oc] and instance_seg uint8 [B,H,W], the
instance index of the visible hit (0 on background).  target_seg / filtered_seg stay CLASS labels, pixel_gt_count is per object, summed over its
instances.  With instances=1 every draw and every byte of every batch is what it was.
"""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

CAMERA = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
FULL_H, FULL_W = 480, 640


def _rot(rng) -> np.ndarray:
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _fibonacci_sphere(n: int) -> np.ndarray:
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


class SyntheticSceneDataset:
    distance = (650.0, 1100.0)   # the range an instance's depth is drawn from, mm (MeshSceneDataset sets its own)

    def __init__(self, no_objects: int, image_size: Tuple[int, int] = (448, 448), no_points: int = 9, length: int = 64, seed: int = 0,
                 mesh_vertices: int = 642, random_crop: bool = True, instances: int = 1):
        if no_points != 9:
            raise ValueError("the synthetic scene defines 9 keypoints per object (centre + bounding-box corners)")
        if not 1 <= int(instances) <= 16 or no_objects * int(instances) > 254:
            raise ValueError("instances must lie in 1..16 with no_objects * instances <= 254 (got %d objects, %r instances)" % (no_objects, instances))
        self.instances = int(instances)
        self.oc, self.size, self.kp, self.length, self.seed = no_objects, tuple(image_size), no_points, length, seed
        self.random_crop = random_crop
        rng = np.random.default_rng(seed)
        self.axes = rng.uniform(35.0, 70.0, (no_objects, 3))                      # semi-axes, mm
        self.colors = rng.uniform(0.15, 0.95, (no_objects, 3))
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
        self.keypoints3d = np.concatenate([np.zeros((no_objects, 1, 3)), corners[None] * self.axes[:, None, :]], axis=1)  # [oc,9,3]
        sph = _fibonacci_sphere(mesh_vertices)
        self.mesh_vertex_array = sph[None] * self.axes[:, None, :]                  # [oc,V,3]
        self.mesh_vertex_count = np.full((no_objects, 1), mesh_vertices, np.int32)
        self.diameters = 2.0 * self.axes.max(axis=1)                                 # largest vertex distance
        self._device_scenes: Dict[str, object] = {}

    def __len__(self):
        return self.length

    # ---- one image ------------------------------------------------------------------------------------
    def _draw(self, rng) -> Tuple[int, int, np.ndarray]:
        """The draws of one image, in this order: the crop origin, then per object z, u, v and the rotation -> (hc, wc, poses [oc,3,4])."""
        oc = self.oc
        H, W = self.size
        if (H, W) == (FULL_H, FULL_W):
            hc, wc = 0, 0
        elif self.random_crop:
            hc, wc = int(rng.integers(0, FULL_H - H + 1)), int(rng.integers(0, FULL_W - W + 1))
        else:
            hc, wc = (FULL_H - H) // 2, (FULL_W - W) // 2
        K = CAMERA
        # poses: centres spread over the crop, in front of the camera
        poses = np.zeros((oc, 3, 4))
        for o in range(oc):
            z = rng.uniform(*self.distance)
            u = rng.uniform(wc + 0.12 * W, wc + 0.88 * W)
            v = rng.uniform(hc + 0.12 * H, hc + 0.88 * H)
            poses[o, :, :3] = _rot(rng)
            poses[o, :, 3] = [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
        return hc, wc, poses

    def _draw_instances(self, rng) -> Tuple[int, int, np.ndarray, np.ndarray]:
        """The draws of one image with an instance axis, in this order: the crop origin, then per object the count n in 1..I and, per present
        instance, z, u, v and the rotation -> (hc, wc, counts [oc] int32, poses [oc,I,3,4]; absent instances zero)."""
        oc, I = self.oc, self.instances
        H, W = self.size
        if (H, W) == (FULL_H, FULL_W):
            hc, wc = 0, 0
        elif self.random_crop:
            hc, wc = int(rng.integers(0, FULL_H - H + 1)), int(rng.integers(0, FULL_W - W + 1))
        else:
            hc, wc = (FULL_H - H) // 2, (FULL_W - W) // 2
        K = CAMERA
        counts = np.zeros(oc, np.int32)
        poses = np.zeros((oc, I, 3, 4))
        for o in range(oc):
            counts[o] = int(rng.integers(1, I + 1))
            for r in range(counts[o]):
                z = rng.uniform(*self.distance)
                u = rng.uniform(wc + 0.12 * W, wc + 0.88 * W)
                v = rng.uniform(hc + 0.12 * H, hc + 0.88 * H)
                poses[o, r, :, :3] = _rot(rng)
                poses[o, r, :, 3] = [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
        return hc, wc, counts, poses

    def _pixels(self, rng, hc: int, wc: int, poses: np.ndarray, noise: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """The per-pixel part of one image -> (img [H,W,3] float64 in [-1,1], label [H,W] uint8).  With noise it draws N(0, 0.02) for the background
        and then N(0, 0.01) for every pixel from `rng`; without, it draws nothing.  csrc/scene_math.h restates this function."""
        return self._cast(rng, hc, wc, poses, self.axes, self.colors, None, noise)

    def _cast(self, rng, hc: int, wc: int, poses: np.ndarray, axes: np.ndarray, colors: np.ndarray, present, noise: bool) -> Tuple[np.ndarray, np.ndarray]:
        """_pixels over a list of ellipsoids (poses [S,3,4], axes / colors [S,3]; present [S] bool or None = all): the label is the 1-based index of the
        nearest hit in that list.  One object per entry is _pixels; with an instance axis entry (o * I + r) is instance r of object o."""
        oc = poses.shape[0]
        H, W = self.size
        K = CAMERA
        # ray casting on the crop
        ys, xs = np.mgrid[hc:hc + H, wc:wc + W].astype(np.float64) + 0.5
        rays = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)  # camera frame
        depth = np.full((H, W), np.inf)
        label = np.zeros((H, W), np.uint8)
        shade = np.zeros((H, W))
        for o in range(oc):
            if present is not None and not present[o]:
                continue
            R, t = poses[o, :, :3], poses[o, :, 3]
            inv = 1.0 / axes[o]
            d = (rays @ R) * inv           # ray direction in the unit-sphere frame (R^T r, scaled)
            c = (-(R.T @ t)) * inv         # camera centre in that frame
            a = (d * d).sum(-1)
            bq = (d * c).sum(-1)
            cq = c @ c - 1.0
            disc = bq * bq - a * cq
            hit = disc > 0
            s = np.where(hit, (-bq - np.sqrt(np.where(hit, disc, 0.0))) / a, np.inf)  # ray parameter = depth (r_z = 1)
            nearer = hit & (s > 0) & (s < depth)
            nrm = (c + d * s[..., None])                                                 # unit-sphere normal
            depth = np.where(nearer, s, depth)
            label = np.where(nearer, o + 1, label).astype(np.uint8)
            shade = np.where(nearer, 0.55 + 0.45 * np.abs(nrm[..., 2]), shade)
        img = np.empty((H, W, 3))
        bg = 0.35 + 0.1 * np.sin(xs / 37.0)[..., None] * np.cos(ys / 53.0)[..., None]
        if noise:
            bg = bg + rng.normal(0, 0.02, (H, W, 3))
        col = np.concatenate([np.zeros((1, 3)), colors])[label]
        img[:] = np.where(label[..., None] > 0, col * shade[..., None], bg)
        if noise:
            img = img + rng.normal(0, 0.01, img.shape)
        img = np.clip(img, 0, 1) * 2.0 - 1.0        # normal = [0.5, 0.5] -> [-1, 1]
        return img, label

    def _keypoints(self, hc: int, wc: int, poses: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(kp2 [oc,kp,2]: the 2-D keypoints in crop pixels (y,x), offsets [10])"""
        oc = self.oc
        K = CAMERA
        kp2 = np.zeros((oc, self.kp, 2))
        for o in range(oc):
            cam = self.keypoints3d[o] @ poses[o, :, :3].T + poses[o, :, 3]
            uv = (cam @ K.T)
            uv = uv[:, :2] / uv[:, 2:]
            kp2[o, :, 0], kp2[o, :, 1] = uv[:, 1] - hc, uv[:, 0] - wc
        return kp2, np.array([hc, wc, 0, 0, 0, 0, 0, 1, FULL_W, FULL_H], np.float32)

    def _keypoints_instances(self, hc: int, wc: int, counts: np.ndarray, poses: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(kp2 [oc,I,kp,2]: the 2-D keypoints in crop pixels (y,x), -1000 for absent instances; offsets [10])"""
        K = CAMERA
        kp2 = np.full((self.oc, self.instances, self.kp, 2), -1000.0)
        for o in range(self.oc):
            for r in range(counts[o]):
                cam = self.keypoints3d[o] @ poses[o, r, :, :3].T + poses[o, r, :, 3]
                uv = (cam @ K.T)
                uv = uv[:, :2] / uv[:, 2:]
                kp2[o, r, :, 0], kp2[o, r, :, 1] = uv[:, 1] - hc, uv[:, 0] - wc
        return kp2, np.array([hc, wc, 0, 0, 0, 0, 0, 1, FULL_W, FULL_H], np.float32)

    def split_slots(self, slots: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """slot map (o * I + r + 1, 0 = background: the id convention of pose_estimation/instance_voting.py) -> (class labels, instance_seg), uint8"""
        s = slots.astype(np.int64)
        on = s > 0
        return np.where(on, (s - 1) // self.instances + 1, 0).astype(np.uint8), np.where(on, (s - 1) % self.instances, 0).astype(np.uint8)

    def _render_instances(self, rng, noise: bool = True) -> Dict[str, np.ndarray]:
        oc, I = self.oc, self.instances
        hc, wc, inst, poses = self._draw_instances(rng)
        present = (np.arange(I)[None, :] < inst[:, None]).reshape(-1)
        img, slots = self._cast(rng, hc, wc, poses.reshape(oc * I, 3, 4), np.repeat(self.axes, I, axis=0), np.repeat(self.colors, I, axis=0), present, noise)
        label, iseg = self.split_slots(slots)
        kp2, offsets = self._keypoints_instances(hc, wc, inst, poses)
        counts = np.array([(label == o + 1).sum() for o in range(oc)], np.int32)
        return dict(img=img.astype(np.float32), label=label, instance_seg=iseg, instance_count=inst, poses=poses, kp2=kp2, counts=counts, offsets=offsets)

    def _render(self, rng, noise: bool = True) -> Dict[str, np.ndarray]:
        if self.instances > 1:
            return self._render_instances(rng, noise)
        oc = self.oc
        hc, wc, poses = self._draw(rng)
        img, label = self._pixels(rng, hc, wc, poses, noise)
        kp2, offsets = self._keypoints(hc, wc, poses)
        counts = np.array([(label == o + 1).sum() for o in range(oc)], np.int32)
        return dict(img=img.astype(np.float32), label=label, poses=poses, kp2=kp2, counts=counts, offsets=offsets)

    def _small_arrays(self, items) -> Dict[str, torch.Tensor]:
        """The batch entries that do not depend on pixels, from per-image dicts with "kp2", "offsets" and "poses"."""
        b = len(items)
        if self.instances > 1:       # the instance axis; absent instances padded as the reference's reader pads them
            inst = np.stack([it["instance_count"] for it in items]).astype(np.int32)                       # [b,oc]
            there = np.arange(self.instances)[None, None, :] < inst[:, :, None]                            # [b,oc,I]
            k3 = np.where(there[..., None, None], self.keypoints3d[None, :, None], -1000.0)
            return dict(
                keypoints3d=torch.from_numpy(k3.astype(np.float32)),
                target_vert=torch.from_numpy(np.stack([it["kp2"] for it in items]).astype(np.float32)),
                cam_mat=torch.from_numpy(np.tile(CAMERA[None], (b, 1, 1)).astype(np.float32)),
                diameters=torch.from_numpy(np.where(there, self.diameters[None, :, None], -1.0).astype(np.float32)),
                offsets=torch.from_numpy(np.stack([it["offsets"] for it in items])),
                poses_gt=torch.from_numpy(np.stack([it["poses"] for it in items]).astype(np.float32)),
                instance_count=torch.from_numpy(inst),
            )
        return dict(
            keypoints3d=torch.from_numpy(np.tile(self.keypoints3d[None, :, None], (b, 1, 1, 1, 1)).astype(np.float32)),
            target_vert=torch.from_numpy(np.stack([it["kp2"] for it in items])[:, :, None].astype(np.float32)),
            cam_mat=torch.from_numpy(np.tile(CAMERA[None], (b, 1, 1)).astype(np.float32)),
            diameters=torch.from_numpy(np.tile(self.diameters[None, :, None, None], (b, 1, 1, 1)).astype(np.float32)),
            offsets=torch.from_numpy(np.stack([it["offsets"] for it in items])),
            poses_gt=torch.from_numpy(np.stack([it["poses"] for it in items])[:, :, None].astype(np.float32)),
        )

    def device_scenes(self, device, prefetch: int = 1):
        """The DeviceScenes (device_scenes.py) that renders this dataset on `device`, built on first use and kept."""
        from .device_scenes import DeviceScenes

        key = str(torch.device(device))
        if key not in self._device_scenes:
            self._device_scenes[key] = DeviceScenes(self, device, prefetch)
        return self._device_scenes[key]

    def batch(self, index: int, batchsize: int, shard: Tuple[int, int] = (0, 1), device=None) -> Dict[str, torch.Tensor]:
        """Deterministic batch `index` (images index*batchsize ... of the endless stream seeded by `seed`).  `shard = (rank, world)`
        renders only that replica's contiguous slice of the global batch (casapose_amd.parallel.shard_range) -- image i of the
        stream is the same picture whichever replica draws it.  With a `device` the pixels are rendered there (device_scenes.py): the same
        labels, poses and keypoints, other noise samples of the same distribution; img / target_seg / filtered_seg are device tensors."""
        from ..parallel import shard_range

        begin, end = shard_range(batchsize, shard[0], shard[1])
        if device is not None:
            return self.device_scenes(device).render(range(index * batchsize + begin, index * batchsize + end))
        items = [self._render(np.random.default_rng([self.seed, index * batchsize + i])) for i in range(begin, end)]
        K1 = self.oc + 1
        lab = np.stack([it["label"] for it in items])
        seg = np.eye(K1, dtype=np.float32)[lab]
        small = self._small_arrays(items)
        extra = {}
        if self.instances > 1:
            extra = dict(instance_count=small["instance_count"], instance_seg=torch.from_numpy(np.stack([it["instance_seg"] for it in items])))
        return dict(
            img=torch.from_numpy(np.stack([it["img"] for it in items])),
            target_seg=torch.from_numpy(seg),
            keypoints3d=small["keypoints3d"],
            target_vert=small["target_vert"],
            cam_mat=small["cam_mat"],
            diameters=small["diameters"],
            offsets=small["offsets"],
            filtered_seg=torch.from_numpy(lab[..., None].astype(np.int32)),
            poses_gt=small["poses_gt"],
            pixel_gt_count=torch.from_numpy(np.stack([it["counts"] for it in items]).astype(np.float32)[:, :, None, None]),
            **extra,
        )

    def generate_object_vertex_array(self):
        """(vertex_array [oc,V,3], vertex_count [oc,1]) like VectorfieldDataset.generate_object_vertex_array."""
        return self.mesh_vertex_array.astype(np.float32), self.mesh_vertex_count

    def generate_dataset(self, batchsize: int, epochs: int = 1, prefetch: int = 0, *_unused, shard: Tuple[int, int] = (0, 1), device=None,
                         **_unused_kw) -> Tuple[Iterator[Dict[str, torch.Tensor]], int]:
        """(iterator over epochs*batches batches, batches per epoch) -- the shape of VectorfieldDataset.generate_dataset
        (vectorfield_dataset.py:905-1013).  The same `length` images are revisited every epoch.  `batchsize` is the GLOBAL batch
        (vectorfield_dataset.py:923,1002); with shard = (rank, world) every replica produces only its own slice of each batch.  With a
        `device` the batches are rendered there, up to max(prefetch, 1) of them ahead of the consumer (device_scenes.py).  A caller that
        names no device gets the host path, unless CASAPOSE_DEVICE_SCENES=1 is set: then the current GPU renders, and one line says so
        (test_casapose.py, which passes no device, is switched this way)."""
        if device is None:
            from . import device_scenes

            device = device_scenes.device_from_environment()
        n = self.length // batchsize

        def indices():
            for _ in range(max(epochs, 1) + 1):
                for i in range(n):
                    yield i

        if device is not None:
            return self.device_scenes(device, prefetch).batches(indices(), batchsize, shard, prefetch), n
        return (self.batch(i, batchsize, shard) for i in indices()), n
