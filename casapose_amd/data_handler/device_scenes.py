"""Device path of SyntheticSceneDataset: the host draws what it draws today (crop origin, poses) and computes the small arrays, the MI355X casts
the rays (csrc/scenes.hip, one launch per batch).

Per image the host half takes `default_rng([seed, image index])` -- the stream of the host path -- through SyntheticSceneDataset._draw, then one
more 63-bit integer from it, the image seed of the device noise, and packs one fp64 record (csrc/scene_math.h): crop origin, camera, image seed,
object count, and per object R, t, 1 / semi-axes, colour.  Labels, poses and keypoints are therefore the host path's; the noise is another sample of
the same distribution, a function of (image seed, pixel) alone, so image i of the stream is the same picture whichever replica, batch size or batch
position renders it.

A side stream copies the records and runs the kernel; an event recorded there is what the consumer's stream waits on.  `batches` keeps up to
max(prefetch, 1) batches in flight, the convention of device_pipeline.DeviceBatches.  The host half of a batch (0.1 ms per image) runs in the
consumer's thread: a background thread for it changed nothing measurable in a training loop.  The batch dict has the keys, shapes and dtypes of the host
path; img / target_seg / filtered_seg are device tensors, pixel_gt_count comes from the kernel's counts, the rest stays on the host as before.

A dataset with an instance axis (SyntheticSceneDataset(instances=I), I > 1) gives the unchanged ray-caster oc * I slots per image, slot o * I + r
being instance r of object o with the object's semi-axes and colour; an absent instance's record is placed behind the camera, where the
ray-caster's `s > 0` never hits it.  The label map that comes back is the slot map (o * I + r + 1: the id convention of instance_voting.py), and
one small pass (cp_slot_labels_u8, csrc/slot_labels.hip) turns it into the class labels, instance_seg, the (oc + 1)-channel one-hot and the
per-object counts.  filtered_seg, instance_seg, instance_count and the small arrays are the host path's byte for byte.
"""
from __future__ import annotations

import collections
from typing import Dict, Iterable, Iterator, List, Tuple

import numpy as np
import torch

from .. import _lib
from .. import twin as _twin   # DeviceScenes.twin is public API
from .synthetic_scene import CAMERA

HEADER, OBJECT = 8, 18   # cp_scene::HEADER / OBJECT of csrc/scene_math.h


class DeviceScenes:
    def __init__(self, ds, device, prefetch: int = 1):
        self.ds, self.device = ds, torch.device(device)
        self.depth = max(int(prefetch), 1)
        self.stream = None   # created by the first launch: the host half needs no GPU
        self.lib = _lib.load()
        self.instances = int(getattr(ds, "instances", 1))
        self.slots = ds.oc * self.instances          # what the ray-caster sees as objects
        self.words = HEADER + OBJECT * self.slots
        if self.lib.cp_render_scenes_record_words(self.slots) != self.words:
            raise _lib.CasaposeHipError("%d objects: the library's scene record has %d words, this binding packs %d"
                                        % (self.slots, self.lib.cp_render_scenes_record_words(self.slots), self.words))

    # ---- host half ----------------------------------------------------------------------------------------------------------------
    def record(self, image: int) -> Tuple[np.ndarray, dict]:
        """(the fp64 record of image `image` of the stream, its small per-image arrays)"""
        ds = self.ds
        rng = np.random.default_rng([ds.seed, int(image)])
        if self.instances > 1:
            return self._record_instances(rng)
        hc, wc, poses = ds._draw(rng)
        seed = int(rng.integers(0, 1 << 63, dtype=np.int64))   # after the pose draws: they stay the host path's
        kp2, offsets = ds._keypoints(hc, wc, poses)
        rec = np.zeros(self.words, np.float64)
        rec[0:6] = hc, wc, CAMERA[0, 0], CAMERA[1, 1], CAMERA[0, 2], CAMERA[1, 2]
        rec[6:7].view(np.uint64)[0] = seed
        rec[7] = ds.oc
        obj = rec[HEADER:].reshape(ds.oc, OBJECT)
        obj[:, 0:9] = poses[:, :, :3].reshape(ds.oc, 9)
        obj[:, 9:12] = poses[:, :, 3]
        obj[:, 12:15] = 1.0 / ds.axes
        obj[:, 15:18] = ds.colors
        return rec, dict(poses=poses, kp2=kp2, offsets=offsets)

    def _record_instances(self, rng) -> Tuple[np.ndarray, dict]:
        """record() with an instance axis: oc * I slots; an absent one sits behind the camera (identity rotation, t_z < 0)"""
        ds, I = self.ds, self.instances
        hc, wc, inst, poses = ds._draw_instances(rng)
        seed = int(rng.integers(0, 1 << 63, dtype=np.int64))   # after the pose draws, as in record()
        kp2, offsets = ds._keypoints_instances(hc, wc, inst, poses)
        rec = np.zeros(self.words, np.float64)
        rec[0:6] = hc, wc, CAMERA[0, 0], CAMERA[1, 1], CAMERA[0, 2], CAMERA[1, 2]
        rec[6:7].view(np.uint64)[0] = seed
        rec[7] = self.slots
        obj = rec[HEADER:].reshape(ds.oc, I, OBJECT)
        there = np.arange(I)[None, :] < inst[:, None]
        obj[..., 0:9] = np.where(there[..., None], poses[..., :3].reshape(ds.oc, I, 9), np.eye(3).reshape(9))
        obj[..., 9:12] = np.where(there[..., None], poses[..., 3], (0.0, 0.0, -1000.0))
        obj[..., 12:15] = (1.0 / ds.axes)[:, None]
        obj[..., 15:18] = ds.colors[:, None]
        return rec, dict(poses=poses, kp2=kp2, offsets=offsets, instance_count=inst)

    def host_half(self, images: Iterable[int]) -> dict:
        """The records [b, words] of these stream images (pinned when a GPU is present) and the host tensors of their batch."""
        parts = [self.record(i) for i in images]
        records = torch.from_numpy(np.stack([r for r, _ in parts]))
        if torch.cuda.is_available():
            records = records.pin_memory()
        return dict(records=records, small=self.ds._small_arrays([s for _, s in parts]))

    def _render(self, records, noise: bool, device, stream) -> dict:
        """cp_render_scenes_f32 on `stream` over device records, or (device None) its host twin over NumPy records: img, label, target_seg, counts"""
        b, oc, (H, W) = records.shape[0], self.ds.oc, self.ds.size
        if self.instances > 1:
            return self._render_instances(records, noise, device, stream)
        out = _twin.alloc(dict(img=((b, H, W, 3), np.float32), label=((b, H, W), np.uint8), target_seg=((b, H, W, oc + 1), np.float32),
                               counts=((b, oc), np.int32)), device)
        _twin.call("cp_render_scenes_f32", records, b, oc, H, W, int(noise), out["img"], out["label"], out["target_seg"], out["counts"],
                   host=device is None, stream=stream)
        return out

    def _render_instances(self, records, noise: bool, device, stream) -> dict:
        """_render with an instance axis: the ray-caster over the slots, then the slot map split into class labels, instance_seg, one-hot and counts
        (cp_slot_labels_u8 on the device; the same integer arithmetic in NumPy for the host twin)"""
        b, oc, S, (H, W) = records.shape[0], self.ds.oc, self.slots, self.ds.size
        raw = _twin.alloc(dict(img=((b, H, W, 3), np.float32), label=((b, H, W), np.uint8), target_seg=((b, H, W, S + 1), np.float32),
                               counts=((b, S), np.int32)), device)
        _twin.call("cp_render_scenes_f32", records, b, S, H, W, int(noise), raw["img"], raw["label"], raw["target_seg"], raw["counts"],
                   host=device is None, stream=stream)
        if device is None:
            label, iseg = self.ds.split_slots(raw["label"])
            counts = np.stack([(label == o + 1).reshape(b, -1).sum(1) for o in range(oc)], 1).astype(np.int32)
            return dict(img=raw["img"], label=label, instance_seg=iseg, target_seg=np.eye(oc + 1, dtype=np.float32)[label], counts=counts, slots=raw["label"])
        out = _twin.alloc(dict(label=((b, H, W), np.uint8), instance_seg=((b, H, W), np.uint8), target_seg=((b, H, W, oc + 1), np.float32),
                               counts=((b, oc), np.int32)), device)
        _lib.check(self.lib.cp_slot_labels_u8(raw["label"].data_ptr(), b, oc, self.instances, H * W, out["label"].data_ptr(), out["instance_seg"].data_ptr(),
                                              out["target_seg"].data_ptr(), out["counts"].data_ptr(), stream), "cp_slot_labels_u8")
        return dict(out, img=raw["img"], slots=raw["label"])

    def twin(self, records: np.ndarray, noise: bool = True) -> Dict[str, np.ndarray]:
        """Host records [b, words] through cp_render_scenes_host_f32, the kernel's host twin (no GPU): img, label, target_seg, counts as NumPy arrays."""
        return self._render(_twin.array(records, np.float64), noise, None, None)

    # ---- device half --------------------------------------------------------------------------------------------------------------
    def launch_records(self, records: torch.Tensor, noise: bool = True) -> Tuple[dict, torch.cuda.Event]:
        """The kernel on the side stream for host records [b, words] -> (device tensors img, label, target_seg, filtered_seg (the labels as int32
        [b, H, W, 1]), counts and the pinned host copy counts_host, the event that follows all of it)."""
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        dev, st = self.device, self.stream
        with torch.cuda.stream(st):
            rec = records.to(dev, non_blocking=True)
            out = self._render(rec, noise, dev, st.cuda_stream)
            counts_host = torch.empty(out["counts"].shape, dtype=torch.int32, pin_memory=True)
            counts_host.copy_(out["counts"], non_blocking=True)
            filtered = out["label"].to(torch.int32).unsqueeze(-1)   # filtered_seg of the batch dict
            done = torch.cuda.Event()
            done.record(st)
        return dict(out, filtered_seg=filtered, counts_host=counts_host, records=rec), done

    def _launch(self, host: dict, noise: bool = True) -> Tuple[dict, torch.cuda.Event]:
        out, done = self.launch_records(host["records"], noise)
        batch = dict(host["small"], img=out["img"], target_seg=out["target_seg"], filtered_seg=out["filtered_seg"])
        if self.instances > 1:
            batch["instance_seg"] = out["instance_seg"]
        return dict(batch=batch, counts_host=out["counts_host"]), done

    def _finish(self, flight: dict, done: torch.cuda.Event) -> Dict[str, torch.Tensor]:
        """Hand a launched batch to the consumer's stream, in the host path's key order."""
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(done)
        batch = flight["batch"]
        for k in ("img", "target_seg", "filtered_seg"):
            batch[k].record_stream(consumer)
        done.synchronize()   # the counts are host data of the batch
        count = flight["counts_host"].to(torch.float32)[:, :, None, None].clone()
        order = ("img", "target_seg", "keypoints3d", "target_vert", "cam_mat", "diameters", "offsets", "filtered_seg", "poses_gt")
        if self.instances > 1:     # the host path's two extra fields, in its order
            batch["instance_seg"].record_stream(consumer)
            return dict([(k, batch[k]) for k in order], pixel_gt_count=count, instance_count=batch["instance_count"], instance_seg=batch["instance_seg"])
        return dict([(k, batch[k]) for k in order], pixel_gt_count=count)

    def render(self, images: Iterable[int], noise: bool = True) -> Dict[str, torch.Tensor]:
        """One batch of these stream images, rendered now."""
        return self._finish(*self._launch(self.host_half(images), noise))

    def batches(self, indices: Iterable[int], batchsize: int, shard: Tuple[int, int] = (0, 1), prefetch: int = None) -> Iterator[Dict[str, torch.Tensor]]:
        """Batch `i` of the stream for every i of `indices`, this shard's slice of it, up to max(prefetch, 1) launched ahead of the consumer."""
        from ..parallel import shard_range

        depth = self.depth if prefetch is None else max(int(prefetch), 1)
        begin, end = shard_range(batchsize, shard[0], shard[1])
        inflight: collections.deque = collections.deque()   # launched on the side stream
        src = iter(indices)
        exhausted = False
        while True:
            while not exhausted and len(inflight) < depth:
                i = next(src, None)
                if i is None:
                    exhausted = True
                    break
                inflight.append(self._launch(self.host_half(range(i * batchsize + begin, i * batchsize + end))))
            if not inflight:
                return
            yield self._finish(*inflight.popleft())


def describe() -> str:
    return "input: synthetic scenes rendered on the device"


def from_environment() -> bool:
    """CASAPOSE_DEVICE_SCENES=1 selects the device path for a `synthetic` source (train_casapose.py, test_casapose.py)."""
    import os

    return os.environ.get("CASAPOSE_DEVICE_SCENES", "0") == "1"


def device_from_environment():
    """For SyntheticSceneDataset.generate_dataset called without a device: None unless CASAPOSE_DEVICE_SCENES=1; then the current GPU, announced
    in one line.  A set variable without a GPU is an error, not the host path."""
    if not from_environment():
        return None
    if not torch.cuda.is_available():
        raise RuntimeError("CASAPOSE_DEVICE_SCENES=1 needs a ROCm GPU (unset it for the host renderer)")
    print(describe())
    return torch.device("cuda", torch.cuda.current_device())


__all__: List[str] = ["DeviceScenes", "describe", "from_environment", "device_from_environment"]
