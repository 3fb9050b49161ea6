"""Device path of VectorfieldDataset.generate_dataset: the host draws (crop, pose geometry, colour / imgaug parameters) and decodes, the MI355X
does every per-pixel step (csrc/augment.hip).

Per batch: `workers` threads decode the PNGs with PIL into one pinned uint8 buffer (rgb) and one for the segmentation, and fill one
cp_aug_image per image; a side stream copies them to the device and runs geometry (A), the imgaug program (B, use_imgaug only), resize and
the float tail (C); an event recorded there is what the consumer's stream waits on.  Up to max(prefetch, 1) batches are in flight: host
preparation of the next batches runs in the background while the device works on the current one.  The batch dict has the keys, shapes
and dtypes of the host path; img / target_seg / filtered_seg are device tensors, the rest stay on the host as before.
"""
from __future__ import annotations

import collections
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterator, List, Tuple

import numpy as np
import torch

from .. import _lib
from . import augment


def _decode(item, color_input: bool):
    from PIL import Image

    img = Image.open(item[0])
    # grayscale sources are read as L and replicated to three channels: the host path repeats its one channel at the end
    img = img.convert("RGB") if color_input else img.convert("L").convert("RGB")
    seg = Image.open(item[3]).convert("L")
    return np.asarray(img, np.uint8), np.asarray(seg, np.uint8)


class DeviceBatches:
    def __init__(self, ds, device, imagesize, cropratio, workers: int, prefetch: int):
        self.ds, self.device = ds, torch.device(device)
        self.imagesize, self.cropratio = (int(imagesize[0]), int(imagesize[1])), cropratio
        self.pool = ThreadPoolExecutor(max(int(workers), 1))
        self.batch_pool = ThreadPoolExecutor(1)
        self.depth = max(int(prefetch), 1)
        self.stream = None   # created by batches(): the host half (draws, packing) needs no GPU
        self.lib = _lib.load()

    # ---- host half ----------------------------------------------------------------------------------------------------------------
    def _image(self, epoch: int, i: int, order_groups) -> Tuple[dict, "_lib.AugImage", Tuple[np.ndarray, np.ndarray]]:
        from PIL import Image

        ds = self.ds
        rng = np.random.default_rng([ds.seed, 2, epoch, int(i)])   # the reader's rule: the draws of image i in epoch e
        item = ds.imgs[i]
        with Image.open(item[0]) as im:
            width, height = im.size
        data = ds.load_json_minimal(item[2])
        data["_img_path"] = item[1]
        saved, ds.rng = ds.rng, rng
        try:
            geo = ds.draw_geometry(width, height, self.imagesize, self.cropratio)
            ann, remap = ds.annotations(data, item[4], geo)
            if ds.use_imgaug:
                prog = augment.sample_program(rng, order_groups, geo["out_h"], geo["out_w"])
                bright, contrast = 0.0, 1.0
                sigma = float(rng.uniform(0, ds.noise)) if ds.noise else 0.0
            else:
                prog = None
                bright, contrast, sigma = ds.draw_photometric()
        finally:
            ds.rng = saved
        p = _lib.AugImage()
        p.seed = int(rng.integers(0, 1 << 63, dtype=np.int64))
        p.src_h, p.src_w = height, width
        p.crop_x, p.crop_y = geo["w_crop"], geo["h_crop"]
        p.warp = int(bool(geo["dx"] or geo["dy"] or geo["angle"]))
        for k in range(6):
            p.affine[k] = float(geo["affine"][k])
        p.brightness, p.contrast, p.noise_sigma = bright, contrast, sigma
        for sid, lab in remap.items():
            p.label_map[sid] = lab
        if prog is not None:
            augment.pack_image(p, prog.ops, prog)
        pix = self.pool.submit(_decode, item, ds.color_input)
        return ann, p, pix

    def _prepare(self, epoch: int, b: int, indices) -> dict:
        order_groups = augment.group_order(self.ds.seed, epoch, b)
        parts = [self._image(epoch, i, order_groups) for i in indices]
        decoded = [pix.result() for _, _, pix in parts]
        total = sum(s.shape[0] * s.shape[1] for _, s in decoded)
        rgb = torch.empty(3 * total, dtype=torch.uint8, pin_memory=True)
        seg = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        rgb_np, seg_np = rgb.numpy(), seg.numpy()
        off = 0
        for (ann, p, _), (im, sg) in zip(parts, decoded):
            h, w = sg.shape
            if im.shape[:2] != (h, w) or (p.src_h, p.src_w) != (h, w):
                raise ValueError("%s: image and segmentation sizes differ" % ann["image_id"])
            rgb_np[3 * off:3 * (off + h * w)] = im.reshape(-1)
            seg_np[off:off + h * w] = sg.reshape(-1)
            p.src_offset = off
            off += h * w
        n = len(parts)
        progs = torch.empty(n * C.sizeof(_lib.AugImage), dtype=torch.uint8, pin_memory=True)
        for k, (_, p, _) in enumerate(parts):
            C.memmove(progs.data_ptr() + k * C.sizeof(_lib.AugImage), C.addressof(p), C.sizeof(_lib.AugImage))
        anns = [a for a, _, _ in parts]
        crops = {(int(a["offsets"][2]), int(a["offsets"][3])) for a in anns}
        if len(crops) != 1:
            raise ValueError("images of one batch have different crop sizes %s (source frames of different heights)" % sorted(crops))
        crop = crops.pop()
        return dict(rgb=rgb, seg=seg, progs=progs, anns=anns, crop=crop, any_contrast=any(p.contrast != 1.0 for _, p, _ in parts))

    # ---- device half --------------------------------------------------------------------------------------------------------------
    def _launch(self, host: dict) -> Tuple[dict, torch.cuda.Event]:
        lib, dev, st = self.lib, self.device, self.stream
        n, (ch, cw), (H, W) = len(host["anns"]), host["crop"], self.imagesize
        oc = len(self.ds.objectsofinterest)
        s = st.cuda_stream
        with torch.cuda.stream(st):
            rgb = host["rgb"].to(dev, non_blocking=True)
            seg = host["seg"].to(dev, non_blocking=True)
            progs = host["progs"].to(dev, non_blocking=True)
            crop_rgb = torch.empty((n, ch, cw, 3), dtype=torch.uint8, device=dev)
            crop_lab = torch.empty((n, ch, cw), dtype=torch.uint8, device=dev)
            _lib.check(lib.cp_aug_geometry(rgb.data_ptr(), seg.data_ptr(), progs.data_ptr(), n, ch, cw, crop_rgb.data_ptr(), crop_lab.data_ptr(), s),
                       "cp_aug_geometry")
            if self.ds.use_imgaug:
                photo = torch.empty_like(crop_rgb)
                _lib.check(lib.cp_aug_photometric(crop_rgb.data_ptr(), progs.data_ptr(), n, ch, cw, 0, photo.data_ptr(), s), "cp_aug_photometric")
                crop_rgb = photo
            if (ch, cw) != (H, W):
                out_rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
                out_lab = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
                _lib.check(lib.cp_aug_resize(crop_rgb.data_ptr(), crop_lab.data_ptr(), n, ch, cw, H, W, out_rgb.data_ptr(), out_lab.data_ptr(), s),
                           "cp_aug_resize")
                crop_rgb, crop_lab = out_rgb, out_lab
            sums = None
            if host["any_contrast"]:
                sums = torch.empty(3 * n, dtype=torch.int32, device=dev)
                _lib.check(lib.cp_aug_channel_sums(crop_rgb.data_ptr(), n, H * W, sums.data_ptr(), s), "cp_aug_channel_sums")
            img = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
            filtered = torch.empty((n, H, W, 1), dtype=torch.int32, device=dev)
            target = torch.empty((n, H, W, oc + 1), dtype=torch.float32, device=dev)
            _lib.check(lib.cp_aug_finish(crop_rgb.data_ptr(), crop_lab.data_ptr(), progs.data_ptr(), None if sums is None else sums.data_ptr(), n, H, W,
                                         oc + 1, img.data_ptr(), filtered.data_ptr(), target.data_ptr(), s), "cp_aug_finish")
            done = torch.cuda.Event()
            done.record(st)
        anns = host["anns"]
        st_ = lambda k: torch.from_numpy(np.stack([a[k] for a in anns]))  # noqa: E731
        batch = dict(img=img, target_seg=target, target_vert=st_("target_vert"), keypoints3d=st_("keypoints3d"), cam_mat=st_("cam_mat"),
                     diameters=st_("diameters"), offsets=st_("offsets"), filtered_seg=filtered, cuboid3d=st_("cuboid3d"), poses_gt=st_("poses_gt"),
                     pixel_gt_count=st_("pixel_gt_count"), image_id=[a["image_id"] for a in anns])
        return batch, done

    def jobs(self, epochs: int, epoch_batches: int, data_size: int, batchsize: int, begin: int, end: int, shuffle: bool):
        """(epoch, batch, image indices of this shard), in the reader's order"""
        ds = self.ds
        for epoch in range(max(int(epochs), 1)):
            order = ds.order_rng.permutation(data_size) if shuffle else np.arange(data_size)
            for b in range(epoch_batches):
                yield epoch, b, order[b * batchsize + begin:b * batchsize + end]

    def batches(self, epochs: int, epoch_batches: int, data_size: int, batchsize: int, begin: int, end: int, shuffle: bool) -> Iterator[Dict]:
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        pending: collections.deque = collections.deque()   # host preparation running in the background
        inflight: collections.deque = collections.deque()  # launched on the side stream
        src = self.jobs(epochs, epoch_batches, data_size, batchsize, begin, end, shuffle)
        exhausted = False
        while True:
            while not exhausted and len(pending) + len(inflight) < 2 * self.depth:
                job = next(src, None)
                if job is None:
                    exhausted = True
                    break
                pending.append(self.batch_pool.submit(self._prepare, *job))
            while pending and len(inflight) < self.depth:
                inflight.append(self._launch(pending.popleft().result()))
            if not inflight:
                return
            batch, done = inflight.popleft()
            consumer = torch.cuda.current_stream(self.device)
            consumer.wait_event(done)
            for k in ("img", "target_seg", "filtered_seg"):
                batch[k].record_stream(consumer)
            yield batch


def device_batches(ds, device, batchsize, epochs, prefetch, imagesize, cropratio, workers, shard, shuffle=True
                   ) -> Tuple[Iterator[Dict[str, torch.Tensor]], int]:
    from ..parallel import shard_range

    data_size = len(ds.imgs) - (len(ds.imgs) % batchsize)
    epoch_batches = data_size // batchsize
    begin, end = shard_range(batchsize, shard[0], shard[1])
    db = DeviceBatches(ds, device, imagesize, cropratio, workers, prefetch)
    return db.batches(epochs, epoch_batches, data_size, batchsize, begin, end, shuffle), epoch_batches


def describe(ds) -> str:
    return "device input pipeline (%s)" % ("imgaug sequence on the device" if ds.use_imgaug else "brightness / contrast, use_imgaug off")


__all__: List[str] = ["DeviceBatches", "device_batches", "describe"]
