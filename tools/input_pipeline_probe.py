#!/usr/bin/env python3
"""Input-pipeline probe: writes an NDDS folder (write_ndds_scene, 640x480 frames) and measures the device path of
VectorfieldDataset.generate_dataset at config_8 sizes (crop 448 -> 448^2).

    python tools/input_pipeline_probe.py [--images 64] [--batch 32] [--workers 8] [--out input_probe.json]

Reports, as one JSON line (and into --out):
  gpu_ms_per_batch_{plain,imgaug}_incl_h2d  device time of one batch: host-to-device copies + A+B+C (device events on the side stream)
  host_ms_per_image_decode / _rest host clock: PIL decode of one image / everything else the host does per image (draws, annotations, packing)
  images_per_s_workers<N>          images per second delivered by the iterator (host clock, each batch synchronised)
Without a GPU only the host numbers are measured."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from casapose_amd.data_handler import augment  # noqa: E402
from casapose_amd.data_handler.device_pipeline import DeviceBatches, _decode  # noqa: E402
from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset  # noqa: E402
from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset, write_ndds_scene  # noqa: E402

NAMES = ["obj_000001", "obj_000005", "obj_000006", "obj_000008", "obj_000009", "obj_000010", "obj_000011", "obj_000012"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    scene = SyntheticSceneDataset(len(NAMES), (480, 640), length=a.images, seed=3)
    write_ndds_scene(os.path.join(tmp, "data"), os.path.join(tmp, "models"), scene, a.images, NAMES)
    size, crop = (448, 448), 0.933333333

    def ds(imgaug):
        return VectorfieldDataset(root=os.path.join(tmp, "data"), path_meshes=os.path.join(tmp, "models"), color_input=True, objectsofinterest=NAMES,
                                  seed=1, noise=0.0001, brightness=0.001, contrast=0.001, random_translation=(0, 0), random_rotation=0,
                                  use_imgaug=imgaug)

    res = {"images": a.images, "batch": a.batch, "frame": [480, 640], "crop": 448, "imagesize": list(size)}
    # host: decode vs the rest, per image
    d = ds(True)
    db = DeviceBatches(d, "cpu", size, crop, 1, 1)
    order = augment.group_order(d.seed, 0, 0)
    t0 = time.perf_counter()
    for i in range(a.images):
        _decode(d.imgs[i], True)
    res["host_ms_per_image_decode"] = (time.perf_counter() - t0) * 1e3 / a.images
    db.pool.shutdown()
    db.pool = type("Inline", (), {"submit": staticmethod(lambda f, *x: type("F", (), {"result": staticmethod(lambda: None)}))})()
    t0 = time.perf_counter()
    for i in range(a.images):
        db._image(0, i, order)
    res["host_ms_per_image_rest_imgaug"] = (time.perf_counter() - t0) * 1e3 / a.images
    if not torch.cuda.is_available():
        print(json.dumps(res))
        return
    dev = torch.device("cuda:0")
    for name, imgaug in (("plain", False), ("imgaug", True)):
        d = ds(imgaug)
        db = DeviceBatches(d, dev, size, crop, a.workers, 2)
        db.stream = torch.cuda.Stream(device=dev)
        host = [db._prepare(0, b, np.arange(b * a.batch, (b + 1) * a.batch) % a.images) for b in range(4)]
        times = []
        for rep in range(12):
            h = host[rep % 4]
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(db.stream)
            db._launch(h)
            end.record(db.stream)
            torch.cuda.synchronize()
            times.append(start.elapsed_time(end))
        res["gpu_ms_per_batch_%s_incl_h2d" % name] = float(np.median(times[2:]))
        # images/s through the iterator, workers threads decoding
        it, nb = d.generate_dataset(a.batch, 3, prefetch=2, imagesize=size, cropratio=crop, worker=a.workers, device=dev)
        next(it)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        for batch in it:
            torch.cuda.synchronize()
            n += batch["img"].shape[0]
        res["images_per_s_workers%d_%s" % (a.workers, name)] = n / (time.perf_counter() - t0)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
