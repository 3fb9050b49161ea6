#!/usr/bin/env python3
"""Times of the built-in synthetic scenes: the host path (SyntheticSceneDataset.batch: NumPy fp64 ray casting, one image at a time) against the
device path (DeviceScenes, csrc/scenes.hip) in one process, the two alternating.

Cases: a batch of 32 at 448 x 448 with 8 objects, and one image at 480 x 640 with 13 objects.  Per round: one host batch by wall clock; then
the device launch (records to the device, the kernel, the counts back) by device events over CALLS calls, and the whole device batch
(`batch(..., device=)`: host half, launch, label conversion, counts) by wall clock around a synchronise.  Medians over ROUNDS rounds with the spread
(min - max).  With --train-step: images/s of training.train_step at 448 x 448, 8 objects, batch 32, fed a fresh batch every step by either path."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
if not torch.cuda.is_available():
    raise SystemExit("scene_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
ROUNDS, CALLS = 3, 20
spread = lambda v: "%.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))  # noqa: E731

def batch_times():
    for bs, size, oc in ((32, (448, 448), 8), (1, (480, 640), 13)):
        ds = SyntheticSceneDataset(oc, size, seed=1)
        scenes = ds.device_scenes(dev)
        host = scenes.host_half(range(bs))
        for _ in range(3): ds.batch(0, bs, device=dev)
        torch.cuda.synchronize()
        host_s, launch_ms, batch_ms, half_ms = [], [], [], []
        for r in range(ROUNDS):
            t0 = time.perf_counter(); ds.batch(r, bs); host_s.append(time.perf_counter() - t0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(scenes.stream):
                e0.record()
                for _ in range(CALLS): scenes.launch_records(host["records"])
                e1.record()
            e1.synchronize(); launch_ms.append(e0.elapsed_time(e1) / CALLS)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(CALLS): ds.batch(r * CALLS + i, bs, device=dev)
            torch.cuda.synchronize(); batch_ms.append((time.perf_counter() - t0) * 1e3 / CALLS)
            t0 = time.perf_counter()
            for i in range(CALLS): scenes.host_half(range(i * bs, (i + 1) * bs))
            half_ms.append((time.perf_counter() - t0) * 1e3 / CALLS)
        px = bs * size[0] * size[1]
        print("bs %2d, %d x %d, %2d objects: host path %s s per batch; device launch %s ms by device events (%.1f GB/s of output); device batch end to end "
              "%s ms, of which the host half %s ms; host / device batch %.0f x"
              % (bs, size[0], size[1], oc, spread(host_s), spread(launch_ms), px * (12 + 1 + 4 * (oc + 1)) / np.median(launch_ms) / 1e6, spread(batch_ms),
                 spread(half_ms), np.median(host_s) * 1e3 / np.median(batch_ms)))

def train_step_times():
    from types import SimpleNamespace
    from casapose_amd import training as TR
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler
    oc, (H, W), bs = 8, (448, 448), 32
    ds = SyntheticSceneDataset(oc, (H, W), length=1 << 20, seed=1)
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=oc + 1, input_shape=(H, W, 3), input_segmentation_shape=(H, W, oc + 1), weights=None,
                                             base_model="resnet18", device=dev, seed=3)
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=True, max_keypoint_pixel_error=12.5, confidence_regularization=True,
                          use_bpnp_reprojection_loss=False)
    lf, optim = LossWeightHandler(1.0, 0.5, 0.015, 0.007, filter_vertex_with_segmentation=True), TR.Adam(learning_rate=1e-3)
    feeds = {"host": (ds.generate_dataset(bs)[0], 2), "device": (ds.generate_dataset(bs, device=dev, prefetch=2)[0], 20)}
    for name in feeds: TR.train_step(net, next(feeds[name][0]), lf, optim, opt)
    rates = {"host": [], "device": []}
    for _ in range(ROUNDS):
        for name, (it, steps) in feeds.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps): TR.train_step(net, next(it), lf, optim, opt)
            torch.cuda.synchronize(); rates[name].append(steps * bs / (time.perf_counter() - t0))
    print("train_step, 448 x 448, 8 objects, batch 32, a fresh batch every step: host-fed %s images/s, device-fed %s images/s" % (spread(rates["host"]), spread(rates["device"])))

if "--train-step" in sys.argv:
    train_step_times()
else:
    batch_times()
