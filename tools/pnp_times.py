#!/usr/bin/env python3
"""Times of the PnP step: the host estimate_poses (a Python loop over pnp.pnp) against the device path (DevicePnP, csrc/pnp.hip).

Cases b = 1, oc = 8 and b = 16, oc = 8; nine keypoints per object, 0.5 px noise, every fourth object with one gross outlier, crop offsets given.
Reported, in one process: the host function, the device path end to end through estimate_poses(solver=...) (upload, kernel, download,
synchronise), and the kernel alone by device events.  Every figure is the median of REPEATS windows after a warm-up; the spread (min - max) is
printed beside it."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation import pose_evaluation as E
from casapose_amd.pose_estimation.device_pnp import DevicePnP, affine_from_offsets
if not torch.cuda.is_available():
    raise SystemExit("pnp_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
REPEATS, KP, OC = 7, 9, 8
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)

def make_batch(b, seed):
    rng = np.random.default_rng(seed)
    pts, kp3 = np.zeros((b, OC, KP, 2), np.float32), np.zeros((b, OC, 1, KP, 3), np.float32)
    for n in range(b):
        for o in range(OC):
            X = rng.uniform(-60, 60, (KP, 3)); X[0] = 0
            axis = rng.normal(size=3)
            R, t = P.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.2, 2.8)), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1200)])
            x = P.project(X, K.astype(np.float64), R, t) + 0.5 * rng.normal(size=(KP, 2))
            if o % 4 == 3: x[rng.integers(KP)] += rng.uniform(40, 80) * np.array([1.0, 0.0])
            pts[n, o], kp3[n, o, 0] = x - np.array([240.0, 180.0]), X     # crop pixels of a crop at (w 240, h 180), scale 1
    offs = np.tile(np.array([180.0, 240.0, 0, 0, 0, 0, 0, 1, 640, 480]), (b, 1))
    return pts, kp3, np.ones((b, OC), np.float32), offs

def windows(fn, n, sync=False):
    """median, min, max over REPEATS windows of n calls each, in ms per call (host clock; the window ends in a device synchronise when sync)"""
    fn()
    out = []
    for _ in range(REPEATS):
        if sync: torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n): fn()
        if sync: torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return np.median(out), min(out), max(out)

solver = DevicePnP(dev, KP)
for b in (1, 16):
    pts, kp3, valid, offs = make_batch(b, 1237 + b)
    host = lambda: E.estimate_poses(pts, kp3, K, valid, offs, rng=np.random.default_rng(0))
    device = lambda: E.estimate_poses(pts, kp3, K, valid, offs, solver=solver)
    want, got = host()[0].astype(np.float64), device()[0].astype(np.float64)
    print("b = %d, oc = %d (%d solves, %d hypotheses each):" % (b, OC, b * OC, solver.hypotheses))
    print("  device against host: max |dR| %.3g, max |dt| %.3g mm, statuses %s" % (
        np.abs(got[..., :3] - want[..., :3]).max(), np.abs(got[..., 3] - want[..., 3]).max(), np.unique(solver.last_info[..., 0]).tolist()))
    h = windows(host, 1 if b > 1 else 3)
    d = windows(device, 50, sync=True)
    print("  host estimate_poses:           %9.3f ms per batch  (%.3f - %.3f)" % h)
    print("  device end to end:             %9.3f ms per batch  (%.3f - %.3f)  upload, kernel, download, synchronise" % d)
    xy, x3 = torch.from_numpy(pts).to(dev), torch.from_numpy(np.ascontiguousarray(kp3[:, :, 0])).to(dev)
    Kd, mask, aff = torch.from_numpy(K).to(dev), torch.ones((b, OC), dtype=torch.int32, device=dev), torch.from_numpy(affine_from_offsets(offs)).to(dev)
    poses, info, cost = (torch.empty((b, OC, 3, 4), device=dev), torch.empty((b, OC, 4), dtype=torch.int32, device=dev), torch.empty((b, OC, 2), device=dev))
    def kernel(n=50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): solver.launch(xy, x3, Kd, mask, aff, poses, info, cost)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n
    kernel(5)
    ks = [kernel() for _ in range(REPEATS)]
    print("  device kernel alone (events):  %9.3f ms per batch  (%.3f - %.3f)" % (np.median(ks), min(ks), max(ks)))
    print("  host / device end to end: %.0f x" % (h[0] / d[0]))
