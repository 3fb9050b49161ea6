#!/usr/bin/env python3
"""Times of the pose statistics for one image: the host evaluate_poses against the device path (DevicePoseEvaluator, csrc/pose_eval.hip).

b = 1, oc = 8, random meshes.  Of the vertex counts only 7862 and 3417 (the two ADD-S meshes) are known from the code; the other six are
invented stand-ins for the LM evaluation meshes.  Reported, in one process: the host function alone (with and without the np.tile of the mesh
array that evaluate_pose_estimates does first), the device path end to end (pack, upload, two kernels, download, synchronise), and the two
kernels alone by device events.  Every figure is the median of REPEATS windows after a warm-up; the spread (min - max) is printed beside it."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation import pose_evaluation as E
from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator
if not torch.cuda.is_available():
    raise SystemExit("eval_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
COUNTS = np.array([5841, 38325, 7862, 3417, 12655, 18995, 22831, 7912], np.int32)   # 7862 / 3417 real, the rest invented
REPEATS = 7
rng = np.random.default_rng(1237)
oc, vmax = len(COUNTS), int(COUNTS.max())
mesh = np.zeros((oc, vmax, 3), np.float32)
for o, c in enumerate(COUNTS):
    mesh[o, :c] = rng.uniform(-50, 50, (c, 3))
gt, est = np.zeros((1, oc, 1, 3, 4), np.float32), np.zeros((1, oc, 3, 4), np.float32)
for o in range(oc):
    R, t = P.rodrigues(rng.normal(0, 0.6, 3)), np.array([rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(750, 850)])
    gt[0, o, 0] = np.concatenate([R, t[:, None]], 1)
    est[0, o] = np.concatenate([R @ P.rodrigues(np.array([0.05, -0.03, 0.1])), t[:, None] + [[1.0], [-0.5], [2.0]]], 1)
K = np.array([[[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]]], np.float32)
diam, valid, counts = np.full((1, oc, 1), 120.0, np.float32), np.ones((1, oc), np.float32), COUNTS.reshape(oc, 1)

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

pts, cnt = E._eval_points(None, mesh, counts, 1, oc, 1)
host = lambda: E.evaluate_poses(est, gt, None, pts, cnt, K, diam, valid, 5.0)
print("vertex counts %s (7862 and 3417 are the code's ADD-S meshes; the others are invented)" % COUNTS.tolist())
print("host evaluate_poses:            %8.3f ms per image  (%.3f - %.3f)" % windows(host, 3))
print("host np.tile of the mesh array: %8.3f ms per image  (%.3f - %.3f)" % windows(lambda: E._eval_points(None, mesh, counts, 1, oc, 1), 3))
ev = DevicePoseEvaluator(mesh, counts, dev)
want, got = host(), ev.evaluate(est, gt, K, diam, valid)
print("device against host: max |err_2d| diff %.3g px, max |err_3d| diff %.3g mm, flags equal: %s" % (
    np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max(), all(np.array_equal(got[i], want[i]) for i in (2, 3, 4, 5, 6))))
print("device end to end:              %8.3f ms per image  (%.3f - %.3f)  pack, upload, two kernels, download, synchronise" %
      windows(lambda: ev.evaluate(est, gt, K, diam, valid), 200, sync=True))
def kernels(n=200):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): ev.launch(1, 5.0)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n
kernels(20)
ks = [kernels() for _ in range(REPEATS)]
pairs = int((COUNTS[2].astype(np.int64) ** 2 + COUNTS[3].astype(np.int64) ** 2))
print("device kernels alone (events):  %8.3f ms per image  (%.3f - %.3f)  %.1f M point pairs of ADD-S -> %.2f T pairs/s" % (
    np.median(ks), min(ks), max(ks), pairs / 1e6, pairs / np.median(ks) / 1e9))
