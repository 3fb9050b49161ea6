#!/usr/bin/env python3
"""Times of the uncertainty PnP's two device pieces, each beside the call it extends:

  1. cp_kp_cov_seeded_f32 beside cp_ransac_vote_seeded_f32 at the bench's voting shape (16 images, 480 x 640, 8 objects, hyp 512), on one input;
  2. cp_pnp_weighted_f64 beside cp_pnp_f64 for 128 pairs (b = 16, oc = 8, nine keypoints).

The two calls of a pair alternate in one process; every figure is the median of REPEATS windows of device-event time after a warm-up, with the
spread (min - max) beside it.  The voter synchronises the stream inside its call after rounds 1, 2, 4, ...: its event time includes that."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from casapose_amd import _lib
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation.device_pnp import DevicePnP
if not torch.cuda.is_available():
    raise SystemExit("kp_covariance_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
lib = _lib.load()
REPEATS, CALLS = 9, 10
stream = torch.cuda.current_stream(dev).cuda_stream


def alternate(fa, fb):
    """(median, min, max) ms per call of fa and of fb: REPEATS windows of CALLS calls each, a, b, a, b, ..., timed by device events"""
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPEATS):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) / CALLS)
    return tuple((float(np.median(t)), min(t), max(t)) for t in (ta, tb))


# ---- 1. the voting shape: 8 rectangular objects per image, directions at nine keypoints with 0.1 rad of angular noise and 20 % outliers ----------
B, H, W, OC, KP, HYP = 16, 480, 640, 8, 9, 512
rng = np.random.default_rng(0)
labels = np.zeros((B, H, W), np.uint8)
field = np.zeros((B, H, W, 2 * KP), np.float32)
for b in range(B):
    for o in range(OC):
        y0, x0 = 20 + 110 * (o // 4) + int(rng.integers(0, 20)), 10 + 155 * (o % 4) + int(rng.integers(0, 20))
        rows, cols = int(rng.integers(60, 100)), int(rng.integers(80, 140))
        labels[b, y0:y0 + rows, x0:x0 + cols] = o + 1
        ys, xs = np.nonzero(labels[b] == o + 1)
        kp = np.stack([rng.uniform(x0, x0 + cols, KP), rng.uniform(y0, y0 + rows, KP)], 1)
        ang = np.arctan2(kp[None, :, 1] - (ys[:, None] + 0.5), kp[None, :, 0] - (xs[:, None] + 0.5)) + rng.normal(0, 0.1, (ys.size, KP))
        ang = np.where(rng.uniform(size=ang.shape) < 0.2, rng.uniform(-np.pi, np.pi, ang.shape), ang)
        field[b, ys, xs] = np.stack([np.sin(ang), np.cos(ang)], -1).reshape(ys.size, 2 * KP)
lab, fld = torch.from_numpy(labels).to(dev), torch.from_numpy(field).to(dev)
ws = torch.empty(max(lib.cp_ransac_workspace_bytes(B, H, W, OC, KP, HYP), lib.cp_kp_cov_workspace_bytes(B, H, W, OC, KP, HYP)), dtype=torch.uint8, device=dev)
pts = torch.empty(B, OC, KP, 2, dtype=torch.float32, device=dev)
rounds = torch.empty(B, OC, dtype=torch.int32, device=dev)
cov = torch.empty(B, OC, KP, 3, dtype=torch.float32, device=dev)
wsum = torch.empty(B, OC, KP, dtype=torch.int32, device=dev)
head = (lab.data_ptr(), fld.data_ptr(), 2 * KP, 0, B, H, W, OC, KP)


def vote():
    _lib.check(lib.cp_ransac_vote_seeded_f32(*head, 7, HYP, 0.99, 0.99, 20, 20, 30000, ws.data_ptr(), pts.data_ptr(), rounds.data_ptr(), stream), "vote")


def covariance():
    _lib.check(lib.cp_kp_cov_seeded_f32(*head, pts.data_ptr(), 7, HYP, 0.99, 20, 30000, ws.data_ptr(), cov.data_ptr(), wsum.data_ptr(), stream), "kp_cov")


vote(); covariance()
torch.cuda.synchronize()
print("voting shape: %d images %d x %d, %d objects, hyp %d; pixels per object %d..%d; voting rounds %s; median sqrt(trace cov) %.3f px" % (
    B, H, W, OC, HYP, min((labels == o + 1).sum(axis=(1, 2)).min() for o in range(OC)), max((labels == o + 1).sum(axis=(1, 2)).max() for o in range(OC)),
    np.unique(rounds.cpu().numpy()).tolist(), float(torch.sqrt(cov[..., 0] + cov[..., 2]).median())))
tv, tc = alternate(vote, covariance)
print("  cp_ransac_vote_seeded_f32: %8.3f ms per call  (%.3f - %.3f)" % tv)
print("  cp_kp_cov_seeded_f32:      %8.3f ms per call  (%.3f - %.3f)" % tc)

# ---- 2. 128 pairs: nine keypoints, three with an 8 x 0.5 px ellipse, six at 0.3 px ---------------------------------------------------------------
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
b, oc = 16, 8
xy, x3, cv = np.zeros((b, oc, KP, 2), np.float32), np.zeros((b, oc, KP, 3), np.float32), np.zeros((b, oc, KP, 3), np.float32)
for n in range(b):
    for o in range(oc):
        X = rng.uniform(-60, 60, (KP, 3)); X[0] = 0
        axis = rng.normal(size=3)
        R, t = P.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.2, 2.8)), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1200)])
        th = rng.uniform(0, np.pi, KP)
        s0, s1 = np.where(np.arange(KP) < 3, 8.0, 0.3), np.where(np.arange(KP) < 3, 0.5, 0.3)
        e = np.stack([s0, s1], 1) * rng.normal(size=(KP, 2))
        c, s = np.cos(th), np.sin(th)
        xy[n, o] = P.project(X, K.astype(np.float64), R, t) + np.stack([c * e[:, 0] - s * e[:, 1], s * e[:, 0] + c * e[:, 1]], 1)
        x3[n, o] = X
        cv[n, o] = np.stack([c * c * s0 ** 2 + s * s * s1 ** 2, c * s * (s0 ** 2 - s1 ** 2), s * s * s0 ** 2 + c * c * s1 ** 2], 1)
solver = DevicePnP(dev, KP)
d = [torch.from_numpy(a).to(dev) for a in (xy, x3, K, cv)]
mask = torch.ones((b, oc), dtype=torch.int32, device=dev)
poses = torch.empty(b, oc, 3, 4, dtype=torch.float32, device=dev)
info = torch.empty(b, oc, 4, dtype=torch.int32, device=dev)
cost = torch.empty(b, oc, 2, dtype=torch.float32, device=dev)
weighted = torch.empty(b, oc, dtype=torch.int32, device=dev)
plain = lambda: solver._call(d[0], d[1], d[2], mask, None, poses, info, cost, False)
weigh = lambda: solver._call(d[0], d[1], d[2], mask, None, poses, info, cost, False, d[3], 0.0, weighted)
weigh()
torch.cuda.synchronize()
print("%d pairs, %d hypotheses each: statuses %s, weighted %d, LM iterations %s" % (b * oc, solver.hypotheses, np.unique(info[..., 0].cpu().numpy()).tolist(),
                                                                              int(weighted.sum()), np.unique(info[..., 3].cpu().numpy()).tolist()))
tp, tw = alternate(plain, weigh)
print("  cp_pnp_f64:          %8.3f ms per call  (%.3f - %.3f)" % tp)
print("  cp_pnp_weighted_f64: %8.3f ms per call  (%.3f - %.3f)" % tw)
