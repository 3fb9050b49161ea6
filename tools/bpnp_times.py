#!/usr/bin/env python3
"""Times of the BPnP keypoint loss: the host path training.bpnp_reprojection_loss_host (a Python loop over the pairs) against the device call
(DeviceBPnPLoss, csrc/bpnp.hip: both launches, by device events), on the same coordinates in one process.

Cases: 15 pairs (b = 3, oc = 5), 128 (b = 16, oc = 8) and 416 (b = 32, oc = 13); nine keypoints, 0.5 px noise, every fourth object with one gross
outlier, ground truth 2 px away.  The device figure is the median of REPEATS windows of 20 calls after a warm-up, with the spread (min - max);
the host figure is wall clock (one call for the large cases: it takes seconds).  With --train-step: one train_step of the factory model at
64 x 64 (k = 5, b = 2) with use_bpnp_reprojection_loss, by wall clock around synchronised steps, under whatever CASAPOSE_DEVICE_BPNP says."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from casapose_amd import training as TR
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation.device_bpnp import DeviceBPnPLoss
if not torch.cuda.is_available():
    raise SystemExit("bpnp_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
REPEATS, KP, CAP = 7, 9, 12.5
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)

def make_batch(b, oc, seed):
    rng = np.random.default_rng(seed)
    yx, gt, x3 = np.zeros((b, oc, KP, 2), np.float32), np.zeros((b, oc, KP, 2), np.float32), np.zeros((b, oc, KP, 3), np.float32)
    for n in range(b):
        for o in range(oc):
            X = rng.uniform(-60, 60, (KP, 3)); X[0] = 0
            X = X.astype(np.float32)
            axis = rng.normal(size=3)
            R, t = P.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.2, 2.8)), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1200)])
            x = P.project(X.astype(np.float64), K.astype(np.float64), R, t) + 0.5 * rng.normal(size=(KP, 2))
            gt[n, o] = x + 2.0 * rng.normal(size=(KP, 2))
            if o % 4 == 3: x[rng.integers(KP)] += rng.uniform(40, 80) * np.array([1.0, 0.0])
            yx[n, o], x3[n, o] = (x - np.array([240.0, 180.0]))[:, ::-1], X     # crop pixels of a crop at (w 240, h 180), scale 1
    aff = np.tile(np.float32([1, 0, 240, 0, 1, 180]), (b, 1))
    return yx, gt, aff, np.ones((b, oc), np.float32), x3

def train_step_times():
    from types import SimpleNamespace
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler
    b, h, w, k = 2, 64, 64, 5
    rng = np.random.default_rng(3)
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=k, input_shape=(h, w, 3), input_segmentation_shape=(h, w, k), weights=None,
                                             base_model="resnet18", device=dev, seed=3)
    lab = np.zeros((b, h, w), np.int64)
    for o in range(1, k): lab[:, 8 + 12 * (o - 1):20 + 12 * (o - 1), 8:56] = o
    cam = np.array([[100.0, 0, 32.0], [0, 100.0, 32.0], [0, 0, 1]])
    p3d = rng.uniform(-20, 20, (b, k - 1, 1, KP, 3))
    poses = np.zeros((b, k - 1, 1, 3, 4)); poses[..., :3, :3] = np.eye(3); poses[..., 2, 3] = 100.0
    cam3 = p3d.reshape(b, k - 1, 1, KP, 3) + np.array([0, 0, 100.0])
    xy = cam3[..., :2] / cam3[..., 2:] * 100.0 + 32.0
    batch = dict(img=torch.from_numpy(rng.uniform(-1, 1, (b, h, w, 3)).astype(np.float32)), target_seg=torch.from_numpy(np.eye(k, dtype=np.float32)[lab]),
                 keypoints3d=torch.from_numpy(p3d), target_vert=torch.from_numpy(xy[..., ::-1].copy()), cam_mat=torch.from_numpy(cam),
                 offsets=torch.from_numpy(np.tile(np.array([[0.0, 0, 0, 0, 0, 0, 0, 1, 64, 64]]), (b, 1))), poses_gt=torch.from_numpy(poses))
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=True, max_keypoint_pixel_error=CAP, confidence_regularization=True,
                          use_bpnp_reprojection_loss=True)
    lf, optim = LossWeightHandler(1.0, 0.5, 0.015, 0.007, filter_vertex_with_segmentation=True), TR.Adam(learning_rate=1e-3)
    import warnings
    warnings.simplefilter("ignore", UserWarning)
    for _ in range(3): TR.train_step(net, batch, lf, optim, opt)
    out = []
    for _ in range(REPEATS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5): TR.train_step(net, batch, lf, optim, opt)
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3 / 5)
    plan, _ = net.training_plan(b, h, w, None, 1)
    print("train_step, k = 5, 64 x 64, b = 2, 8 pairs, CASAPOSE_DEVICE_BPNP=%s: %.2f ms per step (%.2f - %.2f); unsolved pairs so far %d"
          % (os.environ.get("CASAPOSE_DEVICE_BPNP", "unset"), np.median(out), min(out), max(out), plan.bpnp_unsolved))

if "--train-step" in sys.argv:
    train_step_times()
    raise SystemExit(0)
loss_fn = DeviceBPnPLoss(dev, KP)
for b, oc in ((3, 5), (16, 8), (32, 13)):
    yx, gt, aff, avail, x3 = make_batch(b, oc, 4000 + b)
    t0 = time.perf_counter()
    want = TR.bpnp_reprojection_loss_host(yx, gt, aff, avail, x3, K, CAP, 1.0, rng=np.random.default_rng(0))
    host_ms = (time.perf_counter() - t0) * 1e3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    c, g_, a_, av, p3, Kd = (up(v) for v in (yx, gt, aff, avail, x3, K))
    g, loss = torch.empty((b, oc, KP, 2), device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    poses, info, counts = torch.empty((b, oc, 1, 3, 4), device=dev), torch.empty((b, oc, 4), dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(loss_fn.workspace_bytes(b, oc) // 8, dtype=torch.float64, device=dev)
    def call(n=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): loss_fn.launch(c, g_, a_, av, p3, Kd, CAP, 1.0, g, loss, poses, info, counts, ws)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n
    call(3)
    ks = [call() for _ in range(REPEATS)]
    gm = np.abs(want[1]).reshape(b * oc, -1).max(axis=1)
    rel = (np.abs(g.cpu().numpy().astype(np.float64) - want[1]).reshape(b * oc, -1).max(axis=1) / gm).max()
    print("%3d pairs (b = %d, oc = %d): host path %9.1f ms (wall clock, one call); device call %7.3f ms (%.3f - %.3f); host / device %.0f x; "
          "counts %s, max |dg| / max|g| of the pair %.3g, relative loss difference %.3g"
          % (b * oc, b, oc, host_ms, np.median(ks), min(ks), max(ks), host_ms / np.median(ks), counts.cpu().tolist(), rel, abs(loss.item() - want[0]) / want[0]))
