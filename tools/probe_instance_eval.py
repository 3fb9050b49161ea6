#!/usr/bin/env python3
"""Times of the instance evaluator (cp_pose_match_f32, csrc/pose_match.hip) on one MI355X, by device events after a warm-up.

Workload: batch 16, 8 objects with the vertex counts of tools/eval_times.py (two of them symmetric: 7862 and 3417), every group with I
ground-truth instances and R = I non-empty estimates.  Two steps, each a process of its own, meant to run under its own `timeout` and chained
with `&&`:

    timeout -k 10 300 python tools/probe_instance_eval.py match 1 >> profiles/instance_eval_probe.txt &&
    timeout -k 10 300 python tools/probe_instance_eval.py match 2 >> profiles/instance_eval_probe.txt &&
    timeout -k 10 300 python tools/probe_instance_eval.py match 4 >> profiles/instance_eval_probe.txt &&
    timeout -k 10 300 python tools/probe_instance_eval.py eval <the parent commit's libcasapose_hip.so> >> profiles/instance_eval_probe.txt

match R: the new call against cp_pose_eval_f32 run over the same R x R (estimate, instance) pairs written out one by one -- R x R calls of
  batch 16, the only way the library could compute the matrix before -- with the objects' flags as they are and with every flag cleared (ADD
  only: what is left is the share of the ADD-S walks).  The two paths' errors are compared bit for bit first.
eval LIB: cp_pose_eval_f32 on its own workload (batch 16, one estimate per object) from this build and from LIB (the library built from the
  parent commit, tools/build_variant.sh or a checkout of it), alternating, with the records compared bit for bit.
Every figure is the median of REPEATS windows of CALLS calls; the spread (min - max) is printed beside it."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from casapose_amd import _lib  # noqa: E402
from casapose_amd.pose_estimation import pnp as P  # noqa: E402
from casapose_amd.pose_estimation.instance_evaluation import DeviceInstanceEvaluator  # noqa: E402

COUNTS = np.array([5841, 38325, 7862, 3417, 12655, 18995, 22831, 7912], np.int32)   # 7862 / 3417 real, the rest invented (tools/eval_times.py)
FLAGS = [int(c in (7862, 3417)) for c in COUNTS]
BATCH, REPEATS, CALLS = 16, 7, 20
K = np.array([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0], np.float32)


def scene(side, seed=1237):
    """mesh [oc, vmax, 3], gt and est [BATCH, oc, side, 12]: estimates a few millimetres and degrees off their own instance"""
    rng = np.random.default_rng(seed)
    oc, vmax = len(COUNTS), int(COUNTS.max())
    mesh = np.zeros((oc, vmax, 3), np.float32)
    for o, c in enumerate(COUNTS):
        mesh[o, :c] = rng.uniform(-50, 50, (c, 3))
    gt, est = np.zeros((BATCH, oc, side, 3, 4), np.float32), np.zeros((BATCH, oc, side, 3, 4), np.float32)
    for idx in np.ndindex(BATCH, oc, side):
        R, t = P.rodrigues(rng.normal(0, 0.6, 3)), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(700, 1100)])
        gt[idx] = np.concatenate([R, t[:, None]], 1)
        est[idx] = np.concatenate([R @ P.rodrigues(rng.normal(0, 0.05, 3)), t[:, None] + rng.normal(0, 2.0, (3, 1))], 1)
    return mesh, gt.reshape(BATCH, oc, side, 12), est.reshape(BATCH, oc, side, 12)


def windows(launch):
    """(median, min, max) ms per call over REPEATS windows of CALLS calls, by device events, after a warm-up window"""
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS
    window()
    out = [window() for _ in range(REPEATS)]
    return float(np.median(out)), min(out), max(out)


class PoseEval:
    """cp_pose_eval_f32 of a library (this build's, or another file's) over pre-packed device pair buffers"""

    def __init__(self, lib, dev, mesh, flags):
        self.lib, self.dev = lib, dev
        self.oc, self.vmax = mesh.shape[0], mesh.shape[1]
        self.points = torch.tensor(mesh).to(dev)
        self.counts = torch.tensor(COUNTS).to(dev)
        self.flags = torch.tensor(np.asarray(flags, np.int32)).to(dev)
        self.workspace = torch.empty(lib.cp_pose_eval_workspace_bytes(BATCH, self.oc, self.vmax) // 8, dtype=torch.float64, device=dev)
        self.records = torch.empty((BATCH * self.oc, 6), dtype=torch.float32, device=dev)

    def pairs(self, est, gt):
        """est, gt [BATCH, oc, 12] -> the packed device records [BATCH * oc, 36]"""
        rec = np.zeros((BATCH, self.oc, 36), np.float32)
        rec[..., 0:12], rec[..., 12:24], rec[..., 24:33], rec[..., 33], rec[..., 34] = est, gt, K, 120.0, 1.0
        return torch.tensor(rec.reshape(-1, 36)).to(self.dev)

    def launch(self, pairs, records=None):
        records = self.records if records is None else records
        status = self.lib.cp_pose_eval_f32(self.points.data_ptr(), self.counts.data_ptr(), self.flags.data_ptr(), self.oc, self.vmax, pairs.data_ptr(), BATCH,
                                           5.0, self.workspace.data_ptr(), records.data_ptr(), None, None, torch.cuda.current_stream(self.dev).cuda_stream)
        if status != 0:
            raise _lib.CasaposeHipError("cp_pose_eval_f32 failed (%d)" % status)


def step_match(side, dev):
    mesh, gt, est = scene(side)
    lib = _lib.load()
    print("match R = I = %d: batch %d, vertex counts %s, ADD-S for %s" % (side, BATCH, COUNTS.tolist(), [int(c) for c, f in zip(COUNTS, FLAGS) if f]))
    for flags, name in ((FLAGS, "flags as they are"), ([0] * len(COUNTS), "every flag cleared (ADD only)")):
        ev = DeviceInstanceEvaluator(mesh, COUNTS, dev, symmetric=flags)
        up = [torch.tensor(a).to(dev) for a in (est, gt, np.full((BATCH, len(COUNTS)), side, np.int32), np.tile(K, (BATCH, 1)), np.full(len(COUNTS), 120.0, np.float32))]
        old = PoseEval(lib, dev, mesh, flags)
        pair_sets = [[old.pairs(est[:, :, e], gt[:, :, g]) for g in range(side)] for e in range(side)]
        err = ev.launch(*up, BATCH, side, side, 5.0)[0].cpu().numpy()
        same = True
        for e in range(side):
            for g in range(side):
                old.launch(pair_sets[e][g])
                same &= np.array_equal(old.records.cpu().numpy()[:, :2].view(np.uint32), err[:, :, e, g].reshape(-1, 2).view(np.uint32))
        new = windows(lambda: ev.launch(*up, BATCH, side, side, 5.0))
        one = windows(lambda: [old.launch(p) for row in pair_sets for p in row])
        print("  %-30s errors bit-identical to the pairwise calls: %s" % (name + ":", same))
        print("    cp_pose_match_f32, one call:          %8.3f ms  (%.3f - %.3f)" % new)
        print("    cp_pose_eval_f32, %2d calls of batch %d: %8.3f ms  (%.3f - %.3f)   ratio %.2f" % ((side * side, BATCH) + one + (one[0] / new[0],)))


def step_eval(path, dev):
    mesh, gt, est = scene(1)
    ours = _lib.load()
    other = C.CDLL(path)
    for name, restype, argtypes in _lib.SYMBOLS:
        if name in ("cp_pose_eval_f32", "cp_pose_eval_workspace_bytes"):
            getattr(other, name).restype, getattr(other, name).argtypes = restype, argtypes
    a, b = PoseEval(ours, dev, mesh, FLAGS), PoseEval(other, dev, mesh, FLAGS)
    pairs = a.pairs(est[:, :, 0], gt[:, :, 0])
    ra, rb = torch.empty_like(a.records), torch.empty_like(a.records)
    a.launch(pairs, ra)
    b.launch(pairs, rb)
    torch.cuda.synchronize(dev)
    print("eval: cp_pose_eval_f32, batch %d, one estimate per object; records bit-identical between the two libraries: %s" % (
        BATCH, np.array_equal(ra.cpu().numpy().view(np.uint32), rb.cpu().numpy().view(np.uint32))))
    for round_ in range(3):     # alternating: this build, the other library, this build, ...
        ta, tb = windows(lambda: a.launch(pairs)), windows(lambda: b.launch(pairs))
        print("  round %d: this build %8.3f ms  (%.3f - %.3f)    parent library %8.3f ms  (%.3f - %.3f)" % ((round_,) + ta + tb))


def main(argv):
    if len(argv) != 2 or argv[0] not in ("match", "eval"):
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("probe_instance_eval.py needs a ROCm GPU: a CPU run gives no device time")
    dev = torch.device("cuda:0")
    if argv[0] == "match":
        step_match(int(argv[1]), dev)
    else:
        step_eval(argv[1], dev)


if __name__ == "__main__":
    main(sys.argv[1:])
