#!/usr/bin/env python3
"""Times of the BOP error kernels (cp_bop_errors_f32, csrc/bop_errors.hip) on a seeded synthetic load of the size a user would run: 8 objects of
8 000 - 20 000 vertices, half of them with 315 or 630 symmetry transforms, 2 000 (estimate, ground-truth instance) pairs.

    python tools/bop_score_probe.py [--out profiles/bop_score_probe.json] [--pairs 2000] [--slice 50]

A GPU tool; it reads nothing outside the tree.  Reported, each named for what it is:
  device time per call     both kernels, from device events around repeated launches after a warm-up, over a window of at least half a second
  evaluations per second   point-symmetry evaluations the definition needs (sum over pairs of vertices x symmetries) over that time
  share of the VALU rate   the VALU instructions the kernel issues for the shapes -- its steps of 1024 vertices x 16 symmetries, padding
                           included, at VALU_PER_STEP instructions per thread and step, counted in the compiled loop -- over the time, against
                           256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz
  NumPy baseline           the wall time of tests/bop_reference.py (fp64) on the first `slice` pairs, scaled by evaluations to the whole load: the
                           parent of this kernel is no kernel
It also asserts that the device errors of the slice equal the reference within the gates of tests/test_gpu_bop_scores.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bop_reference as B  # noqa: E402
from casapose_amd.pose_estimation import pnp as P  # noqa: E402
from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer, pack_bop_pairs, symmetry_transforms  # noqa: E402

VALU_PER_STEP = 2336          # v_* instructions in bop_max_kernel's loop body (one step: 4 vertices x 16 symmetries per thread), from the ISA
VALU_LANES_PER_SECOND = 256 * 4 * 32 * 2.4e9
K32 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)


def build_load(pairs, seed=1237):
    rng = np.random.default_rng(seed)
    counts = rng.integers(8000, 20001, 8)
    flip = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    cont = [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]
    entries = [{"symmetries_continuous": cont}, {}, {"symmetries_discrete": [flip], "symmetries_continuous": cont}, {"symmetries_discrete": [flip]},
               {"symmetries_continuous": cont}, {}, {"symmetries_discrete": [flip], "symmetries_continuous": cont}, {}]
    syms = [symmetry_transforms(e) for e in entries]
    mesh = np.zeros((8, int(counts.max()), 3), np.float32)
    for o, c in enumerate(counts):
        a, r = rng.uniform(0, 2 * np.pi, c), rng.uniform(20, 80, c)          # a solid of revolution, about: radius up to 80 mm
        mesh[o, :c] = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-60, 60, c)], axis=1)
    obj = rng.integers(0, 8, pairs)
    gt, est = np.zeros((pairs, 3, 4), np.float32), np.zeros((pairs, 3, 4), np.float32)
    for p in range(pairs):
        R, t = P.rodrigues(rng.normal(0, 0.6, 3)), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(700, 1500)])
        gt[p] = np.concatenate([R, t[:, None]], 1)
        turn = P.rodrigues(np.array([0.0, 0.0, rng.uniform(0, 2 * np.pi)])) @ P.rodrigues(rng.normal(0, 0.03, 3))
        est[p] = np.concatenate([R @ turn, (t + rng.normal(0, 3.0, 3))[:, None]], 1)
    return mesh, counts, syms, obj, est, gt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--slice", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bop_score_probe.py needs a ROCm GPU: a CPU run gives no device time")
    dev = torch.device("cuda:0")
    mesh, counts, syms, obj, est, gt = build_load(a.pairs)
    scorer = DeviceBopScorer(mesh, counts, syms, dev)
    T, G = scorer._lib.cp_bop_errors_tile(), scorer._lib.cp_bop_errors_sym_group()
    sc = scorer.sym_counts_host.astype(np.int64)
    useful = int((counts[obj].astype(np.int64) * sc[obj]).sum())
    steps = int(((-(-counts[obj].astype(np.int64) // T)) * (-(-sc[obj] // G))).sum())        # block steps: 256 threads each
    issued = steps * T * G
    valu = steps * 256 * VALU_PER_STEP                                                        # lane-instructions

    mssd, mspd = scorer.errors(est, gt, K32, obj)                   # warm-up of the whole path, and the values that are checked below
    n = min(a.slice, a.pairs)
    t0 = time.perf_counter()
    ref = []
    for p in range(n):
        f = lambda x: np.asarray(x, np.float32).astype(np.float64)  # noqa: E731
        r3, r2, s0, zmin = B.per_symmetry_errors(f(mesh[obj[p], :counts[obj[p]]]), f(est[p]), f(gt[p]), f(K32), f(syms[obj[p]]))
        ref.append((r3.min(), r2.min(), s0, zmin))
    numpy_s = time.perf_counter() - t0
    slice_evals = int((counts[obj[:n]].astype(np.int64) * sc[obj[:n]]).sum())
    worst3 = worst2 = 0.0
    for p, (r3, r2, s0, zmin) in enumerate(ref):
        assert zmin >= s0 / 2, p
        d3, d2 = abs(float(mssd[p]) - r3), abs(float(mspd[p]) - r2)
        worst3, worst2 = max(worst3, d3 / (4e-6 * s0)), max(worst2, d2 / (2e-6 * (float(K32[1, 1]) + 640.0)))
        assert d3 <= 4e-6 * s0 and d2 <= 2e-6 * (float(K32[1, 1]) + 640.0), (p, d3, d2)

    rec, idx = pack_bop_pairs(est, gt, K32, obj, scorer.objects)
    scorer._pairs[:a.pairs].copy_(torch.from_numpy(rec))
    scorer._index[:a.pairs].copy_(torch.from_numpy(idx))

    def window(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            scorer.launch(a.pairs)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    first = window(3)
    reps = max(3, int(np.ceil(600.0 / first)))                      # at least 0.6 s per window
    times = [window(reps) for _ in range(5)]
    ms = float(np.median(times))
    out = {"pairs": a.pairs, "vertex_counts": counts.tolist(), "symmetry_counts": sc.tolist(), "tile_vertices": T, "symmetry_group": G,
           "calls_per_window": reps, "windows": 5, "device_ms_per_call_median": ms, "device_ms_per_call_min": min(times),
           "device_ms_per_call_max": max(times), "evaluations_needed": useful, "evaluations_issued_with_padding": issued,
           "evaluations_needed_per_second": useful / (ms * 1e-3), "valu_instructions_per_step_per_thread": VALU_PER_STEP,
           "valu_issue_share": valu / (ms * 1e-3) / VALU_LANES_PER_SECOND, "numpy_fp64_slice_pairs": n, "numpy_fp64_slice_seconds": numpy_s,
           "numpy_fp64_whole_load_seconds_scaled": numpy_s * useful / slice_evals, "slice_worst_share_of_gate_3d": worst3,
           "slice_worst_share_of_gate_2d": worst2}
    print("load: %d pairs, vertices %s, symmetries %s" % (a.pairs, counts.tolist(), sc.tolist()))
    print("device time per call (both kernels, events, median of 5 windows of %d calls): %.3f ms (%.3f - %.3f)" % (reps, ms, min(times), max(times)))
    print("point-symmetry evaluations: %.4g needed (%.4g issued with padding) -> %.4g needed evaluations/s" % (useful, issued, out["evaluations_needed_per_second"]))
    print("share of the fp32 VALU issue rate (%d VALU instructions per thread and step): %.1f %%" % (VALU_PER_STEP, 100 * out["valu_issue_share"]))
    print("NumPy fp64 reference: %.2f s for %d pairs, scaled by evaluations to the whole load: %.0f s" % (numpy_s, n, out["numpy_fp64_whole_load_seconds_scaled"]))
    print("slice against the reference: worst %.1f %% of the 3-D gate, %.1f %% of the 2-D gate" % (100 * worst3, 100 * worst2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
