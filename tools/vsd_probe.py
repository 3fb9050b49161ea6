#!/usr/bin/env python3
"""Times of the VSD kernel (cp_vsd_counts_i32, csrc/vsd.hip) and of DeviceVsdScorer.counts on a seeded synthetic load of the size a user would
run: 8 objects, 250 images of 480 x 640 with one estimate and one ground truth per object, 2 000 pairs.

    python tools/vsd_probe.py [--out profiles/vsd_probe.json] [--images 250] [--slice 24]

A GPU tool; it reads nothing outside the tree.  Reported, each named for what it is:
  kernel time per call     the memset of the counts and vsd_counts_kernel over all pairs, from device events around repeated launches after a
                           warm-up, windows of at least half a second, for every number of blocks per pair in SPLITS; the windows of the
                           choices alternate, the median of 5 per choice with min - max
  counts() end to end      packing, the renders of all 4 000 poses, uploads, the kernel and the download: device events around whole calls
  bytes the kernel needs   per pair the pixels of the union box times 12 (two planes and the sensor depth, 4 bytes each), from the records
  share of the read rate   those bytes over the kernel time, against the rate at which this GPU reads HBM in the same process: torch.sum over
                           2 GiB of fp32, bytes over device time.  The kernel's own share of peak, not a whole-program figure
  NumPy baseline           the wall time of tests/vsd_reference.py (fp64, whole images) on the first `slice` pairs, scaled by pairs: the parent
                           of this kernel is no kernel
It also asserts that the device counts of the slice pass the gate of tests/test_gpu_vsd.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raster_reference as RR  # noqa: E402
import vsd_reference as VR  # noqa: E402
from casapose_amd.pose_estimation.bop_vsd import DEFAULT_FAR, DEFAULT_NEAR, VSD_DELTA, VSD_TAUS, DeviceVsdScorer  # noqa: E402

SPLITS = (1, 2, 4, 8, 16, 32, 64)
H, W = 480, 640
CAM = (572.4114, 573.57043, 325.2611, 242.04899)
K = np.array([[CAM[0], 0.0, CAM[2]], [0.0, CAM[1], CAM[3]], [0.0, 0.0, 1.0]])
AXES = [(70, 50, 60), (55, 75, 45), (60, 60, 80), (40, 30, 35), (30, 45, 25), (80, 40, 40), (35, 35, 35), (50, 65, 30)]


def build_load(images, seed=4711):
    rng = np.random.default_rng(seed)
    sphere, faces = RR.icosphere(3)
    meshes = [((sphere * np.asarray(a, np.float64)).astype(np.float32), faces) for a in AXES]
    est, gt, obj, img = [], [], [], []
    for m in range(images):
        for o in range(len(AXES)):
            z = rng.uniform(600.0, 1200.0)
            P = RR.pose_at(CAM, rng.uniform(60, W - 60), rng.uniform(60, H - 60), z, RR.rotation(rng.normal(0, 1, 3), rng.uniform(0, 3)))
            E = np.hstack([RR.rotation(rng.normal(0, 1, 3), rng.normal(0, 0.05)) @ P[:, :3], P[:, 3:] + rng.normal(0, 1, (3, 1)) * [[5.0], [5.0], [15.0]]])
            est.append(E), gt.append(P), obj.append(o), img.append(m)
    return meshes, np.stack(est), np.stack(gt), np.array(obj), np.array(img), np.array([2.0 * max(AXES[o]) for o in obj])


def union_box_pixels(records, pairs):
    """the pixels each pair's block walks: csrc/vsd_math.h pair_setup on the downloaded records"""
    def clip(r):
        x, y, w, h = (r[:, k].astype(np.int64) for k in (2, 3, 4, 5))
        x0, y0, x1, y1 = np.maximum(x, 0), np.maximum(y, 0), np.minimum(x + w, W - 1), np.minimum(y + h, H - 1)
        return x0, y0, x1, y1, (w >= 0) & (h >= 0) & (x0 <= x1) & (y0 <= y1)

    a, b = clip(records[pairs[:, 1]]), clip(records[pairs[:, 2]])
    big = np.int64(1) << 40
    lo = [np.minimum(np.where(a[4], a[k], big), np.where(b[4], b[k], big)) for k in (0, 1)]
    hi = [np.maximum(np.where(a[4], a[k], -big), np.where(b[4], b[k], -big)) for k in (2, 3)]
    return np.where(a[4] | b[4], (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1), 0)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=250)
    ap.add_argument("--slice", type=int, default=24)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vsd_probe.py needs a ROCm GPU: a CPU run gives no device time")
    dev = torch.device("cuda:0")
    meshes, est, gt, obj, img, diam = build_load(a.images)
    npairs = len(obj)
    scorer = DeviceVsdScorer([m[0] for m in meshes], [m[1] for m in meshes], dev, workspace_cap=1 << 34)      # all planes of the load at once

    # the sensor depth: the nearest ground truth over a background at 1500 mm, in whole millimetres, with 3 % of the pixels missing
    rng = np.random.default_rng(5)
    frames = [dict(cam=CAM, instances=[(int(obj[p]), 1, gt[p]) for p in np.flatnonzero(img == m)]) for m in range(a.images)]
    with torch.cuda.device(dev):
        taus = np.asarray(VSD_TAUS, np.float64)
        job = scorer.prepare([dict(cam=CAM, depth=np.zeros((H, W), np.float32), slots=[(o, P) for o, _, P in fr["instances"]], pairs=[]) for fr in frames],
                             H, W, len(AXES), VSD_DELTA, taus)
        planes = job["planes"].view(torch.float32).view(a.images, len(AXES), H, W)
        nearest = torch.where(job["planes"].view(torch.int32).view(a.images, len(AXES), H, W) == -1, torch.full_like(planes, 1500.0), planes).amin(dim=1)
        depths = torch.round(nearest).cpu().numpy().astype(np.float32)
        del job, planes, nearest
    depths[rng.random(depths.shape) < 0.03] = 0.0
    depths = list(depths)

    # ---- end to end: the warm-up call gives the values that are checked below -----------------------------------------------------------
    with torch.cuda.device(dev):
        counts = scorer.counts(est, gt, K, obj, img, depths, diam)
        chunks, renders, dropped = scorer.last_chunks, scorer.last_renders, scorer.last_dropped
        t0 = time.perf_counter()
        e2e = [events(lambda: scorer.counts(est, gt, K, obj, img, depths, diam), 1) for _ in range(5)]
        e2e_wall = (time.perf_counter() - t0) / 5.0

        # ---- the slice against the reference ---------------------------------------------------------------------------------------------
        n = min(a.slice, npairs)
        ref = VR.Scene(meshes, DEFAULT_NEAR, DEFAULT_FAR)
        planes_of = [(ref.plane(int(obj[p]), est[p], CAM, H, W), ref.plane(int(obj[p]), gt[p], CAM, H, W)) for p in range(n)]
        t0 = time.perf_counter()
        both = [VR.pair_counts(planes_of[p][0], planes_of[p][1], depths[img[p]], CAM, diam[p]) for p in range(n)]
        numpy_s = time.perf_counter() - t0
        loose = VR.check_counts(counts[:n], np.stack([c for c, _ in both]), np.array([u for _, u in both]), "slice")

        # ---- the kernel alone, over one prepared job that holds every pair --------------------------------------------------------------------
        per_image = {}
        for p in range(npairs):
            im = per_image.setdefault(int(img[p]), dict(cam=CAM, depth=depths[img[p]], slots=[], pairs=[]))
            im["slots"] += [(int(obj[p]), est[p]), (int(obj[p]), gt[p])]
            im["pairs"].append((p, len(im["slots"]) - 2, len(im["slots"]) - 1, diam[p]))
        job = scorer.prepare([per_image[m] for m in sorted(per_image)], H, W, 2 * len(AXES), VSD_DELTA, taus)
        scorer.launch(job, 1)
        assert np.array_equal(job["counts"].cpu().numpy(), counts[job["where"]])
        pixels = union_box_pixels(job["records"].view(-1, 11).cpu().numpy(), job["pairs"].cpu().numpy())
        need = int(pixels.sum()) * 12
        first = {s: events(lambda: scorer.launch(job, s), 20) for s in SPLITS}
        reps = {s: max(20, int(np.ceil(600.0 / first[s]))) for s in SPLITS}                 # at least 0.6 s per window
        times = {s: [] for s in SPLITS}
        for _ in range(5):                                                                   # the choices alternate
            for s in SPLITS:
                times[s].append(events(lambda: scorer.launch(job, s), reps[s]))
                scorer.launch(job, s)
                assert np.array_equal(job["counts"].cpu().numpy(), counts[job["where"]]), s

        # ---- the rate at which this GPU reads HBM ----------------------------------------------------------------------------------------------
        big = torch.ones(1 << 29, dtype=torch.float32, device=dev)                           # 2 GiB: beyond every cache
        events(big.sum, 3)
        read = [events(big.sum, 20) for _ in range(5)]
        read_rate = big.numel() * 4 / (float(np.median(read)) * 1e-3)

    med = {s: float(np.median(times[s])) for s in SPLITS}
    best = min(SPLITS, key=lambda s: med[s])
    out = {"pairs": npairs, "images": a.images, "height": H, "width": W, "objects": len(AXES), "triangles_per_object": int(len(meshes[0][1])),
           "tile_pixels": int(scorer._lib.cp_vsd_tile()), "ntau": len(VSD_TAUS), "union_box_pixels": int(pixels.sum()),
           "union_box_pixels_per_pair_median": float(np.median(pixels)), "bytes_needed": need,
           "kernel_ms_per_call": {str(s): {"median": med[s], "min": min(times[s]), "max": max(times[s]), "calls_per_window": reps[s]} for s in SPLITS},
           "windows": 5, "best_split": best, "bytes_needed_per_second_at_best": need / (med[best] * 1e-3),
           "hbm_read_bytes_per_second_measured": read_rate, "hbm_read_share_at_best": need / (med[best] * 1e-3) / read_rate,
           "hbm_read_share_at_split_1": need / (med[1] * 1e-3) / read_rate,
           "counts_end_to_end_ms": {"median": float(np.median(e2e)), "min": min(e2e), "max": max(e2e), "wall_ms_mean": 1e3 * e2e_wall, "calls": 5,
                                    "launches_per_call": chunks, "renders_per_call": renders, "dropped_triangles": dropped},
           "numpy_fp64_slice_pairs": n, "numpy_fp64_slice_seconds": numpy_s, "numpy_fp64_whole_load_seconds_scaled": numpy_s * npairs / n,
           "slice_pairs_with_undecided_pixels": loose}
    lines = ["load: %d pairs in %d images of %d x %d, %d objects of %d triangles, ntau %d; union boxes %.4g pixels (median %d per pair)"
             % (npairs, a.images, H, W, len(AXES), len(meshes[0][1]), len(VSD_TAUS), pixels.sum(), np.median(pixels))]
    for s in SPLITS:
        lines.append("kernel alone, %d block(s) per pair (events, median of 5 alternating windows of %d calls): %.4f ms (%.4f - %.4f)"
                     % (s, reps[s], med[s], min(times[s]), max(times[s])))
    lines.append("bytes the kernel needs: %.4g -> %.4g B/s at %d block(s) per pair; this GPU reads HBM at %.4g B/s (torch.sum over 2 GiB): %.1f %% of it "
                 "(%.1f %% at 1 block per pair)" % (need, out["bytes_needed_per_second_at_best"], best, read_rate, 100 * out["hbm_read_share_at_best"],
                                                    100 * out["hbm_read_share_at_split_1"]))
    lines.append("counts() end to end (%d renders, %d launch(es); events, median of 5 calls): %.1f ms (%.1f - %.1f), wall %.1f ms"
                 % (renders, chunks, np.median(e2e), min(e2e), max(e2e), 1e3 * e2e_wall))
    lines.append("NumPy fp64 reference: %.2f s for %d pairs, scaled by pairs to the whole load: %.0f s; the slice passes the gate (%d pairs with undecided pixels)"
                 % (numpy_s, n, out["numpy_fp64_whole_load_seconds_scaled"], loose))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
