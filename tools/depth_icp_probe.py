#!/usr/bin/env python3
"""Times of the depth refinement's step (cp_depth_icp_step_f64, csrc/depth_icp.hip), of the render of the same planes and of
DeviceDepthRefiner.refine on the seeded synthetic load of tools/vsd_probe.py: 8 objects, 250 images of 480 x 640, 2 000 estimates.

    python tools/depth_icp_probe.py [--out profiles/depth_icp_probe.json] [--images 250]

A GPU tool; it reads nothing outside the tree.  Reported, each named for what it is:
  step per call        the step's two launches (accumulate, solve; update = 0, so every call does the same work) over all jobs, from device
                       events around repeated calls after a warm-up, windows of at least 0.4 s, for every number of blocks per job in SPLITS
  render per call      cp_render_masks_u8 of the same 2 000 planes, the yardstick, timed the same way; the windows of all choices alternate, the
                       median of 5 per choice with min - max
  refine() end to end  packing, uploads, 9 x (render, step) and the copy back at 8 iterations: device events around whole calls
  box pixels           the pixels the jobs walk (their clipped boxes) and the pixels they use, from the records and the stats
It asserts that every split gives the bytes of split 1 and that the estimates refine() keeps are closer to the ground truth than they were."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vsd_probe import AXES, CAM, H, K, W, build_load, events  # noqa: E402
from casapose_amd.pose_estimation.depth_refine import DeviceDepthRefiner  # noqa: E402

SPLITS = (1, 2, 3, 4, 6, 8, 12, 16)
GATE, JUMP, DAMPING, MIN_PIXELS = 0.25, 0.75, 1e-6, 32


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=250)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("depth_icp_probe.py needs a ROCm GPU: a CPU run gives no device time")
    dev = torch.device("cuda:0")
    meshes, est, gt, obj, img, diam = build_load(a.images)
    n, imax = len(obj), len(AXES)
    refiner = DeviceDepthRefiner([m[0] for m in meshes], [m[1] for m in meshes], dev, workspace_cap=1 << 34)      # the whole load in one chunk
    cams = np.tile(np.asarray(CAM, np.float64), (a.images, 1))
    jobs = np.array([(int(img[p]), p, 0, 0) for p in range(n)], np.int32)                                        # build_load: slot p = image * 8 + object
    assert all(int(img[p]) * imax + int(obj[p]) == p for p in range(n))
    frames_of = lambda poses: [dict(cam=CAM, instances=[(int(obj[p]), 1, poses[p]) for p in range(m * imax, (m + 1) * imax)]) for m in range(a.images)]   # noqa: E731

    with torch.cuda.device(dev):
        # the sensor depth: the nearest ground truth over a background at 1500 mm, in whole millimetres, with 3 % of the pixels missing
        c = refiner.prepare(frames_of(gt), [np.zeros((H, W), np.float32)] * a.images, cams, jobs, GATE * diam, imax, H, W, 1)
        refiner.render(c)
        planes = c["planes"].view(torch.float32).view(a.images, imax, H, W)
        nearest = torch.where(c["planes"].view(torch.int32).view(a.images, imax, H, W) == -1, torch.full_like(planes, 1500.0), planes).amin(dim=1)
        depths = torch.round(nearest).cpu().numpy().astype(np.float32)
        del c, planes, nearest
        depths[np.random.default_rng(5).random(depths.shape) < 0.03] = 0.0
        depths = list(depths)

        # ---- the step and the render alone, over one chunk that holds every estimate -------------------------------------------------------
        c = refiner.prepare(frames_of(est), depths, cams, jobs, GATE * diam, imax, H, W, 1)
        render = lambda: refiner.render(c)                                                                       # noqa: E731
        step = lambda s: refiner.step(c, 0, 0, JUMP, DAMPING, MIN_PIXELS, s)                                     # noqa: E731
        render()
        step(1)
        _, stats1, status1 = (x.copy() for x in refiner.finish(c))
        records = c["records"].view(-1, 11).cpu().numpy()
        x, y, w, h = (records[:, k].astype(np.int64) for k in (2, 3, 4, 5))
        box = np.where((w >= 0) & (h >= 0), np.maximum(np.minimum(x + w, W - 2) - np.maximum(x, 1) + 1, 0) * np.maximum(np.minimum(y + h, H - 2) - np.maximum(y, 1) + 1, 0), 0)
        choices = ["render"] + list(SPLITS)
        run = {k: (render if k == "render" else (lambda s=k: step(s))) for k in choices}
        first = {k: events(run[k], 5) for k in choices}
        reps = {k: max(5, int(np.ceil(400.0 / first[k]))) for k in choices}
        times = {k: [] for k in choices}
        for _ in range(5):                                                                                       # the choices alternate
            for k in choices:
                times[k].append(events(run[k], reps[k]))
        for s in SPLITS:
            step(s)
            _, stats, status = refiner.finish(c)
            assert stats.tobytes() == stats1.tobytes() and status.tobytes() == status1.tobytes(), s
        del c

        # ---- end to end ------------------------------------------------------------------------------------------------------------------------
        call = lambda: refiner.refine(est, K, obj, img, depths, diam)                                             # noqa: E731
        refined, info = call()
        chunks, renders = refiner.last_chunks, refiner.last_renders
        t0 = time.perf_counter()
        e2e = [events(call, 1) for _ in range(3)]
        e2e_wall = (time.perf_counter() - t0) / 3.0

    t_err = lambda P: np.linalg.norm(P[:, :, 3] - gt[:, :, 3], axis=1)   # noqa: E731
    ok = info["status"] == 0
    med = {k: float(np.median(times[k])) for k in choices}
    best = min(SPLITS, key=lambda s: med[s])
    out = {"jobs": n, "images": a.images, "height": H, "width": W, "objects": imax, "triangles_per_object": int(len(meshes[0][1])),
           "tile_pixels": int(refiner._lib.cp_depth_icp_tile()), "box_pixels": int(box.sum()), "box_pixels_per_job_median": float(np.median(box)),
           "box_pixels_per_job_max": int(box.max()), "pixels_used": int(stats1[0, :, 0].sum()), "jobs_solved_first_pass": int((status1[0] == 0).sum()),
           "ms_per_call": {str(k): {"median": med[k], "min": min(times[k]), "max": max(times[k]), "calls_per_window": reps[k]} for k in choices},
           "windows": 5, "best_split": best, "step_over_render_at_best": med[best] / med["render"], "step_over_render_at_split_1": med[1] / med["render"],
           "refine_end_to_end_ms": {"median": float(np.median(e2e)), "min": min(e2e), "max": max(e2e), "wall_ms_mean": 1e3 * e2e_wall, "calls": 3,
                                    "iterations": 8, "chunks": chunks, "renders": renders},
           "refined": int(ok.sum()), "status_counts": np.bincount(info["status"], minlength=6).tolist(),
           "translation_error_mm_median": {"before": float(np.median(t_err(est)[ok])), "after": float(np.median(t_err(refined)[ok]))}}
    lines = ["load: %d jobs in %d images of %d x %d, %d objects of %d triangles; clipped boxes %.4g pixels (median %d, largest %d per job), %.4g pixels used, "
             "%d jobs solve the first pass" % (n, a.images, H, W, imax, len(meshes[0][1]), box.sum(), np.median(box), box.max(), stats1[0, :, 0].sum(),
                                               (status1[0] == 0).sum()),
             "render of the %d planes (events, median of 5 alternating windows of %d calls): %.4f ms (%.4f - %.4f) = %.2f us per plane"
             % (n, reps["render"], med["render"], min(times["render"]), max(times["render"]), 1e3 * med["render"] / n)]
    for s in SPLITS:
        lines.append("step, %2d block(s) per job (accumulate + solve; %d calls per window): %.4f ms (%.4f - %.4f) = %.2f us per job = %.2f x the render"
                     % (s, reps[s], med[s], min(times[s]), max(times[s]), 1e3 * med[s] / n, med[s] / med["render"]))
    lines.append("refine() end to end at 8 iterations (%d renders, %d chunk(s); events, median of 3 calls): %.1f ms (%.1f - %.1f), wall %.1f ms; %d of %d "
                 "refined, median translation error %.2f -> %.3f mm" % (renders, chunks, np.median(e2e), min(e2e), max(e2e), 1e3 * e2e_wall, ok.sum(), n,
                                                                        out["translation_error_mm_median"]["before"], out["translation_error_mm_median"]["after"]))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    assert ok.sum() >= n // 2 and np.median(t_err(refined)[ok]) < 0.2 * np.median(t_err(est)[ok]), "refine() did not bring the estimates it kept closer"


if __name__ == "__main__":
    main()
