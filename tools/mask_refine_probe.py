#!/usr/bin/env python3
"""Times of the mask refinement's kernels (cp_mask_edt_u16, cp_contour_step_f64, csrc/mask_contour.hip) and of DeviceMaskRefiner.refine on the
seeded synthetic load of tools/vsd_probe.py: 8 objects, 250 images of 480 x 640, 2 000 estimates; the label maps are rendered from the ground
truth (sample offset 0.5), so they say nothing about real segmentation errors.

    python tools/mask_refine_probe.py [--out profiles/mask_refine_probe.json] [--images 250]

A GPU tool; it reads nothing outside the tree.  Reported, each named for what it is:
  field per call       cp_mask_edt_u16 (rows, columns) for 16 images x 8 labels = 128 fields, at the default gate and at GATES, from device events
                       around repeated calls after a warm-up, windows of at least 0.4 s
  its yardsticks       cp_ccl_filter_labels on the same 16 label maps, and the render of the same 128 planes, timed the same way
  step per call        the step's two launches (accumulate, solve; update = 0, so every call does the same work) over all 2 000 jobs, for every
                       number of blocks per job in SPLITS; render per call: cp_render_masks_u8 of the same 2 000 planes, the yardstick
  refine() end to end  packing, uploads, the fields, 9 x (render, step) and the copy back at 8 iterations: device events around whole calls
The windows of all choices of a group alternate; the median of 5 per choice with min - max.  It asserts that every split gives the bytes of
split 1, that the device fields are the host twin's on one image, and that the estimates refine() keeps are closer in the image plane."""
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
from casapose_amd import _lib, twin  # noqa: E402
from casapose_amd.pose_estimation.mask_refine import DEFAULT_GATE, DEFAULT_MIN_PIXELS, DeviceMaskRefiner  # noqa: E402

SPLITS = (1, 2, 4, 8, 16)
GATES = (8, 24)            # beside the default: gates of the size a 480 x 640 frame's errors ask for
FIELD_IMAGES = 16
DAMPING = 1e-6


def windows(run, choices):
    first = {k: events(run[k], 5) for k in choices}
    reps = {k: max(5, int(np.ceil(400.0 / first[k]))) for k in choices}
    times = {k: [] for k in choices}
    for _ in range(5):
        for k in choices:
            times[k].append(events(run[k], reps[k]))
    return {str(k): {"median": float(np.median(times[k])), "min": min(times[k]), "max": max(times[k]), "calls_per_window": reps[k]} for k in choices}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=250)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mask_refine_probe.py needs a ROCm GPU: a CPU run gives no device time")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    meshes, est, gt, obj, img, _ = build_load(a.images)
    n, imax = len(obj), len(AXES)
    refiner = DeviceMaskRefiner([m[0] for m in meshes], [m[1] for m in meshes], dev, workspace_cap=1 << 35)      # the whole load in one chunk
    cams = np.tile(np.asarray(CAM, np.float64), (a.images, 1))
    assert all(int(img[p]) * imax + int(obj[p]) == p for p in range(n))                                          # build_load: slot p = image * 8 + object
    frames_of = lambda poses, lo, hi: [dict(cam=CAM, instances=[(int(obj[p]), int(obj[p]) + 1, poses[p]) for p in range(m * imax, (m + 1) * imax)])   # noqa: E731
                                       for m in range(lo, hi)]
    fields_all = np.array([(m, o + 1) for m in range(a.images) for o in range(imax)], np.int32)
    jobs_all = np.array([(int(img[p]), p, p, DEFAULT_GATE) for p in range(n)], np.int32)

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        # the label maps: the ground truth rendered with label = object + 1
        c = refiner.buffers(frames_of(gt, 0, a.images), n, imax, H, W, 1)
        labels, _ = refiner.renderer._render(c["mesh"], c["packed"], c["frames"], H, W, refiner.near, refiner.far, refiner.sample_offset, c["planes"],
                                             c["planes_bytes"], dev, stream)
        labels = labels.clone()
        del c

        # ---- the field, 16 images x 8 labels ---------------------------------------------------------------------------------------------------
        fi = min(FIELD_IMAGES, a.images)
        nf = fi * imax
        lab16 = labels[:fi].contiguous()
        c16 = refiner.prepare(frames_of(est, 0, fi), lab16, fi, cams[:fi], jobs_all[:nf], fields_all[:nf], imax, H, W, 1)
        ccl_ws = torch.empty(lib.cp_ccl_workspace_bytes(fi, H, W, imax), dtype=torch.uint8, device=dev)
        ccl_out = torch.empty_like(lab16)
        ccl = lambda: _lib.check(lib.cp_ccl_filter_labels(lab16.data_ptr(), fi, H, W, imax, 50, 1, ccl_ws.data_ptr(), ccl_out.data_ptr(), stream),   # noqa: E731
                                 "cp_ccl_filter_labels")
        run = {"ccl_filter": ccl, "render": lambda: refiner.render(c16)}
        for g in (DEFAULT_GATE,) + GATES:
            run["field_gate_%d" % g] = lambda g=g: refiner.distance(c16, g)
        field_ms = windows(run, list(run))
        refiner.distance(c16, DEFAULT_GATE)
        got = c16["fields"][:imax].cpu().numpy()
        want = twin.alloc(dict(p=((imax, H, W), np.uint16), s=((imax,), np.int32), r=((imax, H, W), np.uint16)))
        twin.call("cp_mask_edt_u16", lab16[:1].cpu().numpy(), 1, H, W, fields_all[:imax], imax, DEFAULT_GATE, want["p"], want["s"], want["r"], imax * H * W * 2,
                  host=True)
        assert got.tobytes() == want["p"].tobytes(), "the device fields of image 0 are not the host twin's"
        seeds = int((c16["fields"] == 0).sum())
        del c16

        # ---- the step and the render alone, over one chunk that holds every estimate -------------------------------------------------------
        c = refiner.prepare(frames_of(est, 0, a.images), labels, a.images, cams, jobs_all, fields_all, imax, H, W, 1)
        refiner.distance(c, DEFAULT_GATE)
        render = lambda: refiner.render(c)                                                                       # noqa: E731
        step = lambda s: refiner.step(c, 0, 0, DAMPING, DEFAULT_MIN_PIXELS, s)                                   # noqa: E731
        render()
        step(1)
        _, stats1, status1 = (x.copy() for x in refiner.finish(c))
        run = {"render": render}
        run.update({s: (lambda s=s: step(s)) for s in SPLITS})
        step_ms = windows(run, list(run))
        for s in SPLITS:
            step(s)
            _, stats, status = refiner.finish(c)
            assert stats.tobytes() == stats1.tobytes() and status.tobytes() == status1.tobytes(), s
        del c

        # ---- end to end ------------------------------------------------------------------------------------------------------------------------
        e2e = {}
        for g, mp in ((DEFAULT_GATE, DEFAULT_MIN_PIXELS), (GATES[0], 60)):
            call = lambda: refiner.refine(est, K, obj, img, labels, obj + 1, gate=g, min_pixels=mp)               # noqa: E731
            refined, info = call()
            t0 = time.perf_counter()
            t = [events(call, 1) for _ in range(3)]
            wall = (time.perf_counter() - t0) / 3.0
            ok = info["status"] == 0
            xy = lambda P: np.linalg.norm(P[:, :2, 3] - gt[:, :2, 3], axis=1)                                     # noqa: E731
            e2e[g] = dict(gate=g, min_pixels=mp, median=float(np.median(t)), min=min(t), max=max(t), wall_ms_mean=1e3 * wall, calls=3, iterations=8,
                          chunks=refiner.last_chunks, renders=refiner.last_renders, fields=refiner.last_fields, refined=int(ok.sum()),
                          status_counts=np.bincount(info["status"], minlength=6).tolist(),
                          image_plane_error_mm_median={"before": float(np.median(xy(est)[ok])), "after": float(np.median(xy(refined)[ok]))},
                          axis_error_mm_median={"before": float(np.median(np.abs(est[ok, 2, 3] - gt[ok, 2, 3]))),
                                                "after": float(np.median(np.abs(refined[ok, 2, 3] - gt[ok, 2, 3])))})

    best = min(SPLITS, key=lambda s: step_ms[str(s)]["median"])
    per_image_field = field_ms["field_gate_%d" % DEFAULT_GATE]["median"] / fi
    per_image_render = field_ms["render"]["median"] / fi
    out = {"jobs": n, "images": a.images, "height": H, "width": W, "objects": imax, "triangles_per_object": int(len(meshes[0][1])),
           "tile_pixels": int(lib.cp_contour_tile()), "default_gate": DEFAULT_GATE, "default_min_pixels": DEFAULT_MIN_PIXELS,
           "field_images": fi, "fields": nf, "field_seeds": seeds, "field_group_ms_per_call": field_ms, "step_group_ms_per_call": step_ms, "windows": 5,
           "contour_pixels": int(stats1[0, :, 2].sum()), "pixels_used": int(stats1[0, :, 0].sum()), "jobs_solved_first_pass": int((status1[0] == 0).sum()),
           "best_split": best, "step_over_render_at_best": step_ms[str(best)]["median"] / step_ms["render"]["median"],
           "step_over_render_at_split_4": step_ms["4"]["median"] / step_ms["render"]["median"],
           "field_per_image_over_8_renders_of_its_planes": per_image_field / (8.0 * per_image_render),
           "field_over_ccl_filter": field_ms["field_gate_%d" % DEFAULT_GATE]["median"] / field_ms["ccl_filter"]["median"],
           "refine_end_to_end": {str(g): v for g, v in e2e.items()}}
    fmt = lambda d: "%.4f ms (%.4f - %.4f)" % (d["median"], d["min"], d["max"])   # noqa: E731
    lines = ["load: %d jobs in %d images of %d x %d, %d objects of %d triangles; %d contour pixels, %d used at gate %d, %d jobs solve the first pass"
             % (n, a.images, H, W, imax, len(meshes[0][1]), stats1[0, :, 2].sum(), stats1[0, :, 0].sum(), DEFAULT_GATE, (status1[0] == 0).sum()),
             "fields of %d images x %d labels (%d seeds; events, median of 5 alternating windows):" % (fi, imax, seeds)]
    for k, d in field_ms.items():
        lines.append("  %-16s %s = %.4f ms per image" % (k, fmt(d), d["median"] / fi))
    lines.append("  the fields of an image at the default gate cost %.2f x 8 renders of its planes and %.2f x cp_ccl_filter_labels of its label map"
                 % (out["field_per_image_over_8_renders_of_its_planes"], out["field_over_ccl_filter"]))
    lines.append("render of the %d planes: %s = %.2f us per plane" % (n, fmt(step_ms["render"]), 1e3 * step_ms["render"]["median"] / n))
    for s in SPLITS:
        d = step_ms[str(s)]
        lines.append("step, %2d block(s) per job (accumulate + solve): %s = %.2f us per job = %.2f x the render"
                     % (s, fmt(d), 1e3 * d["median"] / n, d["median"] / step_ms["render"]["median"]))
    for g, v in e2e.items():
        lines.append("refine() end to end at 8 iterations, gate %d, min_pixels %d (%d renders, %d fields, %d chunk(s); events, median of 3 calls): %.1f ms "
                     "(%.1f - %.1f), wall %.1f ms; %d of %d refined, median error of those %.2f -> %.2f mm in the image plane, %.2f -> %.2f mm along the axis"
                     % (g, v["min_pixels"], v["renders"], v["fields"], v["chunks"], v["median"], v["min"], v["max"], v["wall_ms_mean"], v["refined"], n,
                        v["image_plane_error_mm_median"]["before"], v["image_plane_error_mm_median"]["after"], v["axis_error_mm_median"]["before"],
                        v["axis_error_mm_median"]["after"]))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
    v = e2e[GATES[0]]
    assert v["image_plane_error_mm_median"]["after"] < v["image_plane_error_mm_median"]["before"], "refine() did not bring the estimates it kept closer"


if __name__ == "__main__":
    main()
