#!/usr/bin/env python3
"""Times of the pose verification's kernel (cp_pose_verify_i32, csrc/pose_verify.hip), of DevicePoseVerifier.verify and of the instance path with
and without verified scores, on the seeded synthetic load of tools/vsd_probe.py: 8 objects, 250 images of 480 x 640, 2 000 estimates, 8 per
image; the label maps are rendered from the ground truth (sample offset 0.5) and the field holds, in the production record ld 36 / dir_off 9 /
kp 9, the unit directions to the ground truth's keypoints turned by N(0, 0.05 rad), so they say nothing about a real network's errors.

    python tools/pose_verify_probe.py [--out profiles/pose_verify_probe.json] [--images 250]

A GPU tool; it reads nothing outside the tree.  Reported, each named for what it is:
  verify per call      the two memsets, the histogram pass and the counts kernel over all 2 000 jobs, from device events around repeated calls
                       after a warm-up, windows of at least 0.4 s, for every number of blocks per job in SPLITS
  its yardsticks       cp_render_masks_u8 of the same 2 000 planes, and cp_vsd_counts_i32 over the same planes (each plane against itself, no
                       sensor depth, so that it walks the very boxes), timed the same way in the same alternation
  verify() end to end  packing, uploads, the render, the verification and the copy back: device events around whole calls
  instance path        one 480 x 640 frame at batch 1 -- InstanceLSVoting (R = 4) on a record made of image 0's label map and field, the host PnP
                       per instance, and with the switch verify_instance_estimates -- wall time with a device synchronisation around each frame
The windows of all choices alternate; the median of 5 per choice with min - max.  It asserts that every split gives the bytes of split 1, that
the device counts of image 0 are the host twin's, and that the estimates' scores fall with their error."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mask_refine_probe import windows  # noqa: E402
from vsd_probe import AXES, CAM, H, K, W, build_load, events  # noqa: E402
from casapose_amd import _lib, twin  # noqa: E402
from casapose_amd.pose_estimation.bop_vsd import VSD_DELTA, VSD_TAUS  # noqa: E402
from casapose_amd.pose_estimation.pose_verify import (DEFAULT_COS_MIN, DevicePoseVerifier, project_keypoints, score_from_counts,  # noqa: E402
                                                      verify_instance_estimates)

SPLITS = (1, 2, 4, 8, 16)
KP, LD, DIR_OFF = 9, 36, 9
TURN_SIGMA = 0.05
R = 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=250)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_verify_probe.py needs a ROCm GPU: a CPU run gives no device time")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    meshes, est, gt, obj, img, diam = build_load(a.images)
    n, imax, M = len(obj), len(AXES), a.images
    verifier = DevicePoseVerifier([m[0] for m in meshes], [m[1] for m in meshes], dev, workspace_cap=1 << 35)      # the whole load in one chunk
    assert all(int(img[p]) * imax + int(obj[p]) == p for p in range(n))                                            # build_load: slot p = image * 8 + object
    signs = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    kps3 = np.stack([np.array([(0.0, 0.0, 0.0)] + [tuple(s * e for s, e in zip(sg, ax)) for sg in signs], np.float64) for ax in AXES])   # centre, box corners
    cams = np.tile(np.asarray(CAM, np.float64), (n, 1))
    frames_of = lambda poses: [dict(cam=CAM, instances=[(int(obj[p]), int(obj[p]) + 1, poses[p]) for p in range(m * imax, (m + 1) * imax)])   # noqa: E731
                               for m in range(M)]
    jobs = np.array([(int(img[p]), p, int(obj[p]) + 1, 0) for p in range(n)], np.int32)

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        # the label maps: the ground truth rendered with label = object + 1
        c = verifier.buffers(frames_of(gt), n, imax, H, W, 0)
        labels, _ = verifier.renderer._render(c["mesh"], c["packed"], c["frames"], H, W, verifier.near, verifier.far, verifier.sample_offset, c["planes"],
                                              c["planes_bytes"], dev, stream)
        labels = labels.clone()
        del c
        # the field: on a labelled pixel the directions to its object's true keypoints, turned; N(0, 1) elsewhere and in the other words
        gen = torch.Generator(device=dev).manual_seed(12)
        field = torch.randn((M, H, W, LD), generator=gen, device=dev, dtype=torch.float32)
        true2d = torch.from_numpy(project_keypoints(gt.reshape(n, 12), cams, kps3[obj]).reshape(M, imax, KP, 2)).to(dev)
        on = labels > 0
        which = (labels.long() - 1).clamp(min=0).view(M, -1)
        yc = (torch.arange(H, device=dev, dtype=torch.float64) + 0.5).view(1, H, 1)
        xc = (torch.arange(W, device=dev, dtype=torch.float64) + 0.5).view(1, 1, W)
        for k in range(KP):
            ky, kx = (torch.gather(true2d[:, :, k, c], 1, which).view(M, H, W) for c in (0, 1))
            angle = torch.atan2(ky - yc, kx - xc) + TURN_SIGMA * torch.randn((M, H, W), generator=gen, device=dev, dtype=torch.float64)
            field[..., DIR_OFF + 2 * k] = torch.where(on, torch.sin(angle).float(), field[..., DIR_OFF + 2 * k])
            field[..., DIR_OFF + 2 * k + 1] = torch.where(on, torch.cos(angle).float(), field[..., DIR_OFF + 2 * k + 1])
        del ky, kx, angle, which

        # ---- the kernel, the render and the VSD kernel over one chunk that holds every estimate -----------------------------------------------
        c = verifier.buffers(frames_of(est), n, imax, H, W, 0)
        verifier.render(c)
        kp2d = project_keypoints(est.reshape(n, 12), cams, kps3[obj])
        d_kp2d, d_jobs = twin.array(kp2d, np.float64, dev), twin.array(jobs, np.int32, dev)
        size = int(lib.cp_pose_verify_workspace_bytes(M))
        out = twin.alloc(dict(counts=((n, 8), np.int32), work=((size // 4,), np.int32)), dev)

        def verify(split):
            twin.call("cp_pose_verify_i32", c["planes"], c["records"], n, H, W, c["packed"]["inst_counts"], M, imax, labels, field, M, LD, DIR_OFF, KP, d_kp2d,
                      d_jobs, n, verifier.sample_offset, float(DEFAULT_COS_MIN), split, out["counts"], out["work"], size, stream=stream)

        taus = twin.array(np.asarray(VSD_TAUS, np.float64), np.float64, dev)
        vsd = dict(pairs=twin.array(np.array([(int(img[p]), p, p, 0) for p in range(n)], np.int32), np.int32, dev), diam=twin.array(diam, np.float64, dev),
                   cams=twin.array(cams[:M], np.float64, dev), depth=torch.zeros((M, H, W), dtype=torch.float32, device=dev),
                   counts=torch.empty((n, 2 + len(VSD_TAUS)), dtype=torch.int32, device=dev))

        def vsd_counts(split):
            _lib.check(lib.cp_vsd_counts_i32(c["planes"].data_ptr(), c["records"].data_ptr(), n, H, W, vsd["depth"].data_ptr(), vsd["cams"].data_ptr(), M,
                                             vsd["pairs"].data_ptr(), vsd["diam"].data_ptr(), n, float(VSD_DELTA), taus.data_ptr(), len(VSD_TAUS), split,
                                             vsd["counts"].data_ptr(), stream), "cp_vsd_counts_i32")

        verify(1)
        counts1 = out["counts"].cpu().numpy()
        run = {"render": lambda: verifier.render(c), "vsd_1": lambda: vsd_counts(1), "vsd_4": lambda: vsd_counts(4)}
        run.update({s: (lambda s=s: verify(s)) for s in SPLITS})
        ms = windows(run, list(run))
        for s in SPLITS:
            verify(s)
            assert out["counts"].cpu().numpy().tobytes() == counts1.tobytes(), s
        # image 0 against the host twin
        host = dict(planes=c["planes"].view(n, H, W)[:imax].cpu().numpy(), records=c["records"].view(n, 11)[:imax].cpu().numpy())
        want = twin.alloc(dict(counts=((imax, 8), np.int32), work=((256,), np.int32)))
        twin.call("cp_pose_verify_i32", host["planes"], host["records"], imax, H, W, np.array([imax], np.int32), 1, imax, labels[:1].cpu().numpy(),
                  field[:1].cpu().numpy(), 1, LD, DIR_OFF, KP, np.ascontiguousarray(kp2d[:imax]), np.ascontiguousarray(jobs[:imax]), imax,
                  verifier.sample_offset, float(DEFAULT_COS_MIN), 1, want["counts"], want["work"], 1024, host=True)
        assert want["counts"].tobytes() == counts1[:imax].tobytes(), "the device counts of image 0 are not the host twin's"
        box = c["records"].view(n, 11).cpu().numpy()
        box_pixels = int(sum(max(0, min(x + w, W - 1) - max(x, 0) + 1) * max(0, min(y + h, H - 1) - max(y, 0) + 1) for x, y, w, h in box[:, 2:6] if w >= 0 and h >= 0))
        del c

        # ---- end to end ------------------------------------------------------------------------------------------------------------------------
        call = lambda: verifier.verify(est, K, obj, img, labels, obj + 1, field, kps3, DIR_OFF)                   # noqa: E731
        got = call()
        assert got["counts"].tobytes() == counts1.tobytes()
        t0 = time.perf_counter()
        t = [events(call, 1) for _ in range(3)]
        wall = (time.perf_counter() - t0) / 3.0
        true = verifier.verify(gt, K, obj, img, labels, obj + 1, field, kps3, DIR_OFF)
        err = np.linalg.norm(est[:, :2, 3] - gt[:, :2, 3], axis=1)
        near, far = err < np.median(err), err >= np.median(err)
        assert np.median(true["score"]) > np.median(got["score"][near]) > np.median(got["score"][far]), "the scores do not fall with the error"

        # ---- the instance path at batch 1: image 0's label map and field as the network's record ------------------------------------------------
        from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting, poses_pnp_instances

        rec = torch.zeros((1, H, W, LD), dtype=torch.float32, device=dev)
        rec[..., :DIR_OFF] = 10.0 * torch.nn.functional.one_hot(labels[:1].long(), DIR_OFF).float()
        rec[..., DIR_OFF:DIR_OFF + 2 * KP] = field[:1, ..., DIR_OFF:DIR_OFF + 2 * KP]
        seg, dirs, conf = torch.split(rec, [DIR_OFF, 2 * KP, LD - DIR_OFF - 2 * KP], dim=3)
        voter = InstanceLSVoting(name="coords_ls_voting", num_classes=1 + imax, num_points=KP, max_instances=R)
        rng = np.random.default_rng(0)
        one = DevicePoseVerifier([m[0] for m in meshes], [m[1] for m in meshes], dev)
        kcam = K[None].astype(np.float32)

        def frame(score):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            coords = voter([seg, dirs, conf])
            poses = poses_pnp_instances(coords, voter.last_counts.cpu().numpy(), kps3.astype(np.float32), kcam, min_num=20, rng=rng)
            scores = verify_instance_estimates(one, np.asarray(poses), voter.last_labels, rec, kps3, kcam, dir_off=DIR_OFF) if score else None
            torch.cuda.synchronize(dev)
            return 1e3 * (time.perf_counter() - t0), poses, scores

        frame(True), frame(False)
        frames_ms = {False: [], True: []}
        for _ in range(15):
            for score in (False, True):
                frames_ms[score].append(frame(score)[0])
        _, poses, scores = frame(True)
        found = int(np.asarray(poses).reshape(-1, 12).any(axis=1).sum())

    best = min(SPLITS, key=lambda s: ms[str(s)]["median"])
    sc = score_from_counts(counts1)
    inst = {("with" if k else "without"): {"median": float(np.median(v)), "min": min(v), "max": max(v), "frames": len(v)} for k, v in frames_ms.items()}
    res = {"jobs": n, "images": M, "height": H, "width": W, "objects": imax, "estimates_per_image": imax, "record": [LD, DIR_OFF, KP],
           "tile_pixels": int(lib.cp_pose_verify_tile()), "cos_min": float(DEFAULT_COS_MIN), "box_pixels": box_pixels,
           "counts_sum": {k: int(v) for k, v in zip(("rendered", "hidden", "on_label", "on_background", "on_other", "label_pixels", "pairs", "inliers"), counts1.sum(0))},
           "group_ms_per_call": ms, "windows": 5, "best_split": best, "verify_over_render_at_best": ms[str(best)]["median"] / ms["render"]["median"],
           "verify_over_vsd_split_1": ms["1"]["median"] / ms["vsd_1"]["median"],
           "verify_end_to_end_ms": {"median": float(np.median(t)), "min": min(t), "max": max(t), "wall_ms_mean": 1e3 * wall, "calls": 3, "chunks": verifier.last_chunks},
           "score_median": {"truth": float(np.median(true["score"])), "estimates_nearer_half": float(np.median(got["score"][near])),
                            "estimates_farther_half": float(np.median(got["score"][far])), "estimates_iou": float(np.median(sc["iou"])),
                            "estimates_agreement": float(np.median(sc["agreement"]))},
           "instance_frame_ms": inst, "instance_frame_found": found, "instance_frame_score_median": float(np.median(scores[scores > 0])) if found else 0.0}
    fmt = lambda d: "%.4f ms (%.4f - %.4f)" % (d["median"], d["min"], d["max"])   # noqa: E731
    lines = ["load: %d jobs in %d images of %d x %d, %d per image, record ld %d / dir_off %d / kp %d; %d box pixels, %d rendered, %d hidden, %d on their label, "
             "%d pairs (events, median of 5 alternating windows)" % (n, M, H, W, imax, LD, DIR_OFF, KP, box_pixels, counts1[:, 0].sum(), counts1[:, 1].sum(),
                                                                     counts1[:, 2].sum(), counts1[:, 6].sum()),
             "render of the %d planes: %s = %.2f us per plane" % (n, fmt(ms["render"]), 1e3 * ms["render"]["median"] / n)]
    for s in (1, 4):
        lines.append("cp_vsd_counts_i32 over the same planes, %d block(s) per pair: %s" % (s, fmt(ms["vsd_%d" % s])))
    for s in SPLITS:
        d = ms[str(s)]
        lines.append("verify, %2d block(s) per job (memsets, histogram, counts): %s = %.2f us per job = %.2f x the render"
                     % (s, fmt(d), 1e3 * d["median"] / n, d["median"] / ms["render"]["median"]))
    v = res["verify_end_to_end_ms"]
    lines.append("verify() end to end (%d renders, %d chunk(s); events, median of 3 calls): %.1f ms (%.1f - %.1f), wall %.1f ms"
                 % (n, v["chunks"], v["median"], v["min"], v["max"], v["wall_ms_mean"]))
    lines.append("median score: ground truth %.4f, the nearer half of the estimates %.4f, the farther half %.4f (iou %.4f, agreement %.4f over all estimates)"
                 % tuple(res["score_median"][k] for k in ("truth", "estimates_nearer_half", "estimates_farther_half", "estimates_iou", "estimates_agreement")))
    lines.append("instance path, one 480 x 640 frame at batch 1, R = %d, host PnP, %d instances found (wall, median of %d alternating frames): without scores %.2f ms "
                 "(%.2f - %.2f), with verified scores %.2f ms (%.2f - %.2f)"
                 % (R, found, inst["with"]["frames"], inst["without"]["median"], inst["without"]["min"], inst["without"]["max"], inst["with"]["median"],
                    inst["with"]["min"], inst["with"]["max"]))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
