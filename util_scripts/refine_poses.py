#!/usr/bin/env python3
"""Refine the poses of a BOP result file against the sensor's depth images (projective point-to-plane ICP on the GPU) and write a result file
with the same rows in the same order:

    python util_scripts/refine_poses.py --result_file <out>/bop_evaluation.csv --dataset_path <bop>/<name> [--split test]
                                        [--model_folder models_eval] [--depth_folder depth] [--iterations 8] [--gate 0.25] --out <refined.csv>

The result file is what test_casapose.py and test_minimal.py write with --write_poses 1.  Cameras and each image's `depth_scale` are read from
<dataset_path>/<split>/<scene>/scene_camera.json as util_scripts/bop_score.py reads them, meshes (with faces) from <dataset_path>/<model_folder>,
diameters from its models_info.json, depth images from <split>/<scene>/<depth_folder>/NNNNNN.png.  Every row that is an estimate (a non-zero
score and pose) is refined (casapose_amd/pose_estimation/depth_refine.py).  A row that is "not found" passes through byte for byte; a row
whose refinement was rejected keeps the text of its pose.  A `time` of -1 stays -1; any other time of an estimate gets its image's share of
the measured refinement time added, whether the refinement was kept or rejected, so that the estimates of one image carry one time (the
share: the time of the whole call times the image's fraction of the rows that went through the loop).  An estimate of an object that has no
mesh or no models_info.json entry cannot be rendered: it keeps its pose, takes its image's time, and is counted in the printed summary.  Every depth image that will be read must exist: a missing one stops the run
before any device work.  The chain is --write_poses 1 -> refine_poses.py -> bop_score.py --vsd."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bop_score import _object_id, load_depth_scales, load_ground_truth  # noqa: E402
from casapose_amd.data_handler.model_prep import find_meshes  # noqa: E402
from casapose_amd.data_handler.vectorfield_dataset import read_faces, read_vertices  # noqa: E402
from casapose_amd.pose_estimation.bop_scores import is_estimate, read_bop_results  # noqa: E402
from casapose_amd.pose_estimation.bop_vsd import depth_path, read_depth  # noqa: E402
from casapose_amd.pose_estimation.depth_refine import REFINED, STATUS_NAMES, DeviceDepthRefiner  # noqa: E402
from casapose_amd.utils.io_utils import BOP_HEADER  # noqa: E402


def data_lines(path: str):
    """the file's lines as read_bop_results counts them: (header or None, the lines of its rows)"""
    header, rows = None, []
    with open(path) as f:
        for no, line in enumerate(f):
            if no == 0 and line.strip().startswith("scene_id"):
                header = line
            elif line.strip():
                rows.append(line)
    return header, rows


def row_text(line: str, pose, add_time: float) -> str:
    """the row `line` with `pose` (float64, written so that it reads back bit for bit; None keeps the row's own pose text) and add_time seconds
    added to a time that is not -1; a row that changes in neither is returned as it is"""
    part = [p.strip() for p in line.split(",")]
    t = float(part[6])
    if pose is None and (t == -1.0 or add_time == 0.0):
        return line
    numbers = lambda a: " ".join(repr(float(x)) for x in a)   # noqa: E731
    R, tr = (part[4], part[5]) if pose is None else (numbers(pose[:, :3].reshape(-1)), numbers(pose[:, 3]))
    return "%s,%s,%s,%s,%s,%s,%s\n" % (part[0], part[1], part[2], part[3], R, tr, part[6] if t == -1.0 else repr(t + add_time))


def main(argv=None):
    ap = argparse.ArgumentParser(description="refine the poses of a BOP result file against the sensor's depth images")
    ap.add_argument("--result_file", required=True)
    ap.add_argument("--dataset_path", required=True, help="<bop>/<name>")
    ap.add_argument("--split", default="test")
    ap.add_argument("--model_folder", default="models_eval")
    ap.add_argument("--depth_folder", default="depth")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--gate", type=float, default=0.25, help="in object diameters")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)

    split_path = os.path.join(a.dataset_path, a.split)
    model_path = os.path.join(a.dataset_path, a.model_folder)
    with open(os.path.join(model_path, "models_info.json")) as f:
        infos = {_object_id(k): v for k, v in json.load(f).items()}
    model_files = {_object_id(name): path for name, path in find_meshes(model_path).items()}
    ids = sorted(o for o in model_files if o in infos)
    if not ids:
        raise FileNotFoundError("no mesh under %s has an entry in its models_info.json" % model_path)
    _, cameras = load_ground_truth(split_path)
    scales, folders = load_depth_scales(split_path)
    results = read_bop_results(a.result_file)
    header, lines = data_lines(a.result_file)
    if len(lines) != len(results["score"]):
        raise ValueError("%s: %d rows were read from %d lines" % (a.result_file, len(results["score"]), len(lines)))
    keys = [(int(s), int(i)) for s, i in zip(results["scene_id"], results["im_id"])]
    estimates = [int(r) for r in np.flatnonzero(is_estimate(results["score"], results["pose"]))]
    rows = [r for r in estimates if int(results["obj_id"][r]) in ids]
    no_mesh = [r for r in estimates if int(results["obj_id"][r]) not in ids]      # cannot be rendered: they keep their pose
    depth_files = {}
    for r in rows:
        key = keys[r]
        if key not in cameras or key not in scales:
            raise KeyError("scene %d, image %d of %s has no entry in scene_camera.json" % (key[0], key[1], a.result_file))
        if key not in depth_files:
            depth_files[key] = depth_path(split_path, folders[key[0]], a.depth_folder, key[1])
            if not os.path.isfile(depth_files[key]):
                raise FileNotFoundError("the refinement needs the depth image %s" % depth_files[key])

    poses, info, seconds = np.zeros((0, 3, 4)), None, 0.0
    if rows:
        refiner = DeviceDepthRefiner([read_vertices(model_files[o]) for o in ids], [read_faces(model_files[o]) for o in ids], "cuda:0")
        index = {key: n for n, key in enumerate(depth_files)}
        depths = [read_depth(depth_files[key], scales[key]) for key in depth_files]
        start = time.perf_counter()
        poses, info = refiner.refine(results["pose"][rows], np.stack([cameras[keys[r]] for r in rows]), [ids.index(int(results["obj_id"][r])) for r in rows],
                                     [index[keys[r]] for r in rows], depths, [float(infos[int(results["obj_id"][r])]["diameter"]) for r in rows],
                                     iterations=a.iterations, gate=a.gate)
        seconds = time.perf_counter() - start
    per_image = {}
    for r in rows:
        per_image[keys[r]] = per_image.get(keys[r], 0) + 1
    share = {key: seconds * n / len(rows) for key, n in per_image.items()}
    out = list(lines)
    for n, r in enumerate(rows):      # a rejected estimate was rendered and stepped like a kept one: it keeps its pose text and takes the time
        out[r] = row_text(lines[r], poses[n] if info["status"][n] == REFINED else None, share[keys[r]])
    for r in no_mesh:                 # one time per image, whatever became of the row
        out[r] = row_text(lines[r], None, share.get(keys[r], 0.0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(header if header is not None else BOP_HEADER)
        f.writelines(out)

    counts = np.bincount(info["status"], minlength=len(STATUS_NAMES)) if rows else np.zeros(len(STATUS_NAMES), int)
    kept = ", ".join("%d %s" % (counts[k], STATUS_NAMES[k]) for k in range(1, len(STATUS_NAMES)) if counts[k]) or "none"
    ok = info["status"] == REFINED if rows else np.zeros(0, bool)
    med = lambda a: float(np.median(a[ok])) if ok.any() else float("nan")   # noqa: E731
    if no_mesh:
        kept += "; %d estimate(s) of objects without a mesh or a models_info.json entry were not refined" % len(no_mesh)
    print("%d rows, %d estimates: %d refined; kept unchanged: %s; median RMS residual of the refined rows %.3f mm -> %.3f mm; %.3f s"
          % (len(lines), len(estimates), int(ok.sum()), kept, med(info["rms_first"]) if rows else float("nan"), med(info["rms_last"]) if rows else float("nan"),
             seconds))
    return dict(rows=len(lines), estimates=len(estimates), no_mesh=len(no_mesh), refined=int(ok.sum()), status=[int(s) for s in info["status"]] if rows else [], seconds=seconds)


if __name__ == "__main__":
    main()
