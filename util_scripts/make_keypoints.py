#!/usr/bin/env python3
"""Keypoint files and models_info.json for a folder of meshes:

    python util_scripts/make_keypoints.py --model_folder <dir> [--out <dir>] [--no_points 9] [--renderer device|host]

<dir> holds the meshes in BOP's layout (<dir>/<name>.ply or .obj) or the reader's (<dir>/<name>/<name>.obj or .ply).  Written under --out (default:
the model folder itself) in the layout VectorfieldDataset reads: <out>/<name>/<name>_keypoints.ply -- the box centre and no_points - 1
farthest-point samples of the vertices -- and <out>/models_info.json with diameter, min_* and size_* per mesh; other fields of an existing
<dir>/models_info.json (symmetries) are carried over.  With another --out the meshes are copied there as well.  --renderer host runs the kernel's
serial twin on the CPU.  The work is casapose_amd/data_handler/model_prep.py."""
import argparse
import json
import os
import sys
from shutil import copyfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from casapose_amd.data_handler.model_prep import find_meshes, model_prep_for, write_keypoints_ply, write_models_info  # noqa: E402
from casapose_amd.data_handler.vectorfield_dataset import read_vertices  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="keypoint files and models_info.json for a folder of meshes")
    ap.add_argument("--model_folder", required=True)
    ap.add_argument("--out", default=None, help="default: the model folder")
    ap.add_argument("--no_points", type=int, default=9, help="keypoints per object, the centre included")
    ap.add_argument("--renderer", choices=("device", "host"), default="device")
    a = ap.parse_args(argv)
    out = a.out or a.model_folder
    files = find_meshes(a.model_folder)
    if not files:
        raise FileNotFoundError("no .ply or .obj meshes under %s" % a.model_folder)
    results = model_prep_for(a.renderer).run({name: read_vertices(f) for name, f in files.items()}, a.no_points, a.renderer)
    existing = None
    if os.path.isfile(os.path.join(a.model_folder, "models_info.json")):
        with open(os.path.join(a.model_folder, "models_info.json")) as f:
            existing = json.load(f)
    for name, f in files.items():
        os.makedirs(os.path.join(out, name), exist_ok=True)
        target = os.path.join(out, name, os.path.basename(f))
        if os.path.abspath(out) != os.path.abspath(a.model_folder) and not os.path.exists(target):
            copyfile(f, target)
        write_keypoints_ply(os.path.join(out, name, name + "_keypoints.ply"), results[name]["keypoints"])
        print("%s: %d vertices, diameter %.6g" % (name, results[name]["vertices"], results[name]["diameter"]))
    write_models_info(os.path.join(out, "models_info.json"), results, existing)


if __name__ == "__main__":
    main()
