#!/usr/bin/env python3
"""BOP scores of a result file: AR_MSSD and AR_MSPD with the objects' symmetries and, with --vsd, AR_VSD and BOP's AR, per object and over all
objects:

    python util_scripts/bop_score.py --result_file <out>/bop_evaluation.csv --dataset_path <bop>/<name> [--split test]
                                     [--model_folder models_eval] [--targets <json>] [--image_width N] [--out scores.json]
                                     [--vsd [--depth_folder depth]]

The result file is what test_casapose.py and test_minimal.py write with --write_poses 1 (BOP's columns scene_id, im_id, obj_id, score, R, t,
time).  Ground truth and cameras are read from <dataset_path>/<split>/<scene>/scene_gt.json, scene_camera.json and, where it exists,
scene_gt_info.json; meshes from <dataset_path>/<model_folder>, diameters and symmetries from its models_info.json.  Without --targets the
instances to be found are those with visib_fract >= 0.1 (every instance where there is no scene_gt_info.json); with it, the entries of BOP's
test_targets file.  The image width (MSPD's thresholds scale with width / 640) is read from the first image of the split unless --image_width
is given.  The errors are computed on the GPU (casapose_amd/pose_estimation/bop_scores.py).  Without --vsd, VSD is not computed and the mean of
the two terms is printed as AR_MSSD_MSPD, not as BOP's AR.  With --vsd the sensor's depth images <split>/<scene>/<depth_folder>/NNNNNN.png are
read with each image's `depth_scale` of scene_camera.json (1.0 where it has none), the meshes' faces are read too, estimates and ground truths
are rendered and compared on the GPU (casapose_amd/pose_estimation/bop_vsd.py), and AR_VSD and AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3 are printed
as well.  Every depth image that will be read must exist: a missing one stops the run before any device work."""
import argparse
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from casapose_amd.data_handler.bop_converter import load_json_info  # noqa: E402
from casapose_amd.data_handler.model_prep import find_meshes  # noqa: E402
from casapose_amd.data_handler.vectorfield_dataset import read_faces, read_vertices  # noqa: E402
from casapose_amd.pose_estimation.bop_scores import DeviceBopScorer, read_bop_results, score, symmetry_transforms  # noqa: E402
from casapose_amd.pose_estimation.bop_vsd import BopVsd, DeviceVsdScorer, depth_path, images_with_pairs, read_depth  # noqa: E402


def _object_id(name) -> int:
    return int(re.findall(r"\d+", str(name))[-1])


def load_ground_truth(split_path: str):
    """({(scene_id, im_id): instances}, {(scene_id, im_id): K}) of every scene folder under the split"""
    gts, cameras = {}, {}
    for scene in sorted(os.listdir(split_path)):
        folder = os.path.join(split_path, scene)
        if not (os.path.isdir(folder) and scene.isdigit() and os.path.isfile(os.path.join(folder, "scene_gt.json"))):
            continue
        files = [os.path.join(folder, n) for n in ("scene_camera.json", "scene_gt.json", "scene_gt_info.json") if os.path.isfile(os.path.join(folder, n))]
        info, gt = load_json_info(files)
        for im, instances in gt.items():
            gts[(int(scene), int(im))] = instances
            cameras[(int(scene), int(im))] = info[im]["cam_mat"]
    return gts, cameras


def load_depth_scales(split_path: str):
    """({(scene_id, im_id): depth_scale}, {scene_id: folder name}) from every scene's scene_camera.json; 1.0 where an image has no depth_scale"""
    scales, folders = {}, {}
    for scene in sorted(os.listdir(split_path)):
        path = os.path.join(split_path, scene, "scene_camera.json")
        if not (scene.isdigit() and os.path.isfile(path)):
            continue
        folders[int(scene)] = scene
        with open(path) as f:
            for im, entry in json.load(f).items():
                scales[(int(scene), int(im))] = float(entry.get("depth_scale", 1.0))
    return scales, folders


def first_image_width(split_path: str) -> int:
    from PIL import Image

    for scene in sorted(os.listdir(split_path)):
        for sub in ("rgb", "gray"):
            files = sorted(glob.glob(os.path.join(split_path, scene, sub, "*.*")))
            if files:
                with Image.open(files[0]) as im:
                    return int(im.size[0])
    raise FileNotFoundError("no image under %s: give --image_width" % split_path)


def main(argv=None):
    ap = argparse.ArgumentParser(description="AR_MSSD and AR_MSPD of a BOP result file; with --vsd also AR_VSD and AR")
    ap.add_argument("--result_file", required=True)
    ap.add_argument("--dataset_path", required=True, help="<bop>/<name>")
    ap.add_argument("--split", default="test")
    ap.add_argument("--model_folder", default="models_eval")
    ap.add_argument("--targets", default=None, help="BOP's test_targets json: a list of {scene_id, im_id, obj_id, inst_count}")
    ap.add_argument("--image_width", type=int, default=None)
    ap.add_argument("--out", default=None, help="write the scores as JSON")
    ap.add_argument("--vsd", action="store_true", help="also compute VSD from the sensor's depth images: AR_VSD and BOP's three-term AR")
    ap.add_argument("--depth_folder", default="depth", help="with --vsd: the depth images' folder inside each scene folder")
    a = ap.parse_args(argv)

    split_path = os.path.join(a.dataset_path, a.split)
    model_path = os.path.join(a.dataset_path, a.model_folder)
    with open(os.path.join(model_path, "models_info.json")) as f:
        infos = {_object_id(k): v for k, v in json.load(f).items()}
    meshes = {_object_id(name): read_vertices(path) for name, path in find_meshes(model_path).items()}
    ids = sorted(o for o in meshes if o in infos)
    if not ids:
        raise FileNotFoundError("no mesh under %s has an entry in its models_info.json" % model_path)
    gts, cameras = load_ground_truth(split_path)
    if not gts:
        raise FileNotFoundError("no scene with a scene_gt.json under %s" % split_path)
    targets = None
    if a.targets:
        with open(a.targets) as f:
            targets = json.load(f)
    width = a.image_width if a.image_width else first_image_width(split_path)
    results = read_bop_results(a.result_file)
    depth_files = {}
    if a.vsd:
        scales, folders = load_depth_scales(split_path)
        for key in images_with_pairs(results, gts, targets):
            depth_files[key] = depth_path(split_path, folders[key[0]], a.depth_folder, key[1])
            if not os.path.isfile(depth_files[key]):
                raise FileNotFoundError("--vsd needs the depth image %s" % depth_files[key])
        model_files = find_meshes(model_path)
        faces = {_object_id(name): read_faces(path) for name, path in model_files.items() if _object_id(name) in ids}

    vmax = max(len(meshes[o]) for o in ids)
    points = np.zeros((len(ids), vmax, 3), np.float32)
    for i, o in enumerate(ids):
        points[i, :len(meshes[o])] = meshes[o]
    scorer = DeviceBopScorer(points, [len(meshes[o]) for o in ids], [symmetry_transforms(infos[o]) for o in ids], "cuda:0")
    vsd = None
    if a.vsd:
        vsd_scorer = DeviceVsdScorer([meshes[o] for o in ids], [faces[o] for o in ids], "cuda:0")
        vsd = BopVsd(vsd_scorer, lambda scene, im: read_depth(depth_files[(scene, im)], scales[(scene, im)]))
    out = score(results, gts, cameras, scorer, ids, {o: float(infos[o]["diameter"]) for o in ids}, targets, float(width), vsd=vsd)

    for o, s in out["objects"].items():
        if a.vsd:
            print("obj %6s: targets %6d  AR_VSD %.4f  AR_MSSD %.4f  AR_MSPD %.4f  AR %.4f" % (o, s["targets"], s["AR_VSD"], s["AR_MSSD"], s["AR_MSPD"], s["AR"]))
        else:
            print("obj %6s: targets %6d  AR_MSSD %.4f  AR_MSPD %.4f  AR_MSSD_MSPD %.4f" % (o, s["targets"], s["AR_MSSD"], s["AR_MSPD"], s["AR_MSSD_MSPD"]))
    if a.vsd:
        print("all objects: targets %6d  AR_VSD %.4f  AR_MSSD %.4f  AR_MSPD %.4f  AR %.4f  (%d pairs, image width %d; %d renders, %d triangles "
              "dropped at the near plane)" % (out["targets"], out["AR_VSD"], out["AR_MSSD"], out["AR_MSPD"], out["AR"], out["pairs"], width,
                                              vsd_scorer.last_renders, vsd_scorer.last_dropped))
    else:
        print("all objects: targets %6d  AR_MSSD %.4f  AR_MSPD %.4f  AR_MSSD_MSPD %.4f  (%d pairs, image width %d; VSD not computed)"
              % (out["targets"], out["AR_MSSD"], out["AR_MSPD"], out["AR_MSSD_MSPD"], out["pairs"], width))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=4)      # repr floats: they read back bit for bit (io_utils.to_json keeps 16 digits)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
