#!/usr/bin/env python3
"""Golden files for the BOP converter (casapose_amd/data_handler/bop_converter.py), written by the REFERENCE'S OWN functions executed here.  They
live in modules that import pyrender / trimesh / TensorFlow at the top, so they are extracted with `ast` and compiled alone (see
make_geometry_golden.py):

    util_scripts/dataset_converter.py:   get_cam_matrix_bop, load_json_info, create_ndds_json, write_camera_setting, write_object_settings
    casapose/utils/geometry_utils.py:    project, matrix_to_quaternion, create_transformation_matrix, get_horizontal_width_angle
    casapose/utils/io_utils.py:          to_json

    python tests/golden/make_bop_converter_golden.py      # needs the reference tree; writes tests/golden/bop_converter/

bop_converter/scene/       a hand-written BOP scene: two frames, three objects (ids 1, 5, 12; object 5 twice in frame 1), integer and float
                           translations, a second camera for frame 1
bop_converter/meshes.json  the hand-built `meshes` dict (what load_object would return, without the renderer's mesh)
bop_converter/with_info/   NNNNNN.json, _camera_settings.json, _object_settings.json as the reference writes them with scene_gt_info.json
bop_converter/without_info/  the same without it.  There the reference's create_ndds_json raises KeyError 'bb' (load_json_info sets "bb" from
                           scene_gt_info.json only): reference_raises.json records that, and the files are what it writes once every ground-truth
                           entry has been given BOP's empty box [-1, -1, -1, -1], the value this build writes in that case."""
import ast
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CASAPOSE_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "bop_converter")


def extract(path, want, ns):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    mod = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want], type_ignores=[])
    exec(compile(mod, path + " (reference, extracted)", "exec"), ns)
    assert set(want) <= set(ns), sorted(set(want) - set(ns))
    return ns


def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def scene():
    def entry(obj, axis, angle, t):
        return {"cam_R_m2c": rot(axis, angle).reshape(-1).tolist(), "cam_t_m2c": t, "obj_id": obj}

    gt = {"0": [entry(1, (1, 2, 3), 0.7, [12.5, -40.25, 812.0]), entry(5, (3, -1, 2), 1.9, [-110, 60, 950]), entry(12, (0, 0, 1), 3.0, [200.75, 10.5, 1234.5])],
          "1": [entry(5, (-1, 1, 4), 2.6, [30.0, 20.0, 700.0]), entry(5, (1, 0, 0), 3.1, [-75.5, -20.0, 1500.25]), entry(1, (2, 2, -1), 0.01, [0.0, 0.0, 640.0])]}
    cam = {"0": {"cam_K": [572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0], "depth_scale": 1.0},
           "1": {"cam_K": [1066.778, 0.0, 312.9869, 0.0, 1067.487, 241.3109, 0.0, 0.0, 1.0], "depth_scale": 0.1}}

    def info(all_, valid, visib, bb, bbv):
        return {"bbox_obj": bb, "bbox_visib": bbv, "px_count_all": all_, "px_count_valid": valid, "px_count_visib": visib, "visib_fract": visib / all_ if all_ else 0.0}

    gt_info = {"0": [info(5120, 5120, 4096, [300, 180, 80, 75], [300, 190, 70, 65]), info(2400, 2300, 2400, [220, 250, 60, 50], [220, 250, 60, 50]),
                     info(900, 900, 0, [400, 230, 30, 31], [-1, -1, -1, -1])],
               "1": [info(7000, 7000, 6999, [310, 230, 100, 90], [310, 230, 100, 90]), info(1200, 1100, 300, [250, 200, 40, 41], [260, 210, 20, 21]),
                     info(0, 0, 0, [-1, -1, -1, -1], [-1, -1, -1, -1])]}
    return gt, cam, gt_info


def meshes_data():
    out = {}
    rng = np.random.default_rng(21)
    for obj, axes in ((1, (40.0, 30.0, 35.0)), (5, (30.0, 45.0, 25.0)), (12, (60.5, 20.25, 33.0))):
        kp = rng.uniform(-1, 1, (9, 3)) * np.asarray(axes)
        lo, hi = -np.asarray(axes), np.asarray(axes)
        vol = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        out[str(obj)] = {"name": "obj_%06d" % obj, "keypoints": kp.tolist(), "volume": vol.tolist(), "volume_size": (kp.max(0) - kp.min(0)).tolist(),
                         "center": ((kp.max(0) + kp.min(0)) / 2.0).tolist(), "fixed_model_transform": np.eye(4).tolist(), "id": obj}
    return out


def load_meshes(data):
    return {int(k): dict(name=m["name"], keypoints=np.array(m["keypoints"]), volume=np.array(m["volume"]), volume_size=np.array(m["volume_size"]),
                         center=np.array(m["center"]), counter=0, fixed_model_transform=np.array(m["fixed_model_transform"]), id=m["id"])
            for k, m in data.items()}


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree at %s" % REF)
    ns = {"np": np, "json": json, "os": os}
    extract("casapose/utils/io_utils.py", ["to_json"], ns)
    extract("casapose/utils/geometry_utils.py", ["project", "matrix_to_quaternion", "create_transformation_matrix", "get_horizontal_width_angle"], ns)
    extract("util_scripts/dataset_converter.py", ["get_cam_matrix_bop", "load_json_info", "create_ndds_json", "write_camera_setting", "write_object_settings"], ns)
    os.makedirs(os.path.join(OUT, "scene"), exist_ok=True)
    gt, cam, gt_info = scene()
    for name, data in (("scene_gt.json", gt), ("scene_camera.json", cam), ("scene_gt_info.json", gt_info)):
        json.dump(data, open(os.path.join(OUT, "scene", name), "w"), indent=1)
    meshes = meshes_data()
    json.dump(meshes, open(os.path.join(OUT, "meshes.json"), "w"), indent=1)
    for variant in ("with_info", "without_info"):
        d = os.path.join(OUT, variant)
        os.makedirs(d, exist_ok=True)
        files = [os.path.join(OUT, "scene", n) for n in ("scene_camera.json", "scene_gt.json") + (("scene_gt_info.json",) if variant == "with_info" else ())]
        info, gts = ns["load_json_info"](sorted(files))
        m = load_meshes(meshes)
        if variant == "without_info":
            try:
                ns["create_ndds_json"](os.path.join(d, "000000.json"), info[0]["cam_mat"], gts[0], load_meshes(meshes))
                sys.exit("the reference no longer raises without scene_gt_info.json: rewrite this generator and the converter's default")
            except KeyError as e:
                json.dump({"error": "KeyError", "key": e.args[0], "bb_given": [-1, -1, -1, -1]}, open(os.path.join(d, "reference_raises.json"), "w"))
            for idx in gts:
                for g in gts[idx]:
                    g["bb"] = [-1, -1, -1, -1]
        ns["write_camera_setting"](os.path.join(d, "_camera_settings.json"), "Viewpoint", next(iter(info.values()))["cam_mat"], 640, 480)
        for idx in sorted(gts):
            m = ns["create_ndds_json"](os.path.join(d, "%06d.json" % idx), info[idx]["cam_mat"], gts[idx], m)
        ns["write_object_settings"](os.path.join(d, "_object_settings.json"), m)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
