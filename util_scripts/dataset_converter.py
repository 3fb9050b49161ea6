#!/usr/bin/env python3
"""BOP folders -> the layout VectorfieldDataset reads, with the reference's interface (fraunhoferhhi/casapose util_scripts/dataset_converter.py):

    from dataset_converter import generate_data
    generate_data(dataset_path, dataset_path_out, settings, model_folder="models", model_folder_out="models", image_folder="train_pbr")

and, as a command (the settings the reference's trailing comments mark "ADD to command line"):

    python util_scripts/dataset_converter.py --dataset_path <bop>/lmo --dataset_path_out <out>/lmo --image_folder test \
        --model_folder ../lm/models_eval --mask render --gt_info render --copy_meshes

--mask reuse builds NNNNNN.seg.png from mask_visib/, --mask render renders it from the meshes on the GPU (--renderer host: on the CPU, the kernel's
serial twin), --mask none writes no mask.  --gt_info render takes px_count_all, px_count_visib, visibility and both bounding boxes from the
renderer instead of scene_gt_info.json.  --keypoints generate and --models_info generate compute obj_NNNNNN_keypoints.ply and models_info.json
from the meshes (--no_points keypoints, the centre included), for datasets that ship neither.  The work is casapose_amd/data_handler/bop_converter.py."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from casapose_amd.data_handler.bop_converter import (  # noqa: E402,F401
    create_bop_mask,
    create_ndds_json,
    generate_data,
    get_cam_matrix_bop,
    load_json_info,
    load_models_bop,
    load_object,
    parse_bop,
    update_data,
    write_camera_setting,
    write_object_settings,
)


def main(argv=None):
    ap = argparse.ArgumentParser(description="convert one image folder of a BOP dataset to the NDDS layout")
    ap.add_argument("--dataset_path", required=True, help="the BOP dataset, e.g. <bop>/lm")
    ap.add_argument("--dataset_path_out", required=True, help="where the converted dataset goes")
    ap.add_argument("--image_folder", default="train_pbr", help="the folder of scenes under --dataset_path (train_pbr, test, ...)")
    ap.add_argument("--model_folder", default="models", help="the folder with obj_NNNNNN.ply, obj_NNNNNN_keypoints.ply and models_info.json")
    ap.add_argument("--model_folder_out", default="models")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--near", type=float, default=100.0)
    ap.add_argument("--far", type=float, default=2000.0)
    ap.add_argument("--filetype_in", default="png")
    ap.add_argument("--mask", choices=("reuse", "render", "none"), default="reuse")
    ap.add_argument("--gt_info", choices=("file", "render"), default="file")
    ap.add_argument("--mask_sample_offset", type=float, default=0.5, help="0.5: the reference's masks; 0.0: BOP's pixel centres at integers")
    ap.add_argument("--renderer", choices=("device", "host"), default="device")
    ap.add_argument("--copy_meshes", action="store_true")
    ap.add_argument("--keypoints", choices=("file", "generate"), default="file",
                    help="generate: the box centre and farthest-point samples of each mesh instead of obj_NNNNNN_keypoints.ply")
    ap.add_argument("--models_info", choices=("file", "generate"), default="file",
                    help="generate: diameter, min_* and size_* from the vertices instead of an existing models_info.json")
    ap.add_argument("--no_points", type=int, default=9, help="keypoints per object with --keypoints generate, the centre included")
    a = ap.parse_args(argv)
    settings = dict(near=a.near, far=a.far, width=a.width, height=a.height, filetype_in=a.filetype_in, mask=a.mask, copy_meshes=a.copy_meshes,
                    draw_debug_image=False, gt_info=a.gt_info, mask_sample_offset=a.mask_sample_offset, renderer=a.renderer, keypoints=a.keypoints,
                    models_info=a.models_info, no_points=a.no_points)
    generate_data(a.dataset_path, a.dataset_path_out, settings, model_folder=a.model_folder, model_folder_out=a.model_folder_out,
                  image_folder=a.image_folder)


if __name__ == "__main__":
    main()
