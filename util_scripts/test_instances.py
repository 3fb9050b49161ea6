#!/usr/bin/env python3
"""Recall and precision with several instances of one object per image, on the scene sources that carry an instance axis.

    CASAPOSE_MAX_INSTANCES=R python util_scripts/test_instances.py -c config/config_8.ini --datatest synthetic[:N] | meshes:<folder>[:N] ...

The source is built with instances=R and random_crop=False; per image the network runs, InstanceLSVoting votes up to R keypoint sets per object,
poses_pnp_instances solves them, and DeviceInstanceEvaluator (pose_estimation/instance_evaluation.py, cp_pose_match_f32) matches the poses with
the image's ground-truth instances: greedily by ADD (ADD-S for a symmetric object), smallest error first.  The network is loaded as
minimal_instances.py loads it (--load_h5_weights / --net).  CASAPOSE_INSTANCE_SPLIT, CASAPOSE_INSTANCE_VOTER, CASAPOSE_INSTANCE_PNP and
CASAPOSE_DEVICE_PNP act as they do there.  Symmetry flags: for a mesh folder, an object whose models_info.json entry has symmetries_discrete
or symmetries_continuous gets ADD-S; otherwise the vertex-count rule of DevicePoseEvaluator applies.

It writes <evalf>/instance_evaluation.csv (one row per object and one `all` row: gt, est, matched, recall_add, recall_2d, precision_add,
precision_2d and the mean / median errors of the matches) and <evalf>/instance_matches.csv (one row per ground-truth instance), and prints the
overall recall and precision.  Without CASAPOSE_MAX_INSTANCES (or with 1), or with a folder as --datatest, it exits and names the variable or
the source: the folder reader has no instance axis.  A batch whose images do not share one camera matrix is refused by name: the PnP takes one.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from casapose_amd.data_handler import mesh_scene  # noqa: E402
from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset  # noqa: E402
from casapose_amd.pose_estimation.instance_evaluation import (DeviceInstanceEvaluator, crop_cameras, evaluate_instance_batch,  # noqa: E402
                                                              summarise, symmetric_from_models_info, write_instance_evaluation,
                                                              write_instance_matches)
from casapose_amd.pose_estimation.instance_voting import (ENV, InstanceLSVoting, instance_pnp_from_environment,  # noqa: E402
                                                          instance_split_from_environment, instance_voter_from_environment,
                                                          max_instances_from_environment)
from casapose_amd.pose_models.tfkeras import Classifiers  # noqa: E402
from casapose_amd.utils.config_parser import parse_config  # noqa: E402
from casapose_amd.utils.io_utils import latest_checkpoint  # noqa: E402


def shared_camera(cam_mat, offsets, where: str) -> np.ndarray:
    """the one crop camera of a batch, float64 [3, 3]; a batch whose images have different ones is refused"""
    cams = crop_cameras(cam_mat, offsets)
    if not np.allclose(cams, cams[:1], rtol=0.0, atol=1e-9):
        raise SystemExit("test_instances.py: the images of %s do not share one camera matrix (the instance PnP takes one per batch)" % where)
    return cams[0]


def main(argv=None):
    instances = max_instances_from_environment()
    by_votes = instance_split_from_environment() == "votes"
    robust = instance_voter_from_environment() == "robust"
    weighted_pnp = instance_pnp_from_environment() == "weighted"
    if instances is None:
        raise SystemExit("test_instances.py needs %s set to an integer in 2..16: the instances per object to vote, solve and evaluate" % ENV)
    opt = parse_config(argv)
    spec = opt.datatest
    if not (spec.startswith("synthetic") or mesh_scene.is_spec(spec)):
        raise SystemExit("test_instances.py: --datatest %s is a folder, and the folder reader has no instance axis; the sources are "
                         "synthetic[:N] and meshes:<folder>[:N]" % spec)
    if not torch.cuda.is_available():
        raise SystemExit("test_instances.py needs a ROCm GPU (there is no CPU fallback for the product path)")
    if opt.modelname == "pvnet":
        raise SystemExit("test_instances.py: modelname pvnet (separated vector fields) has no confidence maps for the LS voting of this script")
    if not opt.estimate_confidence:
        raise SystemExit("test_instances.py needs estimate_confidence = 1: the network output is split into [segmentation, vectors, confidences]")
    torch.cuda.set_device(max(opt.gpuids[0], 0))
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(opt.evalf, exist_ok=True)
    np.random.seed(opt.manualseed)
    torch.manual_seed(opt.manualseed)

    objectsofinterest = [x.strip() for x in opt.object.split(",")]
    no_objects = len(objectsofinterest)
    height, width = opt.imagesize_test
    seed = (opt.manualseed or 0) + 1
    if mesh_scene.is_spec(spec):
        folder, n = mesh_scene.parse_spec(spec)
        ds = mesh_scene.MeshSceneDataset(folder, no_objects, (height, width), opt.no_points, length=32 if n is None else n, seed=seed, random_crop=False,
                                         instances=instances)
        vertex_array, vertex_count = ds.generate_object_vertex_array()
        symmetric = symmetric_from_models_info(folder, ds.names, vertex_count)
    else:
        n = int(spec.split(":")[1]) if ":" in spec else 32
        ds = SyntheticSceneDataset(no_objects, (height, width), opt.no_points, length=n, seed=seed, random_crop=False, instances=instances)
        vertex_array, vertex_count = ds.generate_object_vertex_array()
        symmetric = None
    batches, count = ds.generate_dataset(1, 1, 0, device=device)
    print("testing data: {} batches".format(count))

    net = Classifiers.get(opt.modelname)(ver_dim=opt.no_points * 3, seg_dim=1 + no_objects, input_shape=(height, width, 3), input_segmentation_shape=None,
                                         weights="imagenet" if opt.pretrained else None, base_model=opt.backbonename, device=device, seed=opt.manualseed)
    if opt.load_h5_weights:
        net.load_weights(opt.outf + "/frozen_model/" + opt.load_h5_filename + ".h5", by_name=True, skip_mismatch=True)
    elif opt.net != "":
        latest = latest_checkpoint(opt.outf + "/" + opt.net)
        if latest is not None:
            net.load_weights(latest[0])
    for layer in net.layers:
        layer.trainable = False

    voter = InstanceLSVoting(name="coords_ls_voting", num_classes=1 + no_objects, num_points=opt.no_points, max_instances=instances,
                             split="votes" if by_votes else "components", **(dict(voter="robust") if robust else {}),
                             **(dict(covariance=True) if weighted_pnp else {}))
    evaluator = DeviceInstanceEvaluator(vertex_array, vertex_count, device, symmetric=symmetric)
    print("instances: up to {} per object, {} split, {} voter, {} PnP; ADD-S for {}".format(
        instances, "vote" if by_votes else "component", "robust" if robust else "ls", "weighted" if weighted_pnp else "plain",
        [o for o, s in zip(objectsofinterest, evaluator.symmetric_host) if s] or "no object"))
    rng = np.random.default_rng(opt.manualseed)
    tallies, records = [], []
    for batch_idx in range(int(count)):
        batch = next(batches)
        camera = shared_camera(batch["cam_mat"], batch["offsets"], "batch %d" % batch_idx)
        out = net([batch["img"].to(device)], training=False)
        _, gt_rec, _, tally = evaluate_instance_batch(batch, out, voter, evaluator, ds.keypoints3d, camera, opt.min_object_size_test, rng=rng,
                                                      cov=weighted_pnp)
        tallies.append(tally)
        records.append(gt_rec)
    tallies, records = np.concatenate(tallies), np.concatenate(records)
    summary = summarise(tallies, records)
    write_instance_evaluation(opt.evalf + "/instance_evaluation.csv", objectsofinterest, summary)
    write_instance_matches(opt.evalf + "/instance_matches.csv", objectsofinterest, tallies, records)
    a = summary["all"]
    print("instances: {} ground truth, {} estimated, {} matched".format(a["gt"], a["est"], a["matched"]))
    print("recall ADD(-S) {:.4f}, 2-D {:.4f}; precision ADD(-S) {:.4f}, 2-D {:.4f}".format(a["recall_add"], a["recall_2d"], a["precision_add"], a["precision_2d"]))
    return {"summary": summary, "tallies": tallies, "gt_rec": records}


if __name__ == "__main__":
    main()
