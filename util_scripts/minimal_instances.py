#!/usr/bin/env python3
"""util_scripts/test_minimal.py with several instances of one object per image: the same command line, inputs and timing, the voter and the
PnP keyed by (object, instance) (pose_estimation/instance_voting.py).

    CASAPOSE_MAX_INSTANCES=4 python util_scripts/minimal_instances.py -c config/config_8.ini --datatest <folder> --datameshes <models> --load_h5_weights 1

With CASAPOSE_MAX_INSTANCES unset or 1 this IS test_minimal.py: its main() is called and nothing else happens.  With R in 2..16 the voter is
InstanceLSVoting and the solve poses_pnp_instances, both inside a frame's measured time; the script says `instances: up to R per object`,
<evalf>/poses_est.csv (with --write_poses 1) has the two trailing columns `instance,pixels` and one row per found instance in slot order -- an
object without any gets one zero row with instance 0 and pixels 0 -- and main() returns poses [oc, R, 3, 4] per name.  header_eval.txt,
speed_eval.csv and `average speed:` are test_minimal.py's.  The switch does not combine with CASAPOSE_UNCERTAINTY_PNP=1 or
CASAPOSE_MASK_REFINE=1 (keypoint covariances and the mask refinement are per object): refused by name before any device work.
test_minimal.py itself does not read the switch.

CASAPOSE_INSTANCE_SPLIT=votes (with CASAPOSE_MAX_INSTANCES set; refused by name without it) separates the instances by their votes for the
object's centre instead of by connected components (InstanceLSVoting(split="votes"), cp_vote_split_labels): the script then also says
`instances: split by centre votes` once, and poses_est.csv has one more trailing column `votes` after `instance,pixels`, the votes of the
instance's peak.  Unset or `components`: nothing changes.

CASAPOSE_INSTANCE_VOTER=robust (with CASAPOSE_MAX_INSTANCES set; refused by name without it) votes with the robust voter per slot
(InstanceLSVoting(voter="robust"), cp_ls_vote_slots_robust_f32: two reweighted passes at a cut-off of 4 px reject the pixels a split hands to
the wrong instance): the script then also says `instances: robust voter (cutoff 4 px, 2 passes)` once, and poses_est.csv has one more trailing
column `kept` after whatever columns are there, the share of the plain weight the last pass kept, averaged over the instance's keypoints.  Unset
or `ls`: nothing changes.

CASAPOSE_INSTANCE_PNP=weighted (with CASAPOSE_MAX_INSTANCES set; refused by name without it) weights the PnP of every instance by a covariance
per keypoint (InstanceLSVoting(covariance=True), cp_ls_slot_covariance_f32: one more pass over the slot map; poses_pnp_instances(cov=), on the
host PnP and under CASAPOSE_DEVICE_PNP=1; either split, either voter): the script then also says `instances: covariance-weighted PnP` once,
and poses_est.csv has one more trailing column `weighted` after whatever columns are there, 1 where the instance's solve was weighted and 0
where it fell back to the unweighted one.  Unset or `plain`: nothing changes.  CASAPOSE_UNCERTAINTY_PNP=1 stays refused: that covariance is
the per-object RANSAC one.

CASAPOSE_INSTANCE_SCORE=verify (with CASAPOSE_MAX_INSTANCES set; refused by name without it) scores every found instance against the slot map
and the vector field (pose_estimation/pose_verify.py: the instance's mesh rendered at its pose, cp_pose_verify_i32; it needs the objects' mesh
files under --datameshes; either split, either voter, either PnP), inside the frame's measured time: the script then also says
`instances: verified scores` once, poses_est.csv has one more trailing column `score` after whatever columns are there, and with
--write_poses 1 <evalf>/bop_instances.csv holds one row of BOP's result format per found instance (scene_id and im_id from the first two
numbers of the frame name, scene 0 with a single number; obj_id from the object's name; the verified score; the frame's seconds), which
util_scripts/bop_score.py reads as it is.  Unset or `none`: nothing changes.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "util_scripts"))

import test_minimal  # noqa: E402
from casapose_amd.data_handler.image_only_dataset import ImageOnlyDataset  # noqa: E402
from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset  # noqa: E402
from casapose_amd.pose_estimation.instance_voting import (ENV, ROBUST_CUTOFF, ROBUST_PASSES, InstanceLSVoting,  # noqa: E402
                                                          instance_pnp_from_environment, instance_split_from_environment,
                                                          instance_voter_from_environment,
                                                          max_instances_from_environment, poses_pnp_instances)
from casapose_amd.pose_estimation.pose_verify import instance_score_from_environment  # noqa: E402
from casapose_amd.pose_models.tfkeras import Classifiers  # noqa: E402
from casapose_amd.utils.config_parser import parse_config  # noqa: E402
from casapose_amd.utils.io_utils import latest_checkpoint, write_bop_instances  # noqa: E402


def main(argv=None):
    instances = max_instances_from_environment()
    by_votes = instance_split_from_environment() == "votes"
    robust = instance_voter_from_environment() == "robust"
    weighted_pnp = instance_pnp_from_environment() == "weighted"
    verified = instance_score_from_environment() == "verify"
    if instances is None:
        return test_minimal.main(argv)
    for other in ("CASAPOSE_UNCERTAINTY_PNP", "CASAPOSE_MASK_REFINE"):
        if os.environ.get(other, "0") == "1":
            raise ValueError("minimal_instances.py: %s=%d does not combine with %s=1 (keypoint covariances and the mask refinement are per object)"
                             % (ENV, instances, other))
    opt = parse_config(argv)
    if not torch.cuda.is_available():
        raise SystemExit("minimal_instances.py needs a ROCm GPU (there is no CPU fallback for the product path)")
    if opt.modelname == "pvnet":
        raise SystemExit("minimal_instances.py: modelname pvnet (separated vector fields) has no confidence maps for the LS voting of this script")
    if not opt.estimate_confidence:
        raise SystemExit("minimal_instances.py needs estimate_confidence = 1: the network output is split into [segmentation, vectors, confidences]")
    torch.cuda.set_device(max(opt.gpuids[0], 0))
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(opt.evalf, exist_ok=True)
    os.makedirs(opt.outf + "/control_output", exist_ok=True)
    with open(opt.evalf + "/header_eval.txt", "w") as f:
        f.write(str(opt))
    np.random.seed(opt.manualseed)
    torch.manual_seed(opt.manualseed)

    objectsofinterest = [x.strip() for x in opt.object.split(",")]
    no_objects = len(objectsofinterest)
    height, width = opt.imagesize_test
    frames = ImageOnlyDataset(root=opt.datatest)
    if len(frames) == 0:
        raise SystemExit("minimal_instances.py: no *[0-9].png / *[0-9].jpg frames under %s" % opt.datatest)
    fh, fw, _ = frames.frame_shape()
    if (fh, fw) != (height, width):
        raise SystemExit("minimal_instances.py: frames are %d x %d, imagesize_test is %d x %d (frames are not resized)" % (fh, fw, height, width))
    testing_images, image_batches = frames.generate_dataset(1, device=device)

    # keypoints and camera matrix of the first annotated frame, as test_minimal.py takes them
    annotated = VectorfieldDataset(root=opt.datatest, path_meshes=opt.datameshes, path_filter_root=opt.datatest_path_filter, color_input=opt.color_dataset,
                                   no_points=opt.no_points, objectsofinterest=objectsofinterest, noise=0.00001, contrast=0.00001, brightness=0.00001,
                                   random_translation=(0, 0), random_rotation=0, random_crop=False, wxyz_quaterion_input=opt.datatest_wxyz_quaterion)
    annotated_batches, _ = annotated.generate_dataset(1, 1, 0, opt.imagesize_test, 1.0, 1, no_objects, shuffle=False)
    first = next(annotated_batches, None)
    if first is None:
        raise SystemExit("minimal_instances.py: %s has no annotated frame to take the keypoints and the camera matrix from" % opt.datatest)
    keypoints, camera_matrix = first["keypoints3d"], first["cam_mat"]
    print("testing data: {} batches".format(image_batches))

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
    net.summary()

    with open(opt.evalf + "/speed_eval.csv", "w") as f:
        f.write("batchid,speed \n")
    if opt.write_poses:
        with open(opt.evalf + "/poses_est.csv", "w") as f:
            f.write("name,object," + ",".join("r%d%d" % (i, j) for i in range(1, 4) for j in range(1, 4)) + ",t1,t2,t3,instance,pixels" +
                    (",votes" if by_votes else "") + (",kept" if robust else "") + (",weighted" if weighted_pnp else "") + (",score" if verified else "") + "\n")
        if verified and os.path.exists(opt.evalf + "/bop_instances.csv"):
            os.remove(opt.evalf + "/bop_instances.csv")

    K, kp = 1 + no_objects, opt.no_points
    voter = InstanceLSVoting(name="coords_ls_voting", num_classes=K, num_points=kp, max_instances=instances,
                             split="votes" if by_votes else "components", **(dict(voter="robust") if robust else {}),
                             **(dict(covariance=True) if weighted_pnp else {}))
    print("instances: up to {} per object".format(instances))
    if by_votes:
        print("instances: split by centre votes")
    if robust:
        print("instances: robust voter (cutoff {:g} px, {} passes)".format(ROBUST_CUTOFF, ROBUST_PASSES))
    if weighted_pnp:
        print("instances: covariance-weighted PnP")
    verifier = None
    if verified:
        from casapose_amd.pose_estimation.pose_verify import require_image_frame, verifier_for_dataset, verify_instance_estimates

        # The frames themselves reach the network as they are (their size was checked above; nothing resizes or crops them), so every slot map is
        # in the image's frame.  The camera matrix is the first annotated frame's: its offsets say whether it is the image's, too.
        if first.get("offsets") is None:
            raise ValueError("CASAPOSE_INSTANCE_SCORE=verify needs the offsets of the annotated frame the camera matrix came from: the dataset gave none")
        require_image_frame(first["offsets"], what="CASAPOSE_INSTANCE_SCORE=verify")
        verifier = verifier_for_dataset(annotated, opt.datameshes, objectsofinterest, device)
        print("instances: verified scores")
    rng = np.random.default_rng(opt.manualseed)
    speed, poses_by_name = [], {}
    for batch_idx in range(int(image_batches)):
        img = next(testing_images)
        torch.cuda.synchronize(device)
        start = time.perf_counter()
        out = net([img], training=False)
        seg, dirs, conf = torch.split(out, [K, 2 * kp, out.shape[3] - K - 2 * kp], dim=3)
        coords = voter([seg, dirs, conf])
        pixels = voter.last_counts.cpu().numpy()
        votes = voter.last_instances[..., 1].cpu().numpy() if by_votes else None
        kept = voter.last_kept.mean(dim=-1).cpu().numpy() if robust else None
        weighted = None
        if weighted_pnp:
            poses, weighted = poses_pnp_instances(coords, pixels, keypoints, camera_matrix, min_num=opt.min_object_size_test, rng=rng,
                                                  cov=voter.last_cov, return_weighted=True)
        else:
            poses = poses_pnp_instances(coords, pixels, keypoints, camera_matrix, min_num=opt.min_object_size_test, rng=rng)
        scores = None
        if verified:     # the network's output is the field: its directions start behind the K segmentation channels
            scores = verify_instance_estimates(verifier, np.asarray(poses), voter.last_labels, out, keypoints, camera_matrix, dir_off=K)
        seconds = time.perf_counter() - start
        speed.append(seconds)
        with open(opt.evalf + "/speed_eval.csv", "a") as f:
            f.write("{},{:.7f}\n".format(batch_idx + 1, seconds))
        name = frames[batch_idx]["name"]
        poses_by_name[name] = np.asarray(poses)[0]
        if opt.write_poses:
            with open(opt.evalf + "/poses_est.csv", "a") as f:
                for o, obj in enumerate(objectsofinterest):
                    found = [r for r in range(instances) if poses_by_name[name][o, r].any()]
                    for r in found or [0]:
                        P = poses_by_name[name][o, r]
                        f.write("{},{},".format(name, obj) + ",".join("{:.9g}".format(v) for v in np.concatenate([P[:, :3].reshape(-1), P[:, 3]])) +
                                ",{},{}".format(r, int(pixels[0, o, r]) if found else 0) +
                                (",{}".format(int(votes[0, o, r]) if found else 0) if by_votes else "") +
                                (",{:.6g}".format(float(kept[0, o, r]) if found else 0.0) if robust else "") +
                                (",{}".format(int(weighted[0, o, r]) if found else 0) if weighted_pnp else "") +
                                (",{!r}".format(float(scores[0, o, r]) if found else 0.0) if verified else "") + "\n")
            if verified:
                write_bop_instances(opt.evalf + "/bop_instances.csv", name, objectsofinterest, poses_by_name[name], scores[0], seconds)
    print("average speed: {}".format(float(np.mean(speed[10:])) if len(speed) > 10 else float("nan")))
    return {"speed": speed, "poses": poses_by_name}


if __name__ == "__main__":
    main()
