"""Pose files of an evaluation run, in the reference's on-disk formats (casapose/utils/io_utils.py:54-138, called from
test_casapose.py:392-399 when `--write_poses` is set):

  <path_out>/bop_evaluation.csv                     BOP-challenge result rows `scene_id,im_id,obj_id,score,R,t,time`, one per
                                                    object that is present in the ground truth of the image
  <path_out>/all_poses/poses_init_<name>.txt        every estimate (also false positives), 12 numbers per line
  <path_out>/filtered_poses/poses_gt_<name>.txt     ground truth, zeros where the object is absent
  <path_out>/filtered_poses/poses_init_<name>.txt   estimates, zeros where the object is absent in the ground truth

Host code: strings and a handful of floats per image.
"""
from __future__ import annotations

import os
import re
from typing import Optional, Sequence

import numpy as np

_NUMBER = re.compile(r"\d*\.*\d+")  # the reference's pattern (io_utils.py:60,125)
BOP_HEADER = "scene_id,im_id,obj_id,score,R,t,time\n"
POSE_HEADER = "#r11 r12 r13 r21 r22 r23 r31 r32 r33 tx ty tz\n"


def to_json(o, level=0, INDENT=4, SPACE=" ", NEWLINE="\n") -> str:
    """The reference's JSON text (casapose/utils/io_utils.py:9-51): dicts one key per line, a list on one line unless its LAST element is a
    list, floats as %.16g, NumPy arrays flattened without spaces.  Nested calls use the default layout, as there."""
    pad = SPACE * INDENT
    if isinstance(o, dict):
        head = (NEWLINE + pad * level if level != 0 else "") + "{" + NEWLINE
        rows = [pad * (level + 1) + '"' + str(k) + '":' + SPACE + to_json(v, level + 1) for k, v in o.items()]
        return head + ",\n".join(rows) + NEWLINE + pad * level + "}"
    if isinstance(o, str):
        return '"' + o + '"'
    if isinstance(o, list):
        parts = [to_json(e, level + 1) for e in o]
        if not (o and isinstance(o[-1], list)):
            return "[ " + ", ".join(parts) + " ]"
        inner = NEWLINE + pad * (level + 1)
        return "[ " + inner + (", " + inner).join(parts) + NEWLINE + pad * level + " ]"
    if isinstance(o, bool):
        return "true" if o else "false"
    if isinstance(o, int):
        return str(o)
    if isinstance(o, float):
        return "%.16g" % o
    if isinstance(o, np.ndarray) and np.issubdtype(o.dtype, np.integer):
        return "[" + ",".join(map(str, o.flatten().tolist())) + "]"
    if isinstance(o, np.ndarray) and np.issubdtype(o.dtype, np.inexact):
        return "[" + ",".join("%.16g" % x for x in o.flatten().tolist()) + "]"
    if o is None:
        return "null"
    raise TypeError("Unknown type '%s' for json serialization" % str(type(o)))


def _text(x) -> str:
    while isinstance(x, (list, tuple, np.ndarray)):
        x = x[0]
    if hasattr(x, "numpy"):
        x = x.numpy()
        return _text(x)
    return x.decode("utf-8") if isinstance(x, (bytes, np.bytes_)) else str(x)


def _pose(p) -> np.ndarray:
    p = p.detach().cpu().numpy() if hasattr(p, "detach") else np.asarray(p)
    return p.astype(np.float32).reshape(3, 4)


def _numbers(values) -> str:
    return " ".join(map(str, values))


def _append(path: str, header: str, line: str):
    exists = os.path.isfile(path)
    with open(path, "a") as f:
        if not exists:
            f.write(header)
        f.write(line)


def write_poses(gt_poses, estimated_poses, names: Sequence[str], image_id, path_out: str, time_needed: Optional[float] = None, scores=None):
    """gt_poses [objects,1,3,4] (or [objects,3,4]), estimated_poses [objects,3,4], names = `objectsofinterest`, image_id =
    the batch tuple's entry 12 (`<dir>_<dir>_<file stem>`: its first number is the scene, its second the image).
    score = 1 for a non-zero estimate, 0 for "not found" (all-zero pose); time = -1 when not measured.  scores [objects] (the verified
    scores of pose_estimation/pose_verify.py): a non-zero estimate's score is that value, written as repr(float); "not found" stays 0."""
    gt = np.asarray(gt_poses.detach().cpu() if hasattr(gt_poses, "detach") else gt_poses, np.float32)
    if gt.ndim == 4:
        gt = gt[:, 0]
    found = _NUMBER.findall(_text(image_id))
    scene_id, img_id = int(found[0]), int(found[1])
    time = -1.0 if time_needed is None else float(time_needed)
    if scores is not None:
        scores = np.asarray(scores.detach().cpu() if hasattr(scores, "detach") else scores, np.float64).reshape(-1)
        if len(scores) != len(names):
            raise ValueError("write_poses: scores holds one value per object (got %d for %d objects)" % (len(scores), len(names)))
    all_dir, filtered_dir = path_out + "all_poses/", path_out + "filtered_poses/"
    for d in (path_out, all_dir, filtered_dir):
        os.makedirs(d, exist_ok=True)

    def pose_line(pose):
        return _numbers(pose[:, :3].reshape(-1)) + " " + _numbers(pose[:, 3].reshape(-1)) + "\n"

    zeros = np.zeros((3, 4), np.float32)
    for idx, name in enumerate(names):
        obj_id = int(_NUMBER.findall(name)[0])
        est = _pose(estimated_poses[idx])
        if abs(float(gt[idx].sum())) > 0.0001:
            score = (1.0 if scores is None else float(scores[idx])) if abs(float(est.sum())) > 0 else 0.0
            row = "%d,%d,%d,%s,%s,%s,%s\n" % (scene_id, img_id, obj_id, repr(score), _numbers(est[:, :3].reshape(-1)),
                                               _numbers(est[:, 3].reshape(-1)), str(time))
            _append(path_out + "bop_evaluation.csv", BOP_HEADER, row)
            _append(filtered_dir + "poses_gt_" + name + ".txt", POSE_HEADER, pose_line(_pose(gt[idx])))
            _append(filtered_dir + "poses_init_" + name + ".txt", POSE_HEADER, pose_line(est))
        else:
            _append(filtered_dir + "poses_gt_" + name + ".txt", POSE_HEADER, pose_line(zeros))
            _append(filtered_dir + "poses_init_" + name + ".txt", POSE_HEADER, pose_line(zeros))
        _append(all_dir + "poses_init_" + name + ".txt", POSE_HEADER, pose_line(est))


def write_bop_instances(path: str, frame_name, names: Sequence[str], poses, scores, time_needed: Optional[float] = None):
    """One row of BOP's result format per found instance of a frame, appended to `path` (util_scripts/bop_score.py reads the file as it is):
    poses [objects, R, 3, 4] (the zero pose = an empty slot: no row), scores [objects, R], names = `objectsofinterest` (the first number of a
    name is the obj_id).  scene_id, im_id: the first two numbers of the frame name, as write_poses takes them; with a single number the scene
    is 0.  time = -1 when not measured."""
    found = _NUMBER.findall(_text(frame_name))
    if not found:
        raise ValueError("write_bop_instances: the frame name %r holds no number to take the image id from" % (_text(frame_name),))
    scene_id, img_id = (int(found[0]), int(found[1])) if len(found) > 1 else (0, int(found[0]))
    time = -1.0 if time_needed is None else float(time_needed)
    poses, scores = np.asarray(poses, np.float32), np.asarray(scores, np.float64)
    for idx, name in enumerate(names):
        obj_id = int(_NUMBER.findall(name)[0])
        for r in range(poses.shape[1]):
            est = poses[idx, r]
            if est.any():
                _append(path, BOP_HEADER, "%d,%d,%d,%s,%s,%s,%s\n" % (scene_id, img_id, obj_id, repr(float(scores[idx, r])), _numbers(est[:, :3].reshape(-1)),
                                                                     _numbers(est[:, 3].reshape(-1)), str(time)))


def latest_checkpoint(checkpoint_path: str):
    """(path, number) of the newest `ckpt-<n>.npz` of a run, or None -- tf.train.latest_checkpoint for the checkpoints
    train_casapose.py writes (train_casapose.py:350,393,901)."""
    import glob

    found = []
    for p in glob.glob(os.path.join(checkpoint_path, "ckpt-*.npz")):
        try:
            found.append((int(os.path.basename(p)[5:-4]), p))
        except ValueError:
            pass
    if not found:
        return None
    n, p = max(found)
    return p, n
