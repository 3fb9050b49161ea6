"""Verify estimated poses against the network's own output: a score per estimate.

Every estimate of an image is rendered to a depth plane (the mask renderer, csrc/masks.hip, at the label map's sample offset), and one read-only
kernel (cp_pose_verify_i32, csrc/pose_verify.hip, rules in csrc/verify_math.h) compares each plane with the filtered label map or slot map
(`voter.last_labels`), with the planes of the image's other estimates and with the vector field: how much of the render is hidden by another
estimate, how the visible part falls on the estimate's own label, on background and on other labels, how many pixels the label has in all, and
how many (pixel, keypoint) directions point at the keypoints as the pose projects them.  Eight integers per estimate come back; the ratios and
the score are taken from them on the host.  A chunk is one upload, one render and one verification on the current stream and one copy back.

The counts are the interface.  `score_from_counts` is a starting point, not a measured optimum: it has been looked at on synthetic scenes only.
There is no host fall-back: without a device `verify` raises `CasaposeHipError` unless it is asked for `host=True`, which drives the same calls
through the host twins (the same bytes, for tests and machines without a GPU)."""
from __future__ import annotations

import contextlib
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from .bop_vsd import DEFAULT_FAR, DEFAULT_NEAR
from .depth_refine import MAX_SPLIT
from .mask_refine import gather_meshes, require_image_frame
from .pose_evaluation import _np
from .ransac_voting import INLIER_THRESH
from .refine_common import ChunkedRefiner

COUNT_NAMES = ("rendered", "hidden", "on_label", "on_background", "on_other", "label_pixels", "pairs", "inliers")
RENDERED, HIDDEN, ON_LABEL, ON_BACKGROUND, ON_OTHER, LABEL_PIXELS, PAIRS, INLIERS = range(8)
MAX_KEYPOINTS = 32
DEFAULT_COS_MIN = INLIER_THRESH      # the RANSAC voter's inlier threshold: a direction agrees where the voter would have counted it
WHAT = "CASAPOSE_POSE_SCORE=1"
# blocks per job: a speed setting.  Measured on 2 000 estimates at 480 x 640, 8 per image (tools/pose_verify_probe.py): 0.64 ms at 1, 0.48 at 4,
# 0.40 at 8 and at 16
DEFAULT_SPLIT = 8


def pose_score_enabled() -> bool:
    """CASAPOSE_POSE_SCORE=1; says `score: verified poses` the first time it is"""
    on = os.environ.get("CASAPOSE_POSE_SCORE", "0") == "1"
    if on and not pose_score_enabled.said:
        pose_score_enabled.said = True
        print("score: verified poses (CASAPOSE_POSE_SCORE=1)")
    return on


pose_score_enabled.said = False

ENV_INSTANCE_SCORE = "CASAPOSE_INSTANCE_SCORE"


def instance_score_from_environment() -> str:
    """CASAPOSE_INSTANCE_SCORE (util_scripts/minimal_instances.py): unset or `none` -> "none" (no score column, the existing output); `verify`
    -> "verify" (every instance is scored by verify_instance_estimates), which needs CASAPOSE_MAX_INSTANCES; anything else is an error."""
    from .instance_voting import ENV, MAX_INSTANCES, max_instances_from_environment

    raw = os.environ.get(ENV_INSTANCE_SCORE)
    if raw is None or raw.strip() == "none":
        return "none"
    if raw.strip() != "verify":
        raise ValueError("%s must be unset, `none` or `verify` (got %r)" % (ENV_INSTANCE_SCORE, raw))
    if max_instances_from_environment() is None:
        raise ValueError("%s=verify needs %s set to an integer in 2..%d: without it one instance per object is voted" % (ENV_INSTANCE_SCORE, ENV, MAX_INSTANCES))
    return "verify"


def score_from_counts(counts) -> Dict[str, np.ndarray]:
    """counts int [n, 8] (cp_pose_verify_i32) -> dict of float64 [n] arrays:
      iou        on_label / (label_pixels + on_background): the visible render against the label's pixels.  Pixels the render puts on another
                 label are neutral -- an occluder the network has labelled is not held against the pose, as the mask refiner distrusts edges
                 towards another label -- and so are pixels another estimate hides
      agreement  inliers / pairs: the share of the directions on the overlap that point at the projected keypoints
      visible    (rendered - hidden) / rendered
      score      iou * agreement
    each 0 where its denominator is 0."""
    c = np.asarray(counts, np.float64).reshape(-1, len(COUNT_NAMES))

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros(len(c), np.float64), where=b > 0)

    iou = ratio(c[:, ON_LABEL], c[:, LABEL_PIXELS] + c[:, ON_BACKGROUND])
    agreement = ratio(c[:, INLIERS], c[:, PAIRS])
    visible = ratio(c[:, RENDERED] - c[:, HIDDEN], c[:, RENDERED])
    return dict(iou=iou, agreement=agreement, visible=visible, score=iou * agreement)


def project_keypoints(poses: np.ndarray, cams: np.ndarray, keypoints3d: np.ndarray) -> np.ndarray:
    """poses [n, 12], cams [n, 4] (fx, fy, cx, cy), keypoints3d [n, kp, 3] -> float64 [n, kp, 2] as (y, x) pixels; NaN for a keypoint at or behind
    the camera plane (it makes no pair)"""
    P = poses.reshape(-1, 3, 4)
    X = np.einsum("nij,nkj->nki", P[:, :, :3], keypoints3d) + P[:, None, :, 3]
    with np.errstate(all="ignore"):
        z = np.where(X[..., 2] > 0.0, X[..., 2], np.nan)
        x = cams[:, None, 0] * X[..., 0] / z + cams[:, None, 2]
        y = cams[:, None, 1] * X[..., 1] / z + cams[:, None, 3]
    return np.ascontiguousarray(np.stack([y, x], axis=-1))


class DevicePoseVerifier(ChunkedRefiner):
    """verts, faces: one [V, 3] and one [T, 3] array per object (object_index in `verify` indexes them), uploaded once.  `near`, `far` (in the
    meshes' unit) bound the rendered depths; `workspace_cap` bounds the bytes of depth planes of one chunk.  `sample_offset` is where a pixel
    of the label map was sampled: 0.5, the convention of the reader's masks (data_handler/bop_converter.py)."""

    def __init__(self, verts: Sequence, faces: Sequence, device, near: float = DEFAULT_NEAR, far: float = DEFAULT_FAR,
                 workspace_cap: Optional[int] = None, sample_offset: float = 0.5):
        super().__init__(verts, faces, device, near, far, workspace_cap, sample_offset)
        self.last_counts = None    # verify_estimates / verify_instance_estimates: the counts of the last call, int32 [b, oc(, R), 8]
        self.last_scores = None    # ... and its scores, float64 [b, oc(, R)]

    def count(self, c: dict, labels, field, images: int, ld: int, dir_off: int, kp: int, kp2d: np.ndarray, jobs: np.ndarray, cos_min: float, split: int):
        """cp_pose_verify_i32 (or its host twin) over the chunk's render -> the counts, where the chunk runs"""
        from .. import twin

        dev = c["device"]
        size = int(self._lib.cp_pose_verify_workspace_bytes(images))
        if size == 0:
            raise ValueError("the verifier takes at most 2^22 images in one call (got %d)" % images)
        out = twin.alloc(dict(counts=((len(jobs), len(COUNT_NAMES)), np.int32), work=((size // 4,), np.int32)), dev)
        twin.call("cp_pose_verify_i32", c["planes"], c["records"], c["slots"], c["H"], c["W"], c["packed"]["inst_counts"], c["frames"],
                  c["slots"] // c["frames"], labels, field, images, ld, int(dir_off), int(kp), twin.array(kp2d, np.float64, dev), twin.array(jobs, np.int32, dev),
                  len(jobs), self.sample_offset, float(cos_min), int(split), out["counts"], out["work"], size, host=dev is None, stream=c["stream"])
        return out["counts"]

    def verify(self, poses, K, object_index, image_index, labels, label_of, field, keypoints3d, dir_off: int, cos_min: float = DEFAULT_COS_MIN,
               split: int = DEFAULT_SPLIT, host: bool = False, workspace_cap: Optional[int] = None) -> Dict[str, np.ndarray]:
        """-> dict(counts int32 [n, 8] in the order of COUNT_NAMES, iou, agreement, visible, score float64 [n]).  poses [n, 3, 4] (or [n, 12])
        float64, model -> camera in the meshes' unit; K [n, 3, 3] or one [3, 3], of which fx, fy, cx, cy are read (one camera per image: the
        first estimate's); object_index [n] into the meshes and into keypoints3d [objects, kp, 3]; image_index [n] into `labels`, a uint8
        [images, H, W] device tensor (a NumPy array with host=True) in the frame of K, 0 = background, and into `field`, float32
        [images, H, W, ld] beside it, in which keypoint k's direction is (dy, dx) at dir_off + 2k; label_of [n]: the label value of each
        estimate, 1 .. 255.

        The estimates of an image hide each other, so they share one render frame: more than 256 of one image raise ValueError.  Images are
        cut into chunks under `workspace_cap` (depth planes); no result depends on the cut."""
        if not host and self.device is None:
            raise self._lib_module.CasaposeHipError("DevicePoseVerifier was built without a device; there is no host fall-back (ask for host=True)")
        est = _np(poses, np.float64).reshape(-1, 12)
        obj = _np(object_index, np.int64).reshape(-1)
        img = _np(image_index, np.int64).reshape(-1)
        lab = _np(label_of, np.int64).reshape(-1)
        n = len(obj)
        if not (len(est) == len(img) == len(lab) == n):
            raise ValueError("poses, object_index, image_index and label_of must have one entry per estimate")
        if not (0.0 <= cos_min <= 1.0):
            raise ValueError("cos_min must lie in [0, 1] (got %r)" % (cos_min,))
        if not 1 <= int(split) <= MAX_SPLIT:
            raise ValueError("split must lie in [1, %d] (got %d)" % (MAX_SPLIT, split))
        if len(np.shape(labels)) != 3 or str(labels.dtype).split(".")[-1] != "uint8":
            raise ValueError("labels is a uint8 [images, H, W] array (got %s %s)" % (str(labels.dtype), tuple(np.shape(labels))))
        if host != isinstance(labels, np.ndarray) or host != isinstance(field, np.ndarray):
            raise ValueError("labels and field are device tensors, or NumPy arrays with host=True")
        images, H, W = (int(s) for s in np.shape(labels))
        if len(np.shape(field)) != 4 or tuple(np.shape(field)[:3]) != (images, H, W) or str(field.dtype).split(".")[-1] != "float32":
            raise ValueError("field is a float32 [images, H, W, ld] array beside labels %s (got %s %s)" % ((images, H, W), str(field.dtype), tuple(np.shape(field))))
        ld = int(np.shape(field)[3])
        kps = _np(keypoints3d, np.float64)
        if kps.ndim != 3 or kps.shape[0] != self.objects or kps.shape[2] != 3 or not 1 <= kps.shape[1] <= MAX_KEYPOINTS:
            raise ValueError("keypoints3d is [objects = %d, kp in 1 .. %d, 3] (got %s)" % (self.objects, MAX_KEYPOINTS, kps.shape))
        kp = int(kps.shape[1])
        if int(dir_off) < 0 or int(dir_off) + 2 * kp > ld:
            raise ValueError("the field holds %d words per pixel: dir_off %d + 2 x %d keypoints do not fit" % (ld, dir_off, kp))
        if n and (obj.min() < 0 or obj.max() >= self.objects):
            raise ValueError("object_index must lie in [0, %d)" % self.objects)
        if n and (img.min() < 0 or img.max() >= images):
            raise ValueError("image_index must lie in [0, %d)" % images)
        if n and (lab.min() < 1 or lab.max() > 255):
            raise ValueError("label_of must lie in [1, 255]")
        cams = _np(K, np.float64)
        cams = np.broadcast_to(cams.reshape(-1, 3, 3), (n, 3, 3)) if n else cams.reshape(-1, 3, 3)
        counts = np.zeros((n, len(COUNT_NAMES)), np.int32)
        self.last_chunks = self.last_renders = 0

        from ..data_handler.bop_converter import MAX_INSTANCES

        members: Dict[int, List[int]] = {}
        for p in range(n):
            members.setdefault(int(img[p]), []).append(p)
        members = dict(sorted(members.items()))      # in image order, so that a chunk's images are a range
        for m, rows in members.items():
            if len(rows) > MAX_INSTANCES:
                raise ValueError("image %d has %d estimates; they hide each other, so they share one render frame of at most %d" % (m, len(rows), MAX_INSTANCES))
        image_cams = np.zeros((images, 4), np.float64)
        for m, rows in members.items():
            k = cams[rows[0]]
            image_cams[m] = (k[0, 0], k[1, 1], k[0, 2], k[1, 2])
        cap = self.workspace_cap if workspace_cap is None else int(workspace_cap)
        on_device = contextlib.nullcontext()
        if not host:
            import torch

            on_device = torch.cuda.device(self.device)      # the launches go to the calling thread's current device
            labels, field = labels.to(self.device).contiguous(), field.to(self.device).contiguous()
        else:
            labels, field = np.ascontiguousarray(labels), np.ascontiguousarray(field)
        if n:
            kp2d = project_keypoints(est, image_cams[img], kps[obj])
            imax, chunks = self.frame_chunks(members, H, W, lambda slots: 0, cap, "depth planes")
        for part in chunks if n else []:
            rframes = [dict(cam=tuple(image_cams[m]), instances=[(int(obj[p]), 1, est[p].reshape(3, 4)) for p in rows]) for m, rows in part]
            lo, hi = min(m for m, _ in part), max(m for m, _ in part) + 1      # the chunk's images: only their label maps go through the histogram
            jobs = np.asarray([(m - lo, f * imax + k, int(lab[p]), 0) for f, (m, rows) in enumerate(part) for k, p in enumerate(rows)], np.int32)
            where = np.asarray([p for _, rows in part for p in rows], np.int64)
            with on_device:
                c = self.buffers(rframes, len(jobs), imax, H, W, 0, host)
                self.render(c)
                got = self.count(c, labels[lo:hi], field[lo:hi], hi - lo, ld, dir_off, kp, kp2d[where], jobs, cos_min, split)
                counts[where] = got if host else got.cpu().numpy()
            self.last_chunks += 1
            self.last_renders += len(where)
        return dict(counts=counts, **score_from_counts(counts))


# ---- the PnP poses of a batch ---------------------------------------------------------------------------------------------------------------
def _verify_found(verifier, flat, found, obj, label, labels, field, keypoints3d, camera_matrix, dir_off, kw):
    """the estimates flat[found] (found: rows of indices, the first the image) -> (scores, counts) of flat's leading shape"""
    lead = flat.shape[:-2]
    scores, counts = np.zeros(lead, np.float64), np.zeros(lead + (len(COUNT_NAMES),), np.int32)
    if len(found):
        cams = _np(camera_matrix, np.float64).reshape(-1, 3, 3)
        K = cams[found[:, 0]] if len(cams) == lead[0] else cams[0]
        at = tuple(found.T)
        got = verifier.verify(flat[at].astype(np.float64), K, obj, found[:, 0], labels, label, field, keypoints3d, dir_off, **kw)
        scores[at], counts[at] = got["score"], got["counts"]
    verifier.last_scores, verifier.last_counts = scores, counts
    return scores


def _object_keypoints(keypoints3d, oc: int) -> np.ndarray:
    """keypoints3d [oc, kp, 3], or a batch's [b, oc, 1, kp, 3] (every image holds the same) -> float64 [oc, kp, 3]"""
    k = _np(keypoints3d, np.float64)
    k = k.reshape((-1, oc) + k.shape[-2:])[0] if k.ndim > 3 else k
    if k.shape[0] != oc or k.shape[-1] != 3:
        raise ValueError("keypoints3d holds [kp, 3] per object for %d objects (got %s)" % (oc, np.shape(keypoints3d)))
    return k


def verify_estimates(verifier: "DevicePoseVerifier", poses, labels, field, keypoints3d, camera_matrix, dir_off: int = 0, **kw) -> np.ndarray:
    """The PnP poses of a batch, scored.  poses [b, oc, 1, 3, 4] or [b, oc, 3, 4] (the zero pose = not found: score 0); labels: the voter's
    `last_labels`, uint8 [b, h, w] on the device, in which object o has the value o + 1; field: the direction channels float32 [b, h, w, ld]
    beside it; keypoints3d [oc, kp, 3] or the batch's [b, oc, 1, kp, 3]; camera_matrix [b, 3, 3] or [3, 3].  -> scores float64 [b, oc];
    `verifier.last_scores` and `verifier.last_counts` [b, oc, 8] keep the call's results."""
    given = np.asarray(poses)
    b, oc = given.shape[:2]
    flat = given.reshape(b, oc, 3, 4)
    found = np.argwhere(np.abs(flat).sum(axis=(2, 3)) > 0)
    return _verify_found(verifier, flat, found, found[:, 1], found[:, 1] + 1, labels, field, _object_keypoints(keypoints3d, oc), camera_matrix, dir_off, kw)


def verify_instance_estimates(verifier: "DevicePoseVerifier", poses, slot_map, field, keypoints3d, camera_matrix, dir_off: int = 0, **kw) -> np.ndarray:
    """verify_estimates for the instance path: poses [b, oc, R, 3, 4] and the voter's slot map, in which instance r of object o has the value
    o * R + r + 1 (cp_ccl_instance_labels).  -> scores float64 [b, oc, R]"""
    given = np.asarray(poses)
    if given.ndim != 5 or given.shape[3:] != (3, 4):
        raise ValueError("poses is [b, oc, R, 3, 4] (got %s)" % (given.shape,))
    b, oc, R = given.shape[:3]
    found = np.argwhere(np.abs(given).sum(axis=(3, 4)) > 0)
    return _verify_found(verifier, given, found, found[:, 1], found[:, 1] * R + found[:, 2] + 1, slot_map, field, _object_keypoints(keypoints3d, oc),
                         camera_matrix, dir_off, kw)


# ---- the inference scripts under CASAPOSE_POSE_SCORE=1 ---------------------------------------------------------------------------------------
def verifier_for_meshes(verts, counts, path_meshes: str, objects: Sequence[str], device) -> "DevicePoseVerifier":
    """A verifier over the objects of an inference script (mask_refine.gather_meshes says what it takes)."""
    vs, faces, reach = gather_meshes(verts, counts, path_meshes, objects, what=WHAT)
    return DevicePoseVerifier(vs, faces, device, near=1e-2 * reach, far=1e4 * reach)          # the depth range in the meshes' own unit


def verifier_for_dataset(dataset, path_meshes: str, objects: Sequence[str], device) -> "DevicePoseVerifier":
    """verifier_for_meshes over a VectorfieldDataset's evaluation vertices"""
    if not hasattr(dataset, "generate_object_vertex_array"):
        raise ValueError("%s needs the objects' mesh files under --datameshes (got %r)" % (WHAT, path_meshes))
    verts, counts = dataset.generate_object_vertex_array()
    return verifier_for_meshes(verts, counts, path_meshes, objects, device)


_verifiers: Dict[tuple, "DevicePoseVerifier"] = {}


def verifier_from_environment(opt, evaluation_points, object_points_3d_count, device) -> Optional["DevicePoseVerifier"]:
    """What training.test_step asks (test_casapose.py): None unless CASAPOSE_POSE_SCORE=1; then the one verifier kept for the script's meshes --
    `opt.datameshes`, `opt.object` and the evaluation vertices the script hands to every step."""
    if not pose_score_enabled():
        return None
    objects = [x.strip() for x in str(getattr(opt, "object", "")).split(",") if x.strip()]
    key = (str(getattr(opt, "datameshes", "")), tuple(objects), str(device))
    if key not in _verifiers:
        _verifiers[key] = verifier_for_meshes(evaluation_points, object_points_3d_count, getattr(opt, "datameshes", ""), objects, device)
    return _verifiers[key]


__all__ = ["COUNT_NAMES", "DEFAULT_COS_MIN", "DevicePoseVerifier", "ENV_INSTANCE_SCORE", "instance_score_from_environment", "pose_score_enabled", "project_keypoints", "require_image_frame", "score_from_counts", 
           "verify_estimates", "verify_instance_estimates", "verifier_for_meshes", "verifier_for_dataset", "verifier_from_environment"]
