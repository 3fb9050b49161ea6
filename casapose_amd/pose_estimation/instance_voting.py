"""Several instances of one object per image (opt-in, CASAPOSE_MAX_INSTANCES=R): the least-squares voter of voting_layers_2d.py:43-122 keyed by
(object, instance) instead of by object, and a PnP over that axis.

CASAPose's vector field is shared by all classes and the label map tells the voter which pixel votes for what, so the network is used as it is:
cp_ccl_instance_labels turns the arg-max map into a slot map (the R largest components of each object as separate slots; the rule stands in
include/casapose_hip.h), cp_ls_vote_slots_f32 votes one keypoint set per slot, and poses_pnp_instances solves every (image, object, instance)
triple.  Instance r (0-based) of object o (1-based) has the slot id (o-1)*R + r + 1.

Components cannot separate instances that touch.  With split="votes" (CASAPOSE_INSTANCE_SPLIT=votes) cp_vote_split_labels builds the slot map
instead: the pixels vote for their own instance's centre (keypoint 0) and every pixel goes to the peak its direction points at; the voter and
the PnP are the same.

The split gives a few pixels beside a contact to the neighbouring instance, and the least-squares voter counts them in full.  With
voter="robust" (CASAPOSE_INSTANCE_VOTER=robust) cp_ls_vote_slots_robust_f32 votes instead: after the plain vote, `passes` further passes weight
every term by Tukey's biweight (cut-off `cutoff` pixels) of the distance of the current estimate from the pixel's line.

Neither voter says how far a keypoint can be trusted, and an instance beside another one is occluded or truncated: some of its keypoints lie
far outside its pixels.  With covariance=True (CASAPOSE_INSTANCE_PNP=weighted) cp_ls_slot_covariance_f32 makes one more pass over the slot map
for the voter's own keypoints and gives a 2 x 2 covariance per (slot, keypoint); poses_pnp_instances(cov=) weights the PnP by it."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib, ops
from . import pnp as _pnp
from .pose_evaluation import _np, _solved_poses
from .voting_layers_2d import _as_record

ENV = "CASAPOSE_MAX_INSTANCES"
MAX_INSTANCES = 16     # cp_ccl_instance_labels' bound on R
MAX_SLOTS = 254        # slot ids are bytes
ENV_SPLIT = "CASAPOSE_INSTANCE_SPLIT"
SPLITS = ("components", "votes")
ENV_VOTER = "CASAPOSE_INSTANCE_VOTER"
VOTERS = ("ls", "robust")
ROBUST_CUTOFF, ROBUST_PASSES = 4.0, 2     # the defaults of voter="robust": pixels, reweighted passes
ENV_PNP = "CASAPOSE_INSTANCE_PNP"


def max_instances_from_environment() -> Optional[int]:
    """CASAPOSE_MAX_INSTANCES: unset or 1 -> None (one instance per object, the existing path); an integer in 2..16 -> that many instances per
    object; anything else is an error."""
    raw = os.environ.get(ENV)
    if raw is None or raw.strip() == "1":
        return None
    try:
        r = int(raw.strip())
    except ValueError:
        r = None
    if r is None or not 2 <= r <= MAX_INSTANCES:
        raise ValueError("%s must be unset, 1 (one instance per object) or an integer in 2..%d (got %r)" % (ENV, MAX_INSTANCES, raw))
    return r


def instance_split_from_environment() -> str:
    """CASAPOSE_INSTANCE_SPLIT: unset or `components` -> "components" (cp_ccl_instance_labels, the existing rule); `votes` -> "votes"
    (cp_vote_split_labels), which needs CASAPOSE_MAX_INSTANCES; anything else is an error."""
    raw = os.environ.get(ENV_SPLIT)
    if raw is None or raw.strip() == "components":
        return "components"
    if raw.strip() != "votes":
        raise ValueError("%s must be unset, `components` or `votes` (got %r)" % (ENV_SPLIT, raw))
    if max_instances_from_environment() is None:
        raise ValueError("%s=votes needs %s set to an integer in 2..%d: without it one instance per object is voted" % (ENV_SPLIT, ENV, MAX_INSTANCES))
    return "votes"


def instance_voter_from_environment() -> str:
    """CASAPOSE_INSTANCE_VOTER: unset or `ls` -> "ls" (cp_ls_vote_slots_f32, the existing voter); `robust` -> "robust"
    (cp_ls_vote_slots_robust_f32), which needs CASAPOSE_MAX_INSTANCES; anything else is an error."""
    raw = os.environ.get(ENV_VOTER)
    if raw is None or raw.strip() == "ls":
        return "ls"
    if raw.strip() != "robust":
        raise ValueError("%s must be unset, `ls` or `robust` (got %r)" % (ENV_VOTER, raw))
    if max_instances_from_environment() is None:
        raise ValueError("%s=robust needs %s set to an integer in 2..%d: without it one instance per object is voted" % (ENV_VOTER, ENV, MAX_INSTANCES))
    return "robust"


def instance_pnp_from_environment() -> str:
    """CASAPOSE_INSTANCE_PNP: unset or `plain` -> "plain" (the keypoints of a slot count alike, the existing path); `weighted` -> "weighted"
    (a covariance per slot and keypoint from cp_ls_slot_covariance_f32 weights the PnP), which needs CASAPOSE_MAX_INSTANCES; anything else is
    an error."""
    raw = os.environ.get(ENV_PNP)
    if raw is None or raw.strip() == "plain":
        return "plain"
    if raw.strip() != "weighted":
        raise ValueError("%s must be unset, `plain` or `weighted` (got %r)" % (ENV_PNP, raw))
    if max_instances_from_environment() is None:
        raise ValueError("%s=weighted needs %s set to an integer in 2..%d: without it one instance per object is voted" % (ENV_PNP, ENV, MAX_INSTANCES))
    return "weighted"


class InstanceLSVoting:
    """CoordLSVotingWeighted(filter_estimates=True) with up to `max_instances` instances per object: __call__([seg, dirs, conf]) returns the
    keypoints [b, oc, R, kp, 2] in (y, x).  After a call `last_counts` is int32 [b, oc, R] on the device (the pixels of each instance, in
    descending order per object, 0 for an empty slot) and `last_labels` the uint8 slot map [b, h, w] that voted.

    split="votes" builds the slot map with cp_vote_split_labels instead (touching instances are separated by their votes for the object's
    centre; cell, vote_stride, min_votes, rel_percent, nms_radius and gate are its parameters, min_component its min_size).  Then
    `last_instances` is its int32 table [b, oc, R, 4] = (pixels, votes, peak cy, peak cx), `last_counts` the table's first column (in the order of
    the peaks' votes) and `last_peaks` the peaks' positions, float32 [b, oc, R, 2] in (y, x).

    voter="robust" votes with cp_ls_vote_slots_robust_f32 (`cutoff` in pixels, `passes` reweighted passes in 0..8) over the same slot map.  Then
    `last_kept` is float32 [b, oc, R, kp] on the device: the share of the plain weight that the last pass kept, the trace of the reweighted
    system over the trace of the plain one (0 for an empty slot; with passes = 0 nothing was reweighted and it is 1 wherever there are pixels).  voter="ls" is the plain voter, call for call.

    covariance=True adds one call of cp_ls_slot_covariance_f32 after the vote, for the voter's own keypoints (cut-off: the voter's when
    voter="robust" and passes > 0, otherwise none).  Then `last_cov` is float32 [b, oc, R, kp, 3] = (sxx, sxy, syy) in (x, y) pixels on the
    device, three NaNs where a keypoint has no covariance (an empty slot among them), and `last_cov_stat` float32 [b, oc, R, kp, 2] =
    (sigma2 in px^2, the share of the weight kept).  covariance=False makes the calls the voter made before, with the arguments they had."""

    def __init__(self, name, num_classes, num_points=9, max_instances=4, sigmoid_weights=False, min_component=50, split="components", cell=4,
                 vote_stride=2, min_votes=12, rel_percent=25, nms_radius=2, gate=4.0, voter="ls", cutoff=ROBUST_CUTOFF, passes=ROBUST_PASSES, covariance=False):
        oc = int(num_classes) - 1
        if not 1 <= int(max_instances) <= MAX_INSTANCES or oc < 1 or oc * int(max_instances) > MAX_SLOTS:
            raise ValueError("InstanceLSVoting: max_instances must be in 1..%d and objects * max_instances at most %d (got %d objects, %d instances)"
                             % (MAX_INSTANCES, MAX_SLOTS, oc, int(max_instances)))
        self.name = name
        self.num_classes = int(num_classes)
        self.num_points = int(num_points)
        self.max_instances = int(max_instances)
        self.sigmoid_weights = bool(sigmoid_weights)
        self.min_component = int(min_component)   # voting_layers_2d.py:66 has 50
        self.last_counts: Optional[torch.Tensor] = None
        self.last_labels: Optional[torch.Tensor] = None
        self.last_instances: Optional[torch.Tensor] = None   # int32 [b, oc, R, 2]: (size, image-local root) as cp_ccl_instance_labels wrote them
        if split not in SPLITS:
            raise ValueError("InstanceLSVoting: split must be one of %s (got %r)" % (SPLITS, split))
        self.split = split
        self.split_params = dict(cell=int(cell), vote_stride=int(vote_stride), min_votes=int(min_votes), rel_percent=int(rel_percent),
                                 nms_radius=int(nms_radius), gate=float(gate))
        self.last_peaks: Optional[torch.Tensor] = None       # split="votes": float32 [b, oc, R, 2]
        if voter not in VOTERS:
            raise ValueError("InstanceLSVoting: voter must be one of %s (got %r)" % (VOTERS, voter))
        if not (float(cutoff) > 0.0 and float(cutoff) < float("inf")) or int(passes) != passes or not 0 <= int(passes) <= 8:
            raise ValueError("InstanceLSVoting: cutoff must be finite and > 0 and passes an integer in 0..8 (got %r, %r)" % (cutoff, passes))
        self.voter, self.cutoff, self.passes = voter, float(cutoff), int(passes)
        self.last_kept: Optional[torch.Tensor] = None        # voter="robust": float32 [b, oc, R, kp]
        self.covariance = bool(covariance)
        self.last_cov: Optional[torch.Tensor] = None         # covariance=True: float32 [b, oc, R, kp, 3]
        self.last_cov_stat: Optional[torch.Tensor] = None    # covariance=True: float32 [b, oc, R, kp, 2]

    def slot_of(self, o: int, r: int) -> int:
        """the slot id of instance r (0-based) of object o (1-based)"""
        if not (1 <= o < self.num_classes and 0 <= r < self.max_instances):
            raise ValueError("slot_of: object %d instance %d outside 1..%d / 0..%d" % (o, r, self.num_classes - 1, self.max_instances - 1))
        return (o - 1) * self.max_instances + r + 1

    def __call__(self, inp: Sequence[torch.Tensor], **kwargs) -> torch.Tensor:
        seg, direct, conf = inp
        if not seg.is_cuda:
            raise _lib.CasaposeHipError("InstanceLSVoting needs CUDA (ROCm) tensors; there is no CPU fallback")
        if seg.shape[3] != self.num_classes:
            raise ValueError("InstanceLSVoting: the segmentation has %d classes, the voter was built for %d" % (seg.shape[3], self.num_classes))
        rec, (so, do, co) = _as_record(seg, direct, conf)
        objects, R = self.num_classes - 1, self.max_instances
        b, h, w, _ = rec.shape
        from ..engine import cached_labels

        lab0 = None
        if so == 0 and rec.storage_offset() == 0:
            lab0 = cached_labels(rec.untyped_storage().data_ptr(), (b, h, w), seg._version)  # the forward's own arg-max map
        if lab0 is None:
            lab0 = ops.argmax_labels(rec, classes=objects + 1, offset=so)
        if self.split == "votes":
            slot_map, inst, self.last_peaks = ops.vote_split_labels(lab0, rec, do, objects, R, min_size=self.min_component, **self.split_params)
        else:
            slot_map, inst = ops.ccl_instance_labels(lab0, objects, R, self.min_component)
        if self.voter == "robust":
            out, plain, again = ops.ls_vote_slots_robust(rec, do, co, objects * R, self.num_points, slot_map, cutoff=self.cutoff, passes=self.passes,
                                                         sigmoid_weights=self.sigmoid_weights, return_sums=True)
            again = again if self.passes else plain                                                # no pass: block 1 is not written
            weight, kept = plain[..., 0] + plain[..., 2], again[..., 0] + again[..., 2]           # the two traces, on the device
            self.last_kept = torch.where(weight > 0, kept / weight, torch.zeros_like(weight)).to(torch.float32).view(b, objects, R, self.num_points)
        else:
            out = ops.ls_vote_slots(rec, do, co, objects * R, self.num_points, slot_map, sigmoid_weights=self.sigmoid_weights)
        if self.covariance:
            cutoff = self.cutoff if self.voter == "robust" and self.passes > 0 else None
            cov, stat = ops.ls_slot_covariance(rec, do, co, objects * R, self.num_points, slot_map, out, cutoff=cutoff, sigmoid_weights=self.sigmoid_weights)
            self.last_cov, self.last_cov_stat = cov.view(b, objects, R, self.num_points, 3), stat.view(b, objects, R, self.num_points, 2)
        self.last_labels, self.last_instances, self.last_counts = slot_map, inst, inst[..., 0]
        return out.view(b, objects, R, self.num_points, 2)


def poses_pnp_instances(coords, counts, object_points_3d, camera_data, min_num: int = 20, rng=None, solver=None, cov=None, return_weighted: bool = False):
    """Voted keypoints [b, oc, R, kp, 2] in (y, x) and pixel counts [b, oc, R] (InstanceLSVoting's result and last_counts) -> poses float32
    [b, oc, R, 3, 4].  A slot with count <= min_num gets the zero pose; a pose with t_z < 0 is negated (pose_evaluation._poses_pnp's rules).
    object_points_3d: the objects' 3-D keypoints, [b, oc, (1,) kp, 3] or [oc, kp, 3].  solver: a DevicePnP solves all (image, object, instance)
    triples in one call, as oc * R pseudo-objects that share their object's 3-D keypoints; None asks device_pnp.solver_from_environment
    (CASAPOSE_DEVICE_PNP=1, keypoints on a GPU), and without one the host loop over pnp.pnp_rvec_t runs.
    cov: keypoint covariances [b, oc, R, kp, 3] = (sxx, sxy, syy) in (x, y) pixels (InstanceLSVoting(covariance=True).last_cov) weight the final
    LM of whichever PnP runs, with the floor and the fall-back poses_pnp applies: 1/12 px^2 is added to sxx and syy, and a slot with a
    covariance that is not finite and positive definite is solved unweighted.  A device tensor goes to the solver where it lies.  With
    return_weighted the result is (poses, weighted), weighted an int array [b, oc, R]: 1 where the solve was weighted (all 0 without cov)."""
    if solver is None and hasattr(coords, "detach") and coords.is_cuda:
        from .device_pnp import solver_from_environment

        solver = solver_from_environment(int(coords.shape[3]), coords.device)
    pts = _np(coords)[..., ::-1]     # (y, x) -> (x, y)
    if pts.ndim != 5 or pts.shape[4] != 2:
        raise ValueError("poses_pnp_instances: coords must be [b, oc, R, kp, 2] (got %s)" % (tuple(pts.shape),))
    b, oc, R, kp, _ = pts.shape
    cnt = _np(counts, np.int64)
    if tuple(cnt.shape) != (b, oc, R):
        raise ValueError("poses_pnp_instances: counts must be [%d, %d, %d] (got %s)" % (b, oc, R, tuple(cnt.shape)))
    kp3 = _np(object_points_3d)
    lead = kp3.shape[0] if kp3.ndim >= 4 else 1
    if kp3.size % (lead * kp * 3) or kp3.size // (lead * kp * 3) < oc or lead not in (1, b):
        raise ValueError("poses_pnp_instances: object_points_3d %s does not hold %d keypoints for %d objects" % (tuple(kp3.shape), kp, oc))
    kp3 = np.broadcast_to(kp3.reshape(lead, -1, kp, 3)[:, :oc], (b, oc, kp, 3))
    cam = _np(camera_data)
    cam = cam[0] if cam.ndim == 3 else cam
    mask = cnt > int(min_num)
    if cov is not None and (tuple(cov.shape) != (b, oc, R, kp, 3)):
        raise ValueError("poses_pnp_instances: cov must be [%d, %d, %d, %d, 3] (got %s)" % (b, oc, R, kp, tuple(cov.shape)))
    if solver is not None:
        xy = np.ascontiguousarray(pts.reshape(b, oc * R, kp, 2))
        x3 = np.ascontiguousarray(np.repeat(kp3, R, axis=1))                     # pseudo-object o * R + r has object o's keypoints
        m = np.ascontiguousarray(mask.reshape(b, oc * R).astype(np.int32))
        if cov is not None:
            cov = cov.reshape(b, oc * R, kp, 3).contiguous() if hasattr(cov, "detach") else np.ascontiguousarray(_np(cov).reshape(b, oc * R, kp, 3))
        poses = _solved_poses(solver, xy, x3, cam, m, None, cov)
        bad = np.argwhere((m != 0) & np.isin(np.asarray(solver.last_info)[..., 0], (2, 4)))   # a degenerate keypoint set (3) is the zero pose
        if len(bad):
            raise FloatingPointError("poses_pnp_instances: non-finite pose for image %d object %d instance %d"
                                     % (bad[0][0], bad[0][1] // R, bad[0][1] % R))
        poses = poses.reshape(b, oc, R, 3, 4)
        if not return_weighted:
            return poses
        weighted = np.zeros((b, oc, R), np.int32) if cov is None else np.asarray(solver.last_weighted).reshape(b, oc, R).astype(np.int32)
        return poses, weighted
    out = np.zeros((b, oc, R, 3, 4), np.float32)
    weighted = np.zeros((b, oc, R), np.int32)
    cov = None if cov is None else _np(cov) + np.array([_pnp.COV_FLOOR, 0.0, _pnp.COV_FLOOR])
    for n, o, r in np.argwhere(mask):
        c = None if cov is None else cov[n, o, r]
        weighted[n, o, r] = int(c is not None and _pnp.whitening_factors(c, kp) is not None)
        p6 = _pnp.pnp_rvec_t(kp3[n, o], pts[n, o, r], cam, rng=rng, cov=c)
        if not np.all(np.isfinite(p6)):
            raise FloatingPointError("poses_pnp_instances: non-finite pose for image %d object %d instance %d" % (n, o, r))
        Rm, t = _pnp.rodrigues(p6[:3]), p6[3:].astype(np.float64)
        P = np.concatenate([Rm, t.reshape(3, 1)], axis=1)
        out[n, o, r] = -P if t[2] < 0 else P
    return (out, weighted) if return_weighted else out
