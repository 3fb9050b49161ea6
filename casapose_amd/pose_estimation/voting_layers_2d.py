"""CoordLSVotingWeighted with the reference's constructor / call convention
(casapose/pose_estimation/voting_layers_2d.py:5-122), computed by cp_ls_vote_f32
(+ cp_ccl_filter_labels when filter_estimates=True).
"""
from __future__ import annotations

import os
import warnings
import weakref
from typing import Optional, Sequence

import torch

from .. import _lib, ops
from .._lib import check
from .keypoint_covariance import uncertainty_pnp_enabled
from .refine_common import mask_refine_enabled


def _as_record(seg: torch.Tensor, direct: torch.Tensor, conf: torch.Tensor):
    """If the three inputs are channel slices of ONE [B,H,W,ld] tensor (the usual
    `tf.split(output_net, ...)` of train_casapose.py:539) use it in place; otherwise pack them."""
    ts = (seg, direct, conf)
    b, h, w = seg.shape[:3]
    ld = seg.stride(2)
    want = (h * w * ld, w * ld, ld, 1)
    same_store = all(t.untyped_storage().data_ptr() == seg.untyped_storage().data_ptr() for t in ts)
    if same_store and all(t.dtype == torch.float32 and t.stride() == want for t in ts) and ld % 4 == 0 and 0 < ld <= 64:
        first = min(t.storage_offset() for t in ts)
        offs = [t.storage_offset() - first for t in ts]
        fits = first + b * h * w * ld <= seg.untyped_storage().nbytes() // 4
        if fits and all(o + t.shape[3] <= ld for o, t in zip(offs, ts)) and (seg.untyped_storage().data_ptr() + 4 * first) % 16 == 0:
            return torch.as_strided(seg, (b, h, w, ld), want, storage_offset=first), offs
    k, d, c = seg.shape[3], direct.shape[3], conf.shape[3]
    ld = (k + d + c + 3) // 4 * 4
    rec = torch.zeros(seg.shape[0], seg.shape[1], seg.shape[2], ld, dtype=torch.float32, device=seg.device)
    rec[..., :k] = seg
    rec[..., k:k + d] = direct
    rec[..., k + d:k + d + c] = conf
    return rec, [0, k, k + d]


class CoordLSVotingWeighted:
    def __init__(self, name, num_classes, num_points=9, sigmoid_weights=False, filter_estimates=False,
                 output_second_largest_component=False):
        self.name = name
        # voting_layers_2d.py:58-59,71-73 ("just for testing"): vote with the SECOND largest component of each object (three histogram bins,
        # the third entry of top_k) instead of the largest; only read with filter_estimates
        self.output_second_largest_component = bool(output_second_largest_component)
        self.num_classes = num_classes
        self.num_points = num_points
        self.filter_estimates = filter_estimates
        self.sigmoid_weights = bool(sigmoid_weights)   # w = sigmoid(sigmoid_scale * conf), sigmoid_scale = 1 (voting_layers_2d.py:20,32-33); default softplus
        self.min_component = 50  # voting_layers_2d.py:66
        self._voted = None   # the last call's filtered label map, or (record, objects, seg offset) of an unfiltered call
        self.last_field: Optional[torch.Tensor] = None   # with CASAPOSE_UNCERTAINTY_PNP=1: the last call's merged field [b,h,w,2*kp] (dy,dx), a view
        if os.environ.get("CASAPOSE_MAX_INSTANCES", "1").strip() != "1":   # this voter does not read the switch: say so instead of ignoring it in silence
            warnings.warn("CASAPOSE_MAX_INSTANCES is set, but CoordLSVotingWeighted finds one instance per object: several instances are voted by "
                          "instance_voting.InstanceLSVoting (util_scripts/minimal_instances.py)")

    @property
    def last_labels(self) -> Optional[torch.Tensor]:
        """uint8 [b,h,w]: the label map the last call voted with -- the filtered map with filter_estimates, the arg-max map otherwise.
        keypoint_covariance takes it over the pixels that voted.  With CASAPOSE_UNCERTAINTY_PNP=1 the arg-max map is made in the call
        itself; otherwise the voter takes the arg-max inside its kernel and the map is made when it is first asked for, from the
        segmentation the voter was given: ask before that tensor is overwritten."""
        if isinstance(self._voted, tuple):
            rec, objects, so = self._voted
            self._voted = ops.argmax_labels(rec, classes=objects + 1, offset=so)
        return self._voted

    def __call__(self, inp: Sequence[torch.Tensor], **kwargs) -> torch.Tensor:
        seg, direct, conf = inp
        if not seg.is_cuda:
            raise _lib.CasaposeHipError("CoordLSVotingWeighted needs CUDA (ROCm) tensors; there is no CPU fallback")
        rec, (so, do, co) = _as_record(seg, direct, conf)
        objects = seg.shape[3] - 1
        labels: Optional[torch.Tensor] = None
        if self.filter_estimates:
            lib = _lib.load()
            b, h, w, _ = rec.shape
            from ..engine import cached_labels

            lab0 = None
            if so == 0 and rec.storage_offset() == 0:
                lab0 = cached_labels(rec.untyped_storage().data_ptr(), (b, h, w), seg._version)  # the forward's own arg-max map
            if lab0 is None:
                lab0 = ops.argmax_labels(rec, classes=objects + 1, offset=so)
            ws = torch.empty(lib.cp_ccl_workspace_bytes(b, h, w, objects), dtype=torch.uint8, device=rec.device)
            labels = torch.empty_like(lab0)
            check(lib.cp_ccl_filter_labels(lab0.data_ptr(), b, h, w, objects, self.min_component, 2 if self.output_second_largest_component else 1, ws.data_ptr(),
                                           labels.data_ptr(), torch.cuda.current_stream(rec.device).cuda_stream),
                  "cp_ccl_filter_labels")
        self._voted = labels if labels is not None else (rec, objects, so)
        out = ops.ls_vote(rec, so, do, co, objects, self.num_points, labels=labels, sigmoid_weights=self.sigmoid_weights)
        uncertainty = uncertainty_pnp_enabled()
        if uncertainty or mask_refine_enabled():   # what a caller that only holds the keypoints (poses_pnp) needs: voter_of()
            global _last_vote
            self.last_labels   # (made now: the record may be the network's output buffer)
            if uncertainty:    # to vote the keypoints' covariance; the mask refinement (mask_refine.refine_voted_poses) needs the labels only
                self.last_field = rec[..., do:do + 2 * self.num_points]
            _last_vote = (weakref.ref(out), self)
        return out


_last_vote = None   # (weak reference to the keypoints the last vote under CASAPOSE_UNCERTAINTY_PNP=1 or CASAPOSE_MASK_REFINE=1 returned, its voter)


def voter_of(points) -> Optional[CoordLSVotingWeighted]:
    """The voter whose last call, made under CASAPOSE_UNCERTAINTY_PNP=1 or CASAPOSE_MASK_REFINE=1, returned this very tensor; None for any other
    object."""
    if _last_vote is not None and _last_vote[0]() is points:
        return _last_vote[1]
    return None
