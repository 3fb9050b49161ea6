"""Keypoint covariances from the voting distribution (PVNet's uncertainty), computed by cp_kp_cov_f32 / cp_kp_cov_seeded_f32
(csrc/ransac_vote.hip): per (image, object, keypoint) the inlier-count-weighted second moments of one round of RANSAC hypotheses about the
voted keypoint.  `DevicePnP.solve(..., cov=)` and `pnp.pnp(..., cov=)` weight their final LM by them.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from .. import _lib
from .._lib import check
from .ransac_voting import _device_generator_seed


def uncertainty_pnp_enabled() -> bool:
    """CASAPOSE_UNCERTAINTY_PNP=1; says `pnp: uncertainty-weighted` the first time it is."""
    on = os.environ.get("CASAPOSE_UNCERTAINTY_PNP", "0") == "1"
    if on and not uncertainty_pnp_enabled.said:
        uncertainty_pnp_enabled.said = True
        print("pnp: uncertainty-weighted")
    return on


uncertainty_pnp_enabled.said = False


def keypoint_covariance(labels: torch.Tensor, vertex: torch.Tensor, points_xy: torch.Tensor, hyp: int = 512, inlier_thresh: float = 0.99,
                        min_num: int = 5, max_num: int = 30000, draws: Optional[torch.Tensor] = None,
                        generator: Optional[torch.Generator] = None, return_weight_sum: bool = False):
    """labels: uint8 [b,h,w] (0 background, object o = o + 1), or a one-hot mask [b,h,w,oc] without a background channel; vertex [b,h,w,vn,2]
    or [b,h,w,vn*2] in (dy,dx); points_xy [b,oc,vn,2] in (x,y) pixels, the voted keypoints of either voter (the number of objects is read from
    it).  -> cov float32 [b,oc,vn,3] = (sxx, sxy, syy) in px^2, and with return_weight_sum the int32 [b,oc,vn] sums of the inlier counts.
    Device tensors in and out.  The seed is drawn as ransac_voting_layer_all_masks draws its own (a CPU generator by default; a device
    generator is consumed without a synchronisation); `draws` (int32 [b,oc,hyp,vn,2] in [0, 2^31)) replaces the pixel-pair draws."""
    if not (labels.is_cuda and vertex.is_cuda and points_xy.is_cuda):
        raise _lib.CasaposeHipError("keypoint_covariance needs CUDA (ROCm) tensors; there is no CPU fallback")
    lib = _lib.load()
    dev = labels.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    b, h, w = int(labels.shape[0]), int(labels.shape[1]), int(labels.shape[2])
    mean = points_xy.to(torch.float32).contiguous()
    if mean.dim() != 4 or mean.shape[0] != b or mean.shape[3] != 2:
        raise ValueError("points_xy must be [%d, oc, vn, 2] (got %s)" % (b, tuple(points_xy.shape)))
    oc, vn = int(mean.shape[1]), int(mean.shape[2])
    if labels.dim() == 4:
        if labels.shape[3] != oc:
            raise ValueError("the mask has %d channels for %d objects" % (labels.shape[3], oc))
        lab = torch.empty(b, h, w, dtype=torch.uint8, device=dev)
        counts = torch.empty(b, oc, dtype=torch.int32, device=dev)
        check(lib.cp_mask_to_labels_f32(labels.to(torch.float32).contiguous().data_ptr(), b, h, w, oc, lab.data_ptr(), counts.data_ptr(), stream),
              "cp_mask_to_labels_f32")
    elif labels.dim() == 3 and labels.dtype == torch.uint8:
        lab = labels.contiguous()
    else:
        raise ValueError("labels must be uint8 [b,h,w] or a one-hot mask [b,h,w,oc] (got %s %s)" % (labels.dtype, tuple(labels.shape)))
    vert = vertex.reshape(b, h, w, -1).to(torch.float32).contiguous()
    if vert.shape[3] != 2 * vn:
        raise ValueError("vertex has %d channels for %d keypoints: vote on the merged field" % (vert.shape[3], vn))
    ws = torch.empty(lib.cp_kp_cov_workspace_bytes(b, h, w, oc, vn, hyp), dtype=torch.uint8, device=dev)
    cov = torch.empty(b, oc, vn, 3, dtype=torch.float32, device=dev)
    wsum = torch.empty(b, oc, vn, dtype=torch.int32, device=dev)
    head = (lab.data_ptr(), vert.data_ptr(), vert.shape[3], 0, b, h, w, oc, vn, mean.data_ptr())
    tail = (int(hyp), float(inlier_thresh), int(min_num), int(max_num), ws.data_ptr(), cov.data_ptr(), wsum.data_ptr(), stream)
    if draws is None:
        if generator is not None and generator.device.type != "cpu":
            seed = _device_generator_seed(generator)
        else:
            seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64, generator=generator).item())   # CPU generator: no device synchronisation
        check(lib.cp_kp_cov_seeded_f32(*head, seed, *tail), "cp_kp_cov_seeded_f32")
    else:
        if tuple(draws.shape) != (b, oc, hyp, vn, 2) or draws.dtype != torch.int32 or not draws.is_cuda:
            raise ValueError("draws must be a device int32 tensor with shape [b,oc,hyp,vn,2]")
        draws = draws.contiguous()
        check(lib.cp_kp_cov_f32(*head, draws.data_ptr(), *tail), "cp_kp_cov_f32")
    return (cov, wsum) if return_weight_sum else cov
