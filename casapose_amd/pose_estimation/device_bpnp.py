"""The BPnP keypoint loss on the device: voted keypoints -> loss, d loss / d keypoints and poses for every (image, object) pair of a batch in two
launches (`cp_bpnp_loss_f64`, csrc/bpnp.hip), without a host round trip and without random draws.

The counterpart of the host path `training.bpnp_reprojection_loss_host` (keypoint_reprojection_loss with use_bpnp_reprojection_loss=1,
loss_functions.py:264-323 of the reference): PnP, the reprojection / ground-truth loss at its optimum, and the gradient through that optimum by the
implicit function theorem.  `DeviceBPnPLoss` takes the consensus over `device_pnp.hypothesis_table` instead of RANSAC draws, so a call is
reproducible bit for bit; its optimum is the host path's, not its bits.  `loss_and_grad_host` runs the same code on the CPU
(`cp_bpnp_loss_host_f64`).  There is no host fall-back: a failing call raises `CasaposeHipError`.

One stated difference from the host path: an available pair whose solve fails or is degenerate (a collapsed vote, a non-finite keypoint) is
treated as unavailable -- no loss, no gradient, not in the mean -- and counted in `last_counts[1]`; the host path raises FloatingPointError for
the whole step.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib, twin
from .device_pnp import MAX_POINTS, MIN_POINTS, hypothesis_table
from .pose_evaluation import _np


class DeviceBPnPLoss:
    """device: a torch device, or None for an object that only offers loss_and_grad_host (no GPU needed)."""

    def __init__(self, device, n_points: int, reprojection_error: float = 12.0):
        n = int(n_points)
        if n < MIN_POINTS or n > MAX_POINTS:
            raise ValueError("the device BPnP loss takes %d to %d keypoints (got %d); other point counts stay with the host path "
                             "(training.bpnp_reprojection_loss_host)" % (MIN_POINTS, MAX_POINTS, n))
        self.table_host = hypothesis_table(n)
        self._lib = _lib.load()
        self.n_points, self.hypotheses = n, int(self.table_host.shape[0])
        self.reprojection_error = float(reprojection_error)
        self.device = None if device is None else torch.device(device)
        self.table = None if self.device is None else torch.from_numpy(self.table_host).to(self.device)
        self.points_3d = self.cam = None       # bind(): the targets TrainPlan.kp_loss_and_grad reads
        self._buffers = {}                     # (b, oc) -> run()'s poses, info, counts, workspace
        self._info = self._counts = None       # of the last call: device tensors (launch) or arrays (host twin)

    # ---- what the last call left, downloaded when asked for (the copy synchronises; nothing else here does) ----
    @property
    def last_info(self) -> Optional[np.ndarray]:
        """int32 [b,oc,4]: status, winning hypothesis, its inlier count, iterations of the first LM (cp_pnp_f64's words)"""
        return None if self._info is None else _np(self._info, np.int32)

    @property
    def last_counts(self) -> Optional[np.ndarray]:
        """int32 [2]: solved pairs, available pairs that were not solved"""
        return None if self._counts is None else _np(self._counts, np.int32)

    def workspace_bytes(self, b: int, oc: int) -> int:
        return int(self._lib.cp_bpnp_loss_workspace_bytes(int(b), int(oc), self.n_points))

    def _shapes(self, coords_yx, gt_xy, affine, avail, points_3d, cam) -> Tuple[int, int]:
        if coords_yx.ndim != 4 or coords_yx.shape[2] != self.n_points or coords_yx.shape[3] != 2:
            raise ValueError("coords_yx must be [b, oc, %d, 2] (got %s)" % (self.n_points, tuple(coords_yx.shape)))
        b, oc = int(coords_yx.shape[0]), int(coords_yx.shape[1])
        for name, a, want in (("gt_xy", gt_xy, b * oc * self.n_points * 2), ("affine", affine, b * 6), ("avail", avail, b * oc),
                              ("points_3d", points_3d, b * oc * self.n_points * 3), ("cam", cam, 9)):
            if int(np.prod(a.shape)) != want:
                raise ValueError("%s must hold %d values for b = %d, oc = %d, kp = %d (got %s)" % (name, want, b, oc, self.n_points, tuple(a.shape)))
        return b, oc

    def _outputs(self, b: int, oc: int, device, zero: bool = False) -> dict:
        """poses, info, counts and the workspace of one call, where it runs (a device, or None for NumPy arrays)"""
        return twin.alloc(dict(poses=((b, oc, 1, 3, 4), np.float32), info=((b, oc, 4), np.int32), counts=((2,), np.int32),
                               workspace=((self.workspace_bytes(b, oc) // 8,), np.float64)), device, zero)

    def bind(self, points_3d, cam) -> "DeviceBPnPLoss":
        """Upload the model keypoints [b,oc,kp,3] and the one camera matrix [3,3] that run() uses."""
        cam = _np(cam, np.float32)
        self.points_3d = twin.array(_np(points_3d, np.float32).reshape(-1, self.n_points, 3), np.float32, self.device)
        self.cam = twin.array(cam[0] if cam.ndim == 3 else cam, np.float32, self.device)
        return self

    def _call(self, coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error, weight, g_yx, loss, out: dict, host: bool) -> None:
        """cp_bpnp_loss_f64 on the current stream, or its host twin: the one argument list of both"""
        b, oc = int(coords_yx.shape[0]), int(coords_yx.shape[1])
        twin.call("cp_bpnp_loss_f64", coords_yx, gt_xy, affine, avail, points_3d, cam, self.table_host if host else self.table, b, oc, self.n_points,
                  self.hypotheses, self.reprojection_error, float(max_pixel_error), float(weight), g_yx, loss, out["poses"], out["info"], out["counts"],
                  out["workspace"], host=host, stream=None if host else torch.cuda.current_stream(self.device).cuda_stream)
        self._info, self._counts = out["info"], out["counts"]

    def launch(self, coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error: float, weight: float, g_yx, loss, poses, info, counts, workspace) -> None:
        """cp_bpnp_loss_f64 on the current stream over contiguous device tensors of the right types (fp32; loss fp64 [1]; info, counts int32;
        workspace of workspace_bytes(b, oc)).  It does not synchronise."""
        self._call(coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error, weight, g_yx, loss,
                   dict(poses=poses, info=info, counts=counts, workspace=workspace), host=False)

    def run(self, coords_yx, gt_xy, affine, avail, max_pixel_error: float, weight: float, g_yx, loss):
        """launch() with the bound targets into the caller's gradient [b,oc,kp,2] and fp64 loss [1]; -> (poses, info, counts), device tensors
        this object keeps and overwrites with its next call of the same batch shape."""
        if self.device is None:
            raise _lib.CasaposeHipError("this DeviceBPnPLoss was built without a device: only loss_and_grad_host is available")
        if self.points_3d is None:
            raise _lib.CasaposeHipError("DeviceBPnPLoss.run needs bind(points_3d, cam) first")
        b, oc = self._shapes(coords_yx, gt_xy, affine, avail, self.points_3d, self.cam)
        if (b, oc) not in self._buffers:
            self._buffers[(b, oc)] = self._outputs(b, oc, self.device, zero=True)
        out = self._buffers[(b, oc)]
        self._call(coords_yx, gt_xy, affine, avail, self.points_3d, self.cam, max_pixel_error, weight, g_yx, loss, out, host=False)
        return out["poses"], out["info"], out["counts"]

    def _loss_and_grad(self, coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error, weight, host: bool):
        """the inputs converted and the outputs made where the call runs -> (loss [1], g_yx, poses)"""
        dev = None if host else self.device
        cam = cam if hasattr(cam, "detach") else _np(cam, np.float32)
        c, gt, aff, av, x3, K = (twin.array(a, np.float32, dev) for a in (coords_yx, gt_xy, affine, avail, points_3d, cam[0] if cam.ndim == 3 else cam))
        b, oc = self._shapes(c, gt, aff, av, x3, K)
        out = self._outputs(b, oc, dev)
        res = twin.alloc(dict(g=((b, oc, self.n_points, 2), np.float32), loss=((1,), np.float64)), dev)
        self._call(c, gt, aff, av, x3, K, max_pixel_error, weight, res["g"], res["loss"], out, host)
        return res["loss"], res["g"], out["poses"]

    def loss_and_grad(self, coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error: float = 25.0, weight: float = 1.0):
        """coords_yx [b,oc,kp,2] (y,x) crop pixels, gt_xy [b,oc,kp,2] (x,y) image pixels, affine [b,6] or [b,2,3], avail [b,oc], points_3d
        [b,oc,kp,3], cam [3,3]: device tensors, or host arrays that are uploaded.  -> (loss fp64 scalar, g_yx = weight * d loss / d coords_yx
        float32 [b,oc,kp,2], poses float32 [b,oc,1,3,4]) as device tensors; nothing is downloaded."""
        if self.device is None:
            raise _lib.CasaposeHipError("this DeviceBPnPLoss was built without a device: only loss_and_grad_host is available")
        with torch.cuda.device(self.device):
            loss, g, poses = self._loss_and_grad(coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error, weight, host=False)
        return loss[0], g, poses

    def loss_and_grad_host(self, coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error: float = 25.0, weight: float = 1.0):
        """The host twin of loss_and_grad() on NumPy arrays: the same code, serially, without a GPU.  -> (loss float, g_yx float32 [b,oc,kp,2],
        poses float32 [b,oc,1,3,4])."""
        loss, g, poses = self._loss_and_grad(coords_yx, gt_xy, affine, avail, points_3d, cam, max_pixel_error, weight, host=True)
        return float(loss[0]), g, poses
