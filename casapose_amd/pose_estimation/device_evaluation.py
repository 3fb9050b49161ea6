"""ADD / ADD-S / 2-D projection statistics on the device: the counterpart of evaluate_poses / map_estimates
(casapose/pose_estimation/ransac_voting.py:561-687), which the reference runs as TensorFlow ops.

`DevicePoseEvaluator` keeps the evaluation meshes on the GPU and runs `cp_pose_eval_f32` (csrc/pose_eval.hip) over every (image, object)
pair of a batch: one small upload (a packed 36-float record per pair), two kernels, one small download.  It returns what the host
`evaluate_poses` (pose_evaluation.py) returns, in fp32 arithmetic on direct coordinate differences with fp64 sums; ADD-S is a brute-force
nearest neighbour over LDS tiles instead of the host's cKDTree.  There is no host fall-back: a failing call raises `CasaposeHipError`.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .pose_evaluation import SYMMETRIC_VERTEX_COUNTS, _np

PAIR_FLOATS, RECORD_FLOATS = 36, 6   # cp_pose_eval_f32's packed input and output records


def pack_pairs(poses, poses_gt, camera_matrixes, diameters, valid_points_filter, out: Optional[np.ndarray] = None) -> np.ndarray:
    """-> float32 [b*oc, 36]: estimated pose (12, row-major 3x4), ground-truth pose of instance 0 (12), K (9), diameter of instance 0,
    valid flag, one pad.  poses [b,oc,3,4] (or anything that reshapes to it), poses_gt [b,oc,ic,3,4], camera_matrixes [b,3,3] or [3,3],
    diameters [b,oc,...], valid_points_filter [b,oc]."""
    G = _np(poses_gt, np.float32)
    b, oc = G.shape[0], G.shape[1]
    rec = np.empty((b * oc, PAIR_FLOATS), np.float32) if out is None else out
    r = rec.reshape(b, oc, PAIR_FLOATS)
    r[:, :, 0:12] = _np(poses, np.float32).reshape(b, oc, 12)
    r[:, :, 12:24] = G.reshape(b, oc, -1, 12)[:, :, 0]
    cams = _np(camera_matrixes, np.float32)
    r[:, :, 24:33] = cams.reshape(b, 1, 9) if cams.ndim == 3 else cams.reshape(1, 1, 9)
    r[:, :, 33] = _np(diameters, np.float32).reshape(b, oc, -1)[:, :, 0]
    r[:, :, 34] = _np(valid_points_filter, np.float32).reshape(b, oc)
    r[:, :, 35] = 0.0
    return rec


class DevicePoseEvaluator:
    """evaluation_points [oc, V, 3] and object_points_3d_count [oc] (or [oc,1]) are uploaded once.  symmetric: per-object flags selecting
    ADD-S; None derives them from the vertex counts (SYMMETRIC_VERTEX_COUNTS: the glue and eggbox meshes, ransac_voting.py:619)."""

    def __init__(self, evaluation_points, object_points_3d_count, device, symmetric: Optional[Sequence[int]] = None):
        if evaluation_points is None or object_points_3d_count is None:
            raise ValueError("DevicePoseEvaluator needs evaluation_points and object_points_3d_count (the 9-keypoint evaluation stays on the host)")
        self._lib = _lib.load()
        self.device = torch.device(device)
        pts = _np(evaluation_points, np.float32)
        if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or pts.shape[1] < 1:
            raise ValueError("evaluation_points must be [objects, V, 3] (got %s)" % (pts.shape,))
        self.objects, self.vmax = int(pts.shape[0]), int(pts.shape[1])
        cnt = _np(object_points_3d_count, np.int64).reshape(self.objects, -1)[:, 0]
        if cnt.min() < 0 or cnt.max() > self.vmax:
            raise ValueError("object_points_3d_count must lie in [0, %d] (got %s)" % (self.vmax, cnt.tolist()))
        if symmetric is None:
            symmetric = [int(c) in SYMMETRIC_VERTEX_COUNTS for c in cnt]
        sym = np.asarray(symmetric).reshape(-1).astype(np.int32)
        if sym.shape[0] != self.objects:
            raise ValueError("symmetric has %d entries for %d objects" % (sym.shape[0], self.objects))
        self.counts_host, self.symmetric_host = cnt.astype(np.int32), sym
        self.points = torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)
        self.counts = torch.from_numpy(self.counts_host).to(self.device)
        self.symmetric = torch.from_numpy(sym).to(self.device)
        self.last_records: Optional[np.ndarray] = None
        self.last_point_errors = None
        self._batch = 0

    def _reserve(self, b: int) -> None:
        if b <= self._batch:
            return
        n = b * self.objects
        self._pairs_host = torch.empty((n, PAIR_FLOATS), dtype=torch.float32).pin_memory()
        self._records_host = torch.empty((n, RECORD_FLOATS), dtype=torch.float32).pin_memory()
        self._pairs = torch.empty((n, PAIR_FLOATS), dtype=torch.float32, device=self.device)
        self._records = torch.empty((n, RECORD_FLOATS), dtype=torch.float32, device=self.device)
        ws = self._lib.cp_pose_eval_workspace_bytes(b, self.objects, self.vmax)
        self._workspace = torch.empty(ws // 8, dtype=torch.float64, device=self.device)
        self._batch = b

    def launch(self, b: int, allowed_error_2d: float, point_err2: Optional[torch.Tensor] = None, point_err3: Optional[torch.Tensor] = None) -> None:
        """The two kernels on the current stream over the first b * objects records of the device `pairs` buffer."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.cp_pose_eval_f32(self.points.data_ptr(), self.counts.data_ptr(), self.symmetric.data_ptr(), self.objects, self.vmax,
                                              self._pairs.data_ptr(), b, float(allowed_error_2d), self._workspace.data_ptr(), self._records.data_ptr(),
                                              None if point_err2 is None else point_err2.data_ptr(),
                                              None if point_err3 is None else point_err3.data_ptr(), stream), "cp_pose_eval_f32")

    def evaluate(self, poses, poses_gt, camera_matrixes, diameters, valid_points_filter, allowed_error_2d: float = 5.0, point_errors: bool = False):
        """-> (err_2d, err_3d, valid_2d, valid_3d, missing_object, valid_points_count, false_positive_detection), each [oc], summed over the
        batch like evaluate_poses; the per-pair records stay in `last_records` [b, oc, 6].  Instance 0 only, like the reference and the host
        path.  point_errors=True (tests) also fills `last_point_errors` = (2-D, 3-D) [b, oc, V] per-point distances."""
        G = _np(poses_gt, np.float32)
        b, oc = G.shape[0], G.shape[1]
        if oc != self.objects:
            raise ValueError("poses_gt has %d objects, the evaluator holds %d meshes" % (oc, self.objects))
        self._reserve(b)
        n = b * oc
        pack_pairs(poses, G, camera_matrixes, diameters, valid_points_filter, out=self._pairs_host.numpy()[:n])
        with torch.cuda.device(self.device):
            self._pairs[:n].copy_(self._pairs_host[:n], non_blocking=True)
            e2 = e3 = None
            if point_errors:
                e2 = torch.empty((n, self.vmax), dtype=torch.float32, device=self.device)
                e3 = torch.empty((n, self.vmax), dtype=torch.float32, device=self.device)
            self.launch(b, allowed_error_2d, e2, e3)
            self._records_host[:n].copy_(self._records[:n], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        out = self._records_host[:n].numpy().reshape(b, oc, RECORD_FLOATS).copy()
        self.last_records = out
        self.last_point_errors = None if e2 is None else (e2.cpu().numpy().reshape(b, oc, -1), e3.cpu().numpy().reshape(b, oc, -1))
        s = out.sum(axis=0)
        valid_count = _np(valid_points_filter).reshape(b, oc).sum(axis=0).astype(np.float32)
        return s[:, 0], s[:, 1], s[:, 3], s[:, 2], s[:, 4], valid_count, s[:, 5]


_from_environment = None   # (evaluation_points, object_points_3d_count, device, evaluator) of the last evaluator_from_environment call


def evaluator_from_environment(evaluation_points, object_points_3d_count, device) -> Optional[DevicePoseEvaluator]:
    """CASAPOSE_DEVICE_EVAL=1 (and evaluation meshes given): the evaluator for these meshes, built on the first call and kept while the
    caller passes the same arrays -- test_casapose.py hands training.test_step the same mesh array every step.  Anything else: None, the
    host path.  Says `pose evaluation: device` when it builds one."""
    global _from_environment
    if os.environ.get("CASAPOSE_DEVICE_EVAL", "0") != "1" or evaluation_points is None or object_points_3d_count is None:
        return None
    device = torch.device(device)
    c = _from_environment
    if c is None or c[0] is not evaluation_points or c[1] is not object_points_3d_count or c[2] != device:
        _from_environment = (evaluation_points, object_points_3d_count, device, DevicePoseEvaluator(evaluation_points, object_points_3d_count, device))
        print("pose evaluation: device")
    return _from_environment[3]
