"""PnP on the device: voted keypoints -> [3,4] poses for every (image, object) pair of a batch in one launch (`cp_pnp_f64`, csrc/pnp.hip).

The counterpart of the host path `pnp.pnp` (ransac_voting.pnp :13-57 of the reference: RANSAC-EPnP, then iterative refinement over all points).
`DevicePnP` replaces the random sampling by a fixed table of 5-point hypotheses, all of them when there are at most 256, and takes the consensus by
a total order, so a call is reproducible bit for bit.  Its final pose is the Levenberg-Marquardt optimum of the same all-point reprojection error
as the host's: the same optimum, not the same bits.  `solve_host` runs the same code on the CPU (`cp_pnp_host_f64`).  There is
no host fall-back: a failing call raises `CasaposeHipError`.
"""
from __future__ import annotations

import itertools
import os
from typing import Optional

import numpy as np
import torch

from .. import _lib, twin
from .pose_evaluation import _np

MIN_POINTS, MAX_POINTS, SET_POINTS, MAX_HYPOTHESES = 5, 16, 5, 256
STATUS_OK, STATUS_SKIPPED, STATUS_NONFINITE_INPUT, STATUS_DEGENERATE, STATUS_NO_SOLUTION = range(5)


def hypothesis_table(n_points: int) -> np.ndarray:
    """uint8 [H, 5]: every 5-subset of n points in lexicographic order when there are at most 256 of them (n <= 10), otherwise 256 distinct
    subsets drawn with np.random.default_rng(0), sorted."""
    n = int(n_points)
    if n < MIN_POINTS:
        raise ValueError("the device PnP needs at least %d keypoints (got %d); fewer stay with the host path (pnp.pnp)" % (MIN_POINTS, n))
    if n > MAX_POINTS:
        raise ValueError("the device PnP takes at most %d keypoints (got %d); more stay with the host path (pnp.pnp)" % (MAX_POINTS, n))
    rows = list(itertools.combinations(range(n), SET_POINTS))
    if len(rows) > MAX_HYPOTHESES:
        keep = np.sort(np.random.default_rng(0).choice(len(rows), MAX_HYPOTHESES, replace=False))
        rows = [rows[i] for i in keep]
    return np.asarray(rows, np.uint8).reshape(-1, SET_POINTS)


def affine_from_offsets(offsets) -> np.ndarray:
    """float64 [b, 6]: transform_points_back (pose_evaluation.py) as x' = a0 x + a1 y + a2, y' = a3 x + a4 y + a5."""
    o = _np(offsets).reshape(-1, 10)
    hc, wc, dx, dy, ang, sc, sx, sy = o[:, 0], o[:, 1], o[:, 4], o[:, 5], o[:, 6], o[:, 7], o[:, 8], o[:, 9]
    ar = -ang * (np.pi / 180.0)
    a, b = np.cos(ar), np.sin(ar)
    c = (1.0 - a) * (sx / 2.0) - b * (sy / 2.0)
    d = b * (sx / 2.0) + (1.0 - a) * (sy / 2.0)
    tx, ty = wc - dx, hc - dy   # p = xy / sc + (tx, ty)
    return np.stack([a / sc, b / sc, a * tx + b * ty + c, -b / sc, a / sc, -b * tx + a * ty + d], axis=1)


class DevicePnP:
    """device: a torch device, or None for a solver that only offers solve_host (no GPU needed)."""

    def __init__(self, device, n_points: int, reprojection_error: float = 12.0):
        self.table_host = hypothesis_table(n_points)
        self._lib = _lib.load()
        self.n_points, self.hypotheses = int(n_points), int(self.table_host.shape[0])
        self.reprojection_error = float(reprojection_error)
        self.device = None if device is None else torch.device(device)
        self.table = None if self.device is None else torch.from_numpy(self.table_host).to(self.device)
        self.last_info: Optional[np.ndarray] = None
        self.last_cost: Optional[np.ndarray] = None
        self.last_poses = None
        self.last_weighted: Optional[np.ndarray] = None   # int32 [b,oc] of the last call with cov: 1 where the LM was weighted; None without cov

    def _shapes(self, points_xy, points_3d, K, solve_mask, affine):
        if points_xy.ndim != 4 or points_xy.shape[2] != self.n_points or points_xy.shape[3] != 2:
            raise ValueError("points_xy must be [b, oc, %d, 2] (got %s)" % (self.n_points, tuple(points_xy.shape)))
        b, oc = int(points_xy.shape[0]), int(points_xy.shape[1])
        if tuple(points_3d.shape) != (b, oc, self.n_points, 3):
            raise ValueError("points_3d must be [%d, %d, %d, 3] (got %s)" % (b, oc, self.n_points, tuple(points_3d.shape)))
        if tuple(K.shape) not in ((3, 3), (b, 3, 3)):
            raise ValueError("K must be [3, 3] or [%d, 3, 3] (got %s)" % (b, tuple(K.shape)))
        if tuple(solve_mask.shape) != (b, oc):
            raise ValueError("solve_mask must be [%d, %d] (got %s)" % (b, oc, tuple(solve_mask.shape)))
        if affine is not None and tuple(affine.shape) != (b, 6):
            raise ValueError("affine must be [%d, 6] (got %s)" % (b, tuple(affine.shape)))
        return b, oc

    def _call(self, xy, x3, K, mask, affine, poses, info, cost, host: bool, cov=None, cov_floor: float = 0.0, weighted=None) -> None:
        """cp_pnp_f64 on the current stream, or with cov cp_pnp_weighted_f64; host: their twins.  One argument list per entry point."""
        b, oc = int(xy.shape[0]), int(xy.shape[1])
        head = (xy, x3, K, int(K.ndim == 3), affine, mask, self.table_host if host else self.table, b, oc, self.n_points, self.hypotheses,
                self.reprojection_error)
        stream = None if host else torch.cuda.current_stream(self.device).cuda_stream
        if cov is None:
            twin.call("cp_pnp_f64", *head, poses, info, cost, host=host, stream=stream)
        else:
            twin.call("cp_pnp_weighted_f64", *head, cov, float(cov_floor), poses, info, cost, weighted, host=host, stream=stream)

    def launch(self, xy, x3, K, mask, affine, poses, info, cost) -> None:
        """cp_pnp_f64 on the current stream over contiguous device tensors of the right types."""
        self._call(xy, x3, K, mask, affine, poses, info, cost, host=False)

    def _solve(self, points_xy, points_3d, K, solve_mask, affine, host: bool, cov=None, cov_floor: float = 1.0 / 12.0) -> dict:
        """the inputs converted and the outputs made where the call runs (this device, or NumPy arrays for the twin) -> poses, info, cost and,
        with cov, weighted"""
        dev = None if host else self.device
        xy, x3, Kc = (twin.array(a, np.float32, dev) for a in (points_xy, points_3d, K))
        mask = twin.array(solve_mask, np.int32, dev)
        aff = None if affine is None else twin.array(affine, np.float64, dev)
        b, oc = self._shapes(xy, x3, Kc, mask, aff)
        spec = dict(poses=((b, oc, 3, 4), np.float32), info=((b, oc, 4), np.int32), cost=((b, oc, 2), np.float32))
        if cov is None:
            out = twin.alloc(spec, dev)
            self._call(xy, x3, Kc, mask, aff, out["poses"], out["info"], out["cost"], host)
            return out
        cv = twin.array(cov, np.float32, dev)   # a device tensor stays where it is
        if tuple(cv.shape) != (b, oc, self.n_points, 3):
            raise ValueError("cov must be [%d, %d, %d, 3] (got %s)" % (b, oc, self.n_points, tuple(cv.shape)))
        out = twin.alloc(dict(spec, weighted=((b, oc), np.int32)), dev)
        self._call(xy, x3, Kc, mask, aff, out["poses"], out["info"], out["cost"], host, cv, cov_floor, out["weighted"])
        return out

    def solve(self, points_xy, points_3d, K, solve_mask, affine=None, cov=None, cov_floor: float = 1.0 / 12.0):
        """points_xy [b,oc,n,2] (x,y), points_3d [b,oc,n,3], K [3,3] or [b,3,3], solve_mask [b,oc] (0: the zero pose), affine None or [b,6]
        (affine_from_offsets): device tensors, or host arrays that are uploaded.  -> poses, a device tensor [b,oc,3,4].  `last_info` int32
        [b,oc,4] (status, winning hypothesis, inlier count, LM iterations) and `last_cost` float32 [b,oc,2] are downloaded with it.
        cov: keypoint covariances [b,oc,n,3] = (sxx, sxy, syy) in the pixels of points_xy (keypoint_covariance's output, used where it lies);
        the final LM then minimises the Mahalanobis error (cp_pnp_weighted_f64) and `last_weighted` int32 [b,oc] says where.  cov_floor is
        added to sxx and syy first: by default 1/12 px^2, the variance of a position known only to one pixel of the field's grid.  cov=None is
        the unweighted call."""
        if self.device is None:
            raise _lib.CasaposeHipError("this DevicePnP was built without a device: only solve_host is available")
        with torch.cuda.device(self.device):
            out = self._solve(points_xy, points_3d, K, solve_mask, affine, host=False, cov=cov, cov_floor=cov_floor)
            self.last_info, self.last_cost = out["info"].cpu().numpy(), out["cost"].cpu().numpy()   # the copies synchronise
            self.last_weighted = out["weighted"].cpu().numpy() if cov is not None else None
        self.last_poses = out["poses"]
        return self.last_poses

    def solve_host(self, points_xy, points_3d, K, solve_mask, affine=None, cov=None, cov_floor: float = 1.0 / 12.0) -> np.ndarray:
        """The host twin of solve() on NumPy arrays: the same code, serially, without a GPU.  -> poses float32 [b,oc,3,4]."""
        out = self._solve(points_xy, points_3d, K, solve_mask, affine, host=True, cov=cov, cov_floor=cov_floor)
        self.last_info, self.last_cost, self.last_poses = out["info"], out["cost"], out["poses"]
        self.last_weighted = out.get("weighted")
        return self.last_poses


class HostTwinPnP(DevicePnP):
    """A solver whose solve() is the host twin: the callers' rules (pose_evaluation.py) can be exercised without a GPU."""

    def __init__(self, n_points: int, reprojection_error: float = 12.0):
        super().__init__(None, n_points, reprojection_error)

    def solve(self, points_xy, points_3d, K, solve_mask, affine=None, cov=None, cov_floor: float = 1.0 / 12.0):
        return torch.from_numpy(self.solve_host(points_xy, points_3d, K, solve_mask, affine, cov=cov, cov_floor=cov_floor))


_from_environment = None   # (n_points, device, solver) of the last solver_from_environment call


def solver_from_environment(n_points: int, device) -> Optional[DevicePnP]:
    """CASAPOSE_DEVICE_PNP=1: the solver for n_points keypoints on `device`, built on the first call and kept while both stay the same.  Anything
    else: None, the host path.  Says `pnp: device` when it builds one."""
    global _from_environment
    if os.environ.get("CASAPOSE_DEVICE_PNP", "0") != "1":
        return None
    device = torch.device(device)
    c = _from_environment
    if c is None or c[0] != int(n_points) or c[1] != device:
        _from_environment = (int(n_points), device, DevicePnP(device, n_points))
        print("pnp: device")
    return _from_environment[2]
