"""Evaluation of several instances of one object per image: up to R estimated poses per (image, object) -- the slots of
instance_voting.poses_pnp_instances -- against up to I ground-truth instances, matched, with ADD / ADD-S / 2-D recall and precision.

evaluate_poses and DevicePoseEvaluator compare one estimate per (image, object) with ground-truth instance 0, as the reference's map_estimates
does (ransac_voting.py:561-625).  Here every (estimate e, instance g) pair gets the same two errors -- the mean 2-D reprojection distance and
the mean ADD, or ADD-S for a symmetric object -- and the pairs are matched greedily by the 3-D error: repeatedly the smallest finite cost among
the free non-empty estimates and the free instances, on ties the smaller g, then the smaller e.  This is BOP's and COCO's scheme; no distance
gates a match, a far match is simply no true positive.  Greedy is not the optimal assignment (csrc/match_math.h has the example); for a recall
thresholded at 0.1 diameters the two differ only where two instances lie within 0.2 diameters of each other.

`match_instances_host` is the fp64 NumPy statement of it and needs no GPU.  `DeviceInstanceEvaluator` keeps the evaluation meshes on the GPU
and runs cp_pose_match_f32 (csrc/pose_match.hip); there is no host fall-back: a failing call raises `CasaposeHipError`.  `summarise` turns the
tallies into recall and precision, `write_instance_evaluation` / `write_instance_matches` write them down, and `evaluate_instance_batch` is the
loop body of util_scripts/test_instances.py.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .pose_evaluation import SYMMETRIC_VERTEX_COUNTS, _adds_error, _np, project

UNMATCHED, EMPTY = -1, -2         # est_match: a non-empty estimate without an instance (a false positive); an empty slot
SUMMARY_COLUMNS = ("gt", "est", "matched", "recall_add", "recall_2d", "precision_add", "precision_2d", "mean_err_3d", "median_err_3d", "mean_err_2d",
                   "median_err_2d")


def greedy_match(cost: np.ndarray, live: Sequence[bool], count: int):
    """cost [R, I]; live [R]: the estimate is not empty; count: the instances g < count exist -> (est_match [R], gt_match [I], matched).
    All finite pairs in the order (cost, g, e); a pair is taken when both of its sides are still free."""
    R, I = cost.shape
    est_match = np.where(np.asarray(live, bool), UNMATCHED, EMPTY).astype(np.int32)
    gt_match = np.full(I, UNMATCHED, np.int32)
    pairs = sorted((float(cost[e, g]), g, e) for e in range(R) for g in range(min(int(count), I)) if live[e] and np.isfinite(cost[e, g]))
    matched = 0
    for _, g, e in pairs:
        if est_match[e] == UNMATCHED and gt_match[g] == UNMATCHED:
            est_match[e], gt_match[g] = g, e
            matched += 1
    return est_match, gt_match, matched


def _shapes(poses_est, poses_gt, instance_count, camera_matrixes, dtype):
    G = _np(poses_gt, dtype)
    if G.ndim < 3:
        raise ValueError("poses_gt must be [b, oc, I, 3, 4] (got %s)" % (G.shape,))
    b, oc, I = G.shape[0], G.shape[1], G.shape[2]
    G = G.reshape(b, oc, I, 12)
    E = _np(poses_est, dtype)
    if E.ndim < 3 or E.shape[0] != b or E.shape[1] != oc or E[0, 0, 0].size != 12:
        raise ValueError("poses_est must be [%d, %d, R, 3, 4] (got %s)" % (b, oc, E.shape))
    R = E.shape[2]
    E = E.reshape(b, oc, R, 12)
    cnt = _np(instance_count, np.int64)
    if cnt.size != b * oc:
        raise ValueError("instance_count must be [%d, %d] (got %s)" % (b, oc, cnt.shape))
    cnt = np.clip(cnt.reshape(b, oc), 0, I).astype(np.int32)
    cams = _np(camera_matrixes, dtype)
    cams = np.broadcast_to(cams.reshape(-1, 9) if cams.ndim == 3 else cams.reshape(1, 9), (b, 9))
    return E, G, cnt, np.ascontiguousarray(cams), (b, oc, R, I)


def object_diameters(diameters, oc: int, dtype=np.float64) -> np.ndarray:
    """[oc] from [oc], or from a batch's [b, oc, ...] (absent instances are padded with -1: the largest entry of an object is its diameter)"""
    d = _np(diameters, dtype)
    if d.size == oc:
        return d.reshape(oc)
    if d.ndim < 2 or d.shape[1] != oc:
        raise ValueError("diameters must be [%d] or [b, %d, ...] (got %s)" % (oc, oc, d.shape))
    return np.moveaxis(d, 1, 0).reshape(oc, -1).max(axis=1)


def symmetric_flags(counts: np.ndarray, symmetric) -> np.ndarray:
    """symmetric=None is DevicePoseEvaluator's rule: the vertex counts of the glue and eggbox meshes select ADD-S"""
    if symmetric is None:
        symmetric = [int(c) in SYMMETRIC_VERTEX_COUNTS for c in counts]
    sym = np.asarray(symmetric).reshape(-1).astype(np.int32)
    if sym.shape[0] != len(counts):
        raise ValueError("symmetric has %d entries for %d objects" % (sym.shape[0], len(counts)))
    return sym


def symmetric_from_models_info(folder: str, stems: Sequence[str], counts) -> np.ndarray:
    """The flags of a mesh folder: an object whose entry in <folder>/models_info.json has `symmetries_discrete` or `symmetries_continuous` gets
    ADD-S.  Without the file, or for an object without an entry, the vertex-count rule applies (symmetric_flags(counts, None))."""
    import json
    import os

    from ..data_handler.model_prep import _existing_entry

    flags = symmetric_flags(np.asarray(counts).reshape(-1), None)
    path = os.path.join(folder, "models_info.json")
    if os.path.isfile(path):
        with open(path) as f:
            info = json.load(f)
        for o, stem in enumerate(stems):
            entry = _existing_entry(info, stem)
            if entry:
                flags[o] = int(bool(entry.get("symmetries_discrete")) or bool(entry.get("symmetries_continuous")))
    return flags


def match_instances_host(poses_est, poses_gt, instance_count, evaluation_points, object_points_3d_count, camera_matrixes, diameters, symmetric=None,
                         allowed_error_2d: float = 5.0):
    """fp64 NumPy.  poses_est [b,oc,R,3,4], poses_gt [b,oc,I,3,4], instance_count [b,oc], evaluation_points [oc,V,3], object_points_3d_count [oc]
    (or [oc,1]), camera_matrixes [b,3,3] or [3,3], diameters [oc] (or a batch's [b,oc,I])  ->
      err float64 [b,oc,R,I,2]: (err_2d, err_3d), +inf for an empty estimate (|sum of the pose| < 1e-4) and for g >= count;
      gt_rec float64 [b,oc,I,5]: (matched slot or -1, err_2d, err_3d, valid_3d, valid_2d), (-1, 0, 0, 0, 0) without a match;
      est_match int32 [b,oc,R]: the matched g, -1 for a false positive, -2 for an empty slot;
      tally int32 [b,oc,5]: ground truth, estimates, matched, tp_3d, tp_2d."""
    E, G, cnt, cams, (b, oc, R, I) = _shapes(poses_est, poses_gt, instance_count, camera_matrixes, np.float64)
    pts = _np(evaluation_points)
    vcount = _np(object_points_3d_count, np.int64).reshape(oc, -1)[:, 0]
    sym = symmetric_flags(vcount, symmetric)
    diam = object_diameters(diameters, oc)
    err = np.full((b, oc, R, I, 2), np.inf)
    gt_rec = np.zeros((b, oc, I, 5))
    gt_rec[..., 0] = UNMATCHED
    est_match = np.zeros((b, oc, R), np.int32)
    tally = np.zeros((b, oc, 5), np.int32)
    for n in range(b):
        K = cams[n].reshape(3, 3)
        for o in range(oc):
            X = pts[o][:int(vcount[o])]
            live = [not (abs(E[n, o, e].sum()) < 1e-4) for e in range(R)]
            truth = [project(X, K, G[n, o, g].reshape(3, 4)) for g in range(cnt[n, o])]
            for e in range(R):
                if not live[e] or not truth:
                    continue
                p2, p3 = project(X, K, E[n, o, e].reshape(3, 4))
                for g, (t2, t3) in enumerate(truth):
                    with np.errstate(invalid="ignore"):
                        e2 = np.linalg.norm(t2 - p2, axis=1).mean() if len(X) else np.nan
                        e3 = (_adds_error(t3, p3) if sym[o] else np.linalg.norm(t3 - p3, axis=1)).mean() if len(X) else np.nan
                    err[n, o, e, g] = (e2, e3)
            est_match[n, o], gm, matched = greedy_match(err[n, o, :, :, 1], live, cnt[n, o])
            for g in range(I):
                if gm[g] >= 0:
                    e2, e3 = err[n, o, gm[g], g]
                    gt_rec[n, o, g] = (gm[g], e2, e3, float(e3 < diam[o] * 0.1), float(e2 < allowed_error_2d))
            tally[n, o] = (cnt[n, o], sum(live), matched, gt_rec[n, o, :, 3].sum(), gt_rec[n, o, :, 4].sum())
    return err, gt_rec, est_match, tally


class DeviceInstanceEvaluator:
    """evaluation_points [oc, V, 3] and object_points_3d_count [oc] (or [oc,1]) are uploaded once.  symmetric: per-object flags selecting ADD-S;
    None derives them from the vertex counts, as DevicePoseEvaluator does."""

    def __init__(self, evaluation_points, object_points_3d_count, device, symmetric: Optional[Sequence[int]] = None):
        if evaluation_points is None or object_points_3d_count is None:
            raise ValueError("DeviceInstanceEvaluator needs evaluation_points and object_points_3d_count")
        self._lib = _lib.load()
        self.device = torch.device(device)
        pts = _np(evaluation_points, np.float32)
        if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or pts.shape[1] < 1:
            raise ValueError("evaluation_points must be [objects, V, 3] (got %s)" % (pts.shape,))
        self.objects, self.vmax = int(pts.shape[0]), int(pts.shape[1])
        cnt = _np(object_points_3d_count, np.int64).reshape(self.objects, -1)[:, 0]
        if cnt.min() < 0 or cnt.max() > self.vmax:
            raise ValueError("object_points_3d_count must lie in [0, %d] (got %s)" % (self.vmax, cnt.tolist()))
        self.counts_host, self.symmetric_host = cnt.astype(np.int32), symmetric_flags(cnt, symmetric)
        self.points = torch.tensor(pts).to(self.device)       # a copy: the caller's array may be read-only
        self.counts = torch.from_numpy(self.counts_host).to(self.device)
        self.symmetric = torch.from_numpy(self.symmetric_host).to(self.device)
        self.last_err = self.last_gt_rec = self.last_est_match = self.last_tally = self.last_poses = None

    def launch(self, est: torch.Tensor, gt: torch.Tensor, gt_counts: torch.Tensor, cams: torch.Tensor, diameters: torch.Tensor, b: int, R: int, I: int,
               allowed_error_2d: float):
        """The two kernels on the current stream over device tensors: est float32 [b,oc,R,12], gt [b,oc,I,12], gt_counts int32 [b,oc], cams [b,9],
        diameters [oc] -> the four device outputs.  Sizes the library refuses raise CasaposeHipError before anything is launched."""
        oc = self.objects
        ws = self._lib.cp_pose_match_workspace_bytes(b, oc, self.vmax, R, I)
        workspace = torch.empty(max(ws // 8, 1), dtype=torch.float64, device=self.device)
        err = torch.empty((b, oc, R, I, 2), dtype=torch.float32, device=self.device)
        gt_rec = torch.empty((b, oc, I, 5), dtype=torch.float32, device=self.device)
        est_match = torch.empty((b, oc, R), dtype=torch.int32, device=self.device)
        tally = torch.empty((b, oc, 5), dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.cp_pose_match_f32(self.points.data_ptr(), self.counts.data_ptr(), self.symmetric.data_ptr(), oc, self.vmax, est.data_ptr(),
                                               R, gt.data_ptr(), I, gt_counts.data_ptr(), cams.data_ptr(), diameters.data_ptr(), b,
                                               float(allowed_error_2d), workspace.data_ptr(), err.data_ptr(), gt_rec.data_ptr(), est_match.data_ptr(),
                                               tally.data_ptr(), stream), "cp_pose_match_f32")
        return err, gt_rec, est_match, tally

    def match(self, poses_est, poses_gt, instance_count, camera_matrixes, diameters, allowed_error_2d: float = 5.0):
        """poses_est [b,oc,R,3,4], poses_gt [b,oc,I,3,4], instance_count [b,oc], camera_matrixes [b,3,3] or [3,3], diameters [oc] (or a batch's
        [b,oc,I]) -> (err float32 [b,oc,R,I,2], gt_rec float32 [b,oc,I,5], est_match int32 [b,oc,R], tally int32 [b,oc,5]) as
        match_instances_host describes them, NumPy arrays; they stay in last_err, last_gt_rec, last_est_match and last_tally."""
        E, G, cnt, cams, (b, oc, R, I) = _shapes(poses_est, poses_gt, instance_count, camera_matrixes, np.float32)
        if oc != self.objects:
            raise ValueError("poses_gt has %d objects, the evaluator holds %d meshes" % (oc, self.objects))
        diam = np.ascontiguousarray(object_diameters(diameters, oc, np.float32))
        with torch.cuda.device(self.device):
            up = [torch.tensor(a).to(self.device) for a in (E, G, cnt, cams, diam)]
            out = self.launch(*up, b, R, I, allowed_error_2d)
            host = [t.cpu().numpy() for t in out]
        self.last_err, self.last_gt_rec, self.last_est_match, self.last_tally = host
        return tuple(host)


def _ratio(a: float, b: float) -> float:
    return float(a) / float(b) if b else 0.0   # divide_no_nan, as test_casapose.py reports its recalls


def _row(tally: np.ndarray, rec: np.ndarray) -> dict:
    """tally [n, 5] and the gt records [m, 5] they count -> one row of the summary"""
    gt, est, matched, tp3, tp2 = (int(v) for v in tally.reshape(-1, 5).sum(axis=0))
    on = rec[:, 0] >= 0
    e2, e3 = rec[on, 1].astype(np.float64), rec[on, 2].astype(np.float64)
    stat = lambda f, v: float(f(v)) if len(v) else float("nan")  # noqa: E731
    return dict(gt=gt, est=est, matched=matched, tp_add=tp3, tp_2d=tp2, recall_add=_ratio(tp3, gt), recall_2d=_ratio(tp2, gt),
                precision_add=_ratio(tp3, est), precision_2d=_ratio(tp2, est), mean_err_3d=stat(np.mean, e3), median_err_3d=stat(np.median, e3),
                mean_err_2d=stat(np.mean, e2), median_err_2d=stat(np.median, e2))


def summarise(tallies, gt_rec) -> dict:
    """tallies int [..., oc, 5] and gt_rec [..., oc, I, 5] of one or more match calls (stacked or concatenated along the leading axes) ->
    {"objects": [one row per object], "all": the row over every object}.  A row: gt, est (non-empty estimates), matched, tp_add, tp_2d,
    recall = tp / gt, precision = tp / est (0 where the denominator is 0), and the mean and median err_3d / err_2d over the matched instances
    (NaN without any)."""
    t = np.asarray(tallies)
    r = np.asarray(gt_rec)
    oc, I = t.shape[-2], r.shape[-2]
    if t.shape[-1] != 5 or r.shape[-1] != 5 or r.shape[-3] != oc or t.size // (oc * 5) != r.size // (oc * I * 5):
        raise ValueError("summarise: tallies %s and gt_rec %s do not belong together" % (t.shape, r.shape))
    t, r = t.reshape(-1, oc, 5), r.reshape(-1, oc, I, 5)
    return dict(objects=[_row(t[:, o], r[:, o].reshape(-1, 5)) for o in range(oc)], all=_row(t, r.reshape(-1, 5)))


def write_instance_evaluation(path: str, names: Sequence[str], summary: dict) -> None:
    """one row per object and one `all` row: object, then SUMMARY_COLUMNS"""
    if len(names) != len(summary["objects"]):
        raise ValueError("write_instance_evaluation: %d names for %d objects" % (len(names), len(summary["objects"])))
    with open(path, "w") as f:
        f.write("object," + ",".join(SUMMARY_COLUMNS) + "\n")
        for name, row in list(zip(names, summary["objects"])) + [("all", summary["all"])]:
            f.write(str(name) + "," + ",".join("%d" % row[c] if isinstance(row[c], int) else "%.6g" % row[c] for c in SUMMARY_COLUMNS) + "\n")


def write_instance_matches(path: str, names: Sequence[str], tallies, gt_rec, images: Optional[Sequence[str]] = None) -> int:
    """one row per ground-truth instance (g < the group's count): image, object, instance, slot (-1: not found), err_2d, err_3d, valid_3d, valid_2d.
    tallies [n, oc, 5], gt_rec [n, oc, I, 5], images: n names (default: the index).  Returns the rows written."""
    t, r = np.asarray(tallies), np.asarray(gt_rec)
    oc, I = t.shape[-2], r.shape[-2]
    t, r = t.reshape(-1, oc, 5), r.reshape(-1, oc, I, 5)
    rows = 0
    with open(path, "w") as f:
        f.write("image,object,instance,slot,err_2d,err_3d,valid_3d,valid_2d\n")
        for n in range(t.shape[0]):
            for o in range(oc):
                for g in range(int(t[n, o, 0])):
                    v = r[n, o, g]
                    f.write("%s,%s,%d,%d,%.6g,%.6g,%d,%d\n" % (n if images is None else images[n], names[o], g, int(v[0]), v[1], v[2], int(v[3]), int(v[4])))
                    rows += 1
    return rows


def crop_cameras(camera_matrixes, offsets) -> np.ndarray:
    """float64 [b, 3, 3]: the camera of every image's crop.  A crop pixel p maps to the image pixel A p (transform_points_back, as
    device_pnp.affine_from_offsets states it), so the crop's camera is A^-1 K."""
    from .device_pnp import affine_from_offsets

    A = affine_from_offsets(offsets)
    b = A.shape[0]
    K = _np(camera_matrixes)
    K = np.broadcast_to(K.reshape(-1, 3, 3), (b, 3, 3))
    M = np.tile(np.eye(3), (b, 1, 1))
    M[:, :2, :] = A.reshape(b, 2, 3)
    return np.linalg.solve(M, K)


def evaluate_instance_batch(batch, out, voter, evaluator: DeviceInstanceEvaluator, keypoints, camera_matrix, min_num: int, rng=None, cov: bool = False):
    """The loop body util_scripts/test_instances.py and the tests share: the network output `out` [b,h,w,K + 2 kp + ...] -> InstanceLSVoting ->
    poses_pnp_instances -> evaluator.match against the batch's poses_gt / instance_count / diameters.  keypoints: the objects' 3-D keypoints
    [oc,kp,3]; camera_matrix: the one camera of the pixels the voter sees (the crop's).  cov: weight the PnP by the voter's covariances (a voter
    built with covariance=True).  -> the four arrays of match; the poses [b,oc,R,3,4] stay in evaluator.last_poses."""
    from .instance_voting import poses_pnp_instances

    K, kp = voter.num_classes, voter.num_points
    seg, dirs, conf = torch.split(out, [K, 2 * kp, out.shape[3] - K - 2 * kp], dim=3)
    coords = voter([seg, dirs, conf])
    counts = voter.last_counts.cpu().numpy()
    if cov and voter.last_cov is None:
        raise ValueError("evaluate_instance_batch: cov=True needs a voter built with covariance=True")
    poses = poses_pnp_instances(coords, counts, keypoints, camera_matrix, min_num=min_num, rng=rng, cov=voter.last_cov if cov else None)
    evaluator.last_poses = np.asarray(poses)
    return evaluator.match(poses, batch["poses_gt"], batch["instance_count"], camera_matrix, batch["diameters"])
