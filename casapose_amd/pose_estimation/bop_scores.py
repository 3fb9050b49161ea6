"""BOP scores of a result file: MSSD and MSPD with the objects' symmetries, and the recall-based AR_MSSD and AR_MSPD.

    e_MSSD = min over S of max over x of |P^ x - P_ S x|                     (millimetres)
    e_MSPD = min over S of max over x of |proj_K(P^ x) - proj_K(P_ S x)|     (pixels)

for an estimated pose P^, a ground-truth pose P_, the vertices x of the evaluation mesh and the symmetry transforms S of the object
(`symmetry_transforms`, from the `symmetries_discrete` / `symmetries_continuous` entries of models_info.json).  The errors are computed on the
GPU (`DeviceBopScorer`, cp_bop_errors_f32, csrc/bop_errors.hip) for every (estimate, ground-truth instance) pair of a test set in one call;
targets, matching and recall are small and run on the host in NumPy.  There is no host fall-back for the errors: a failing call raises
`CasaposeHipError`.

An estimate is correct for MSSD at theta when e_MSSD < theta * diameter, theta in 0.05 .. 0.50, and for MSPD at theta when e_MSPD < theta * r,
theta in 5 .. 50 and r = image_width / 640.  Recall at theta is matched targets / all targets; AR_MSSD and AR_MSPD are the means of recall over
their ten thresholds.  The mean of the two terms is reported as AR_MSSD_MSPD.  VSD, the third term of BOP's AR, needs the sensor's depth images and
a renderer: `score(..., vsd=...)` hands the same pairs to pose_estimation/bop_vsd.py and then also reports AR_VSD and AR = (AR_VSD + AR_MSSD +
AR_MSPD) / 3; without it no value is called AR.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .device_evaluation import PAIR_FLOATS
from .pose_evaluation import _np

MSSD_THRESHOLDS = tuple(0.05 * i for i in range(1, 11))    # times the object's diameter
MSPD_THRESHOLDS = tuple(5.0 * i for i in range(1, 11))     # pixels, times image_width / 640
MIN_VISIB_FRACT = 0.1
MAX_BLOCKS = (1 << 24) - 1      # cp_bop_errors_f32: pairs * symmetry groups per call


# ---- symmetry transforms ----------------------------------------------------------------------------------------------------------------
def _axis_rotation(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, np.float64).reshape(3)
    n = np.linalg.norm(a)
    if not n > 0:
        raise ValueError("symmetries_continuous: the axis %s has no direction" % (list(axis),))
    x, y, z = a / n
    c, s = math.cos(angle), math.sin(angle)
    C = 1.0 - c
    return np.array([[c + x * x * C, x * y * C - z * s, x * z * C + y * s],
                     [y * x * C + z * s, c + y * y * C, y * z * C - x * s],
                     [z * x * C - y * s, z * y * C + x * s, c + z * z * C]], np.float64)


def symmetry_transforms(info_entry: dict, max_sym_disc_step: float = 0.01) -> np.ndarray:
    """float64 [S, 3, 4]: the symmetry set of one models_info entry, the identity first.  D = identity, then every `symmetries_discrete` entry (16
    numbers, a row-major 4x4 of which R and t are taken).  Every `symmetries_continuous` entry {axis, offset} gives n = ceil(pi /
    max_sym_disc_step) rotations R_k by 2 pi k / n about the normalised axis with t_k = offset - R_k offset, k = 0 included.  Without continuous
    entries S = D; with them S = {(R_c R_d, R_c t_d + t_c)}, d-major."""
    D = [np.hstack([np.eye(3), np.zeros((3, 1))])]
    for m in info_entry.get("symmetries_discrete", []) or []:
        m = np.asarray(m, np.float64).reshape(4, 4)
        D.append(m[:3, :4].copy())
    C = []
    n = int(math.ceil(math.pi / max_sym_disc_step))
    for sym in info_entry.get("symmetries_continuous", []) or []:
        offset = np.asarray(sym.get("offset", [0.0, 0.0, 0.0]), np.float64).reshape(3)
        for k in range(n):
            R = np.eye(3) if k == 0 else _axis_rotation(sym["axis"], 2.0 * math.pi * k / n)
            C.append(np.hstack([R, (offset - R @ offset).reshape(3, 1)]))
    if not C:
        return np.stack(D)
    out = np.empty((len(D) * len(C), 3, 4), np.float64)
    for i, d in enumerate(D):
        for j, c in enumerate(C):
            out[i * len(C) + j, :, :3] = c[:, :3] @ d[:, :3]
            out[i * len(C) + j, :, 3] = c[:, :3] @ d[:, 3] + c[:, 3]
    return out


# ---- errors on the device ---------------------------------------------------------------------------------------------------------------
class DeviceBopScorer:
    """evaluation_points [objects, V, 3] with counts [objects] (as DevicePoseEvaluator takes them) and symmetries = one [S_o, 3, 4] array per
    object (`symmetry_transforms`) are uploaded once."""

    def __init__(self, evaluation_points, counts, symmetries: Sequence, device):
        import torch

        from .. import _lib

        self._lib_module = _lib
        self._lib = _lib.load()
        self.device = torch.device(device)
        pts = _np(evaluation_points, np.float32)
        if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or pts.shape[1] < 1:
            raise ValueError("evaluation_points must be [objects, V, 3] (got %s)" % (pts.shape,))
        self.objects, self.vmax = int(pts.shape[0]), int(pts.shape[1])
        cnt = _np(counts, np.int64).reshape(self.objects, -1)[:, 0]
        if cnt.min() < 1 or cnt.max() > self.vmax:
            raise ValueError("counts must lie in [1, %d] (got %s)" % (self.vmax, cnt.tolist()))
        if len(symmetries) != self.objects:
            raise ValueError("symmetries has %d entries for %d objects" % (len(symmetries), self.objects))
        syms = [_np(s, np.float64).reshape(-1, 3, 4) for s in symmetries]
        if min(len(s) for s in syms) < 1:
            raise ValueError("every object needs at least one symmetry transform (the identity)")
        self.smax = max(len(s) for s in syms)
        packed = np.zeros((self.objects, self.smax, 12), np.float32)
        for o, s in enumerate(syms):
            packed[o, :len(s)] = s.reshape(-1, 12)
        self.counts_host = cnt.astype(np.int32)
        self.sym_counts_host = np.array([len(s) for s in syms], np.int32)
        self.groups = -(-self.smax // int(self._lib.cp_bop_errors_sym_group()))
        self.max_pairs = max(1, MAX_BLOCKS // self.groups)           # per call; errors() chunks above it
        self.points = torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)
        self.counts = torch.from_numpy(self.counts_host).to(self.device)
        self.syms = torch.from_numpy(packed).to(self.device)
        self.sym_counts = torch.from_numpy(self.sym_counts_host).to(self.device)
        self.last_per_symmetry: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self._reserved = 0

    def _reserve(self, n: int) -> None:
        import torch

        if n <= self._reserved:
            return
        self._pairs = torch.empty((n, PAIR_FLOATS), dtype=torch.float32, device=self.device)
        self._index = torch.empty((n,), dtype=torch.int32, device=self.device)
        self._errors = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        self._workspace = torch.empty(self._lib.cp_bop_errors_workspace_bytes(n, self.smax) // 8, dtype=torch.float64, device=self.device)
        self._reserved = n

    def launch(self, n: int, per_symmetry=None) -> None:
        """The two kernels on the current stream over the first n records of the device `pairs` and `index` buffers."""
        import torch

        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._lib_module.check(self._lib.cp_bop_errors_f32(self.points.data_ptr(), self.counts.data_ptr(), self.objects, self.vmax, self.syms.data_ptr(),
                                                           self.sym_counts.data_ptr(), self.smax, self._pairs.data_ptr(), self._index.data_ptr(), n,
                                                           self._workspace.data_ptr(), self._errors.data_ptr(),
                                                           None if per_symmetry is None else per_symmetry.data_ptr(), stream), "cp_bop_errors_f32")

    def errors(self, est, gt, K, object_index, per_symmetry: bool = False):
        """-> (mssd [n], mspd [n]) float32.  est, gt [n, 3, 4] (or [n, 12]); K [n, 3, 3] or one [3, 3]; object_index [n] into the meshes.  A pair
        whose estimate is the zero pose gives +inf.  per_symmetry=True (tests) also fills `last_per_symmetry` = (mssd, mspd) [n, smax], +inf at
        and beyond an object's symmetry count."""
        import torch

        rec, idx = pack_bop_pairs(est, gt, K, object_index, self.objects)
        n = len(idx)
        out = np.empty((n, 2), np.float32)
        per = np.empty((n, self.smax, 2), np.float32) if per_symmetry else None
        if n == 0:
            self.last_per_symmetry = None if per is None else (per[..., 0], per[..., 1])
            return out[:, 0], out[:, 1]
        chunk = min(n, self.max_pairs)
        self._reserve(chunk)
        with torch.cuda.device(self.device):
            per_dev = torch.empty((chunk, self.smax, 2), dtype=torch.float32, device=self.device) if per_symmetry else None
            for lo in range(0, n, chunk):
                m = min(chunk, n - lo)
                self._pairs[:m].copy_(torch.from_numpy(rec[lo:lo + m]))
                self._index[:m].copy_(torch.from_numpy(idx[lo:lo + m]))
                self.launch(m, per_dev)
                out[lo:lo + m] = self._errors[:m].cpu().numpy()
                if per is not None:
                    per[lo:lo + m] = per_dev[:m].cpu().numpy()
        self.last_per_symmetry = None if per is None else (per[..., 0], per[..., 1])
        return out[:, 0].copy(), out[:, 1].copy()


def pack_bop_pairs(est, gt, K, object_index, objects: int):
    """-> (float32 [n, 36], int32 [n]): estimated pose (12, row-major 3x4), ground-truth pose (12), K (9), three pads -- the record of
    cp_pose_eval_f32 -- and the object of each pair."""
    idx = np.ascontiguousarray(_np(object_index, np.int64).reshape(-1))
    n = len(idx)
    if n and (idx.min() < 0 or idx.max() >= objects):
        raise ValueError("object_index must lie in [0, %d)" % objects)
    rec = np.zeros((n, PAIR_FLOATS), np.float32)
    rec[:, 0:12] = _np(est, np.float32).reshape(n, 12)
    rec[:, 12:24] = _np(gt, np.float32).reshape(n, 12)
    cams = _np(K, np.float32)
    rec[:, 24:33] = cams.reshape(n, 9) if cams.ndim == 3 else cams.reshape(1, 9)
    return rec, idx.astype(np.int32)


# ---- the result file --------------------------------------------------------------------------------------------------------------------
def read_bop_results(path: str) -> Dict[str, np.ndarray]:
    """The CSV `io_utils.write_poses` writes, with BOP's columns scene_id, im_id, obj_id, score, R (9 numbers), t (3), time ->
    {"scene_id", "im_id", "obj_id" int64 [n]; "score", "time" float64 [n]; "pose" float64 [n, 3, 4]}, rows in file order."""
    cols = {"scene_id": [], "im_id": [], "obj_id": [], "score": [], "time": [], "pose": []}
    with open(path) as f:
        for no, line in enumerate(f):
            line = line.strip()
            if not line or (no == 0 and line.startswith("scene_id")):
                continue
            part = [p.strip() for p in line.split(",")]
            if len(part) != 7:
                raise ValueError("%s, line %d: expected 7 comma-separated fields, found %d" % (path, no + 1, len(part)))
            R, t = [float(x) for x in part[4].split()], [float(x) for x in part[5].split()]
            if len(R) != 9 or len(t) != 3:
                raise ValueError("%s, line %d: R has %d numbers and t has %d (expected 9 and 3)" % (path, no + 1, len(R), len(t)))
            for key, value in zip(("scene_id", "im_id", "obj_id"), part[:3]):
                cols[key].append(int(value))
            cols["score"].append(float(part[3]))
            cols["time"].append(float(part[6]))
            cols["pose"].append(np.hstack([np.array(R).reshape(3, 3), np.array(t).reshape(3, 1)]))
    n = len(cols["score"])
    out = {k: np.asarray(cols[k], np.int64) for k in ("scene_id", "im_id", "obj_id")}
    out["score"], out["time"] = np.asarray(cols["score"], np.float64), np.asarray(cols["time"], np.float64)
    out["pose"] = np.asarray(cols["pose"], np.float64).reshape(n, 3, 4)
    return out


# ---- targets, matching, recall ----------------------------------------------------------------------------------------------------------
def select_targets(gts: Dict[Tuple[int, int], List[dict]], targets: Optional[Iterable[dict]] = None) -> Dict[Tuple[int, int, int], Tuple[int, List[int]]]:
    """{(scene_id, im_id, obj_id): (inst_count, candidates)}: how many instances are to be found there, and the indices, into that image's
    ground-truth list, of the instances an estimate may be matched to.  gts: {(scene_id, im_id): [{"id", "R", "t", and "visib_fract" where
    scene_gt_info.json exists}]}, as load_json_info gives them per scene.
      with `targets` (BOP's test_targets: dicts of scene_id, im_id, obj_id, inst_count): its entries, matched against every instance of the object
      without, where the instances carry "visib_fract": the instances with visib_fract >= 0.1
      otherwise: every instance."""
    out: Dict[Tuple[int, int, int], Tuple[int, List[int]]] = {}
    if targets is not None:
        for t in targets:
            key = (int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"]))
            cand = [i for i, g in enumerate(gts.get(key[:2], [])) if int(g["id"]) == key[2]]
            count = int(t["inst_count"]) + (out[key][0] if key in out else 0)
            if count > 0:
                out[key] = (count, cand)
        return out
    for (scene, im), instances in gts.items():
        for i, g in enumerate(instances):
            if "visib_fract" in g and not float(g["visib_fract"]) >= MIN_VISIB_FRACT:
                continue
            key = (int(scene), int(im), int(g["id"]))
            count, cand = out.get(key, (0, []))
            out[key] = (count + 1, cand + [i])
    return out


def is_estimate(score, pose) -> np.ndarray:
    """A row with score 0 or an all-zero pose is "no estimate": what write_poses writes for a miss."""
    pose = _np(pose).reshape(-1, 12)
    return (_np(score).reshape(-1) != 0) & (np.abs(pose).sum(axis=1) != 0)


def greedy_matches(errors: np.ndarray, threshold: float) -> int:
    """errors [estimates, instances], the estimates in descending order of score: each in turn takes the still-unmatched instance with the
    smallest error, and only if that error is below the threshold -> the number of matches."""
    errors = np.asarray(errors, np.float64)
    if errors.size == 0:
        return 0
    free = np.ones(errors.shape[1], bool)
    matched = 0
    for row in errors:
        if not free.any():
            break
        cand = np.where(free, row, np.inf)
        j = int(np.argmin(cand))
        if cand[j] < threshold:
            free[j] = False
            matched += 1
    return matched


def match_and_recall(groups: Iterable[Tuple[int, int, np.ndarray, np.ndarray]], diameters: Dict[int, float], image_width: float = 640.0) -> dict:
    """groups: one (obj_id, inst_count, mssd [e, g], mspd [e, g]) per (scene, image, object) that holds targets: the errors of its kept estimates
    (rows, in descending order of score) against its candidate instances (columns); e or g may be 0.  -> a plain dict of Python numbers that
    io_utils.to_json writes: "targets", "recall_mssd", "recall_mspd" (ten each), "AR_MSSD", "AR_MSPD", "AR_MSSD_MSPD", the thresholds, and the
    same per object under "objects"."""
    r = float(image_width) / 640.0
    total: Dict[int, int] = {}
    hits: Dict[int, np.ndarray] = {}
    for obj, count, mssd, mspd in groups:
        obj = int(obj)
        total[obj] = total.get(obj, 0) + int(count)
        h = hits.setdefault(obj, np.zeros((2, 10), np.int64))
        for i in range(10):
            h[0, i] += greedy_matches(mssd, MSSD_THRESHOLDS[i] * float(diameters[obj]))
            h[1, i] += greedy_matches(mspd, MSPD_THRESHOLDS[i] * r)

    def entry(n, h):
        rec = [[float(x) / n if n else 0.0 for x in h[k]] for k in (0, 1)]
        ar = [sum(v) / 10.0 for v in rec]
        return {"targets": int(n), "AR_MSSD": ar[0], "AR_MSPD": ar[1], "AR_MSSD_MSPD": 0.5 * (ar[0] + ar[1]), "recall_mssd": rec[0], "recall_mspd": rec[1]}

    out = entry(sum(total.values()), sum(hits.values()) if hits else np.zeros((2, 10), np.int64))
    out["image_width"] = float(image_width)
    out["mssd_thresholds"], out["mspd_thresholds"] = list(MSSD_THRESHOLDS), [t * r for t in MSPD_THRESHOLDS]
    out["objects"] = {str(obj): entry(total[obj], hits[obj]) for obj in sorted(total)}
    return out


def score(results: Dict[str, np.ndarray], gts: Dict[Tuple[int, int], List[dict]], cameras: Dict[Tuple[int, int], np.ndarray], scorer,
          object_ids: Sequence[int], diameters: Dict[int, float], targets: Optional[Iterable[dict]] = None, image_width: float = 640.0,
          vsd=None) -> dict:
    """Scores of a result file (`read_bop_results`) against the ground truth.  gts and cameras are keyed by (scene_id, im_id): the instance
    lists and camera matrices load_json_info gives per scene.  scorer.errors(est, gt, K, object_index) is a DeviceBopScorer whose mesh o is
    object object_ids[o].  Per (scene, image, object) with targets: the estimates are sorted by score descending with ties in file order, rows
    that are "no estimate" dropped, the first inst_count kept, and every kept estimate is paired with every candidate instance; all pairs go to
    the device in one call.  vsd (a bop_vsd.BopVsd, or anything with its `errors` and `taus`): the same pairs in the same order, with their
    (scene_id, im_id) and diameters, also go to vsd.errors -> [pairs, ntau], and the result gains "AR_VSD", "recall_vsd" ([tau][theta]) and
    "AR", over all objects and per object; without it the result is what it was before VSD existed."""
    wanted = select_targets(gts, targets)
    index_of = {int(o): i for i, o in enumerate(object_ids)}
    rows: Dict[Tuple[int, int, int], List[int]] = {}
    real = is_estimate(results["score"], results["pose"])
    for i in range(len(results["score"])):
        key = (int(results["scene_id"][i]), int(results["im_id"][i]), int(results["obj_id"][i]))
        if real[i] and key in wanted:
            rows.setdefault(key, []).append(i)
    est, gt, cams, obj_index, shapes, image_keys = [], [], [], [], [], []
    for key, (count, cand) in wanted.items():
        if key[2] not in index_of:
            raise KeyError("object %d has targets but no evaluation mesh" % key[2])
        mine = rows.get(key, [])
        kept = sorted(mine, key=lambda i: -results["score"][i])[:count]      # sorted() is stable: ties stay in file order
        shapes.append((key, count, len(kept), len(cand)))
        for i in kept:
            for j in cand:
                g = gts[key[:2]][j]
                est.append(results["pose"][i])
                gt.append(np.hstack([np.asarray(g["R"], np.float64).reshape(3, 3), np.asarray(g["t"], np.float64).reshape(3, 1)]))
                cams.append(np.asarray(cameras[key[:2]], np.float64).reshape(3, 3))
                obj_index.append(index_of[key[2]])
                image_keys.append(key[:2])
    if est:
        mssd, mspd = scorer.errors(np.stack(est), np.stack(gt), np.stack(cams), np.asarray(obj_index))
    else:
        mssd = mspd = np.zeros(0, np.float32)
    groups, at = [], 0
    for key, count, e, g in shapes:
        groups.append((key[2], count, np.asarray(mssd[at:at + e * g], np.float64).reshape(e, g), np.asarray(mspd[at:at + e * g], np.float64).reshape(e, g)))
        at += e * g
    out = match_and_recall(groups, diameters, image_width)
    out["pairs"] = int(at)
    if vsd is not None:
        from .bop_vsd import add_vsd_scores, match_and_recall_vsd

        pair_diameters = [float(diameters[object_ids[o]]) for o in obj_index]
        e = np.asarray(vsd.errors(np.stack(est), np.stack(gt), np.stack(cams), np.asarray(obj_index), image_keys, pair_diameters) if est
                       else np.zeros((0, len(vsd.taus))), np.float64)
        vsd_groups, at = [], 0
        for key, count, ne, ng in shapes:
            vsd_groups.append((key[2], count, e[at:at + ne * ng].reshape(ne, ng, e.shape[1])))
            at += ne * ng
        add_vsd_scores(out, match_and_recall_vsd(vsd_groups), vsd.taus)
    return out


__all__ = ["MSSD_THRESHOLDS", "MSPD_THRESHOLDS", "symmetry_transforms", "DeviceBopScorer", "pack_bop_pairs", "read_bop_results", "select_targets",
           "is_estimate", "greedy_matches", "match_and_recall", "score"]
