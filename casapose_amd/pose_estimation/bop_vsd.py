"""BOP's Visible Surface Discrepancy and the recall-based AR_VSD, the third term of BOP's AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3.

For an estimated pose P^ and a ground-truth pose P_ of an object in an image with the sensor's depth map D_t, both poses are rendered to
depth, depths are turned into distances from the camera centre, and

    vis_g = hit_g and (D_t missing or d_g - d_t <= delta)          vis_e = hit_e and (D_t missing or d_e - d_t <= delta or vis_g)
    e_VSD(tau) = (|{inter: |d_g - d_e| / diameter >= tau}| + |union| - |inter|) / |union|,   1 where the union is empty

with inter = vis_g and vis_e, union = vis_g or vis_e (BOP19: delta = 15 mm, tau = 0.05 .. 0.50 times the diameter, correct when e_VSD <
theta, theta = 0.05 .. 0.50).  The renders are the depth planes of the mask renderer (csrc/masks.hip, at BOP's sample offset 0.0); the
per-pixel rules and their sums run on the GPU (cp_vsd_counts_i32, csrc/vsd.hip, rules in csrc/vsd_math.h) and give integers per pair, from
which `vsd_errors` takes the error on the host.  There is no host fall-back: a failing call raises `CasaposeHipError`.

`near` and `far` bound the rendered depths.  Their defaults are this project's: they are not checked against the BOP toolkit's renderer."""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .bop_scores import greedy_matches, is_estimate, select_targets
from .pose_evaluation import _np

VSD_DELTA = 15.0                                           # millimetres
VSD_TAUS = tuple(0.05 * i for i in range(1, 11))           # times the object's diameter
VSD_THRESHOLDS = tuple(0.05 * i for i in range(1, 11))     # correct when e_VSD < theta
DEFAULT_NEAR, DEFAULT_FAR = 10.0, 10000.0                  # millimetres
DEFAULT_SPLIT = 8                                          # blocks per pair: the fastest of 1 .. 64 in tools/vsd_probe.py
MAX_TAUS = 32


def read_depth(path: str, depth_scale: float) -> np.ndarray:
    """BOP's depth image (a 16-bit PNG, or any single-channel integer image PIL reads) -> float32 [H, W] in millimetres: the raw value times
    the image's `depth_scale` of scene_camera.json, both as float32.  0 stays 0: "no measurement"."""
    from PIL import Image

    with Image.open(path) as im:
        raw = np.array(im)
    if raw.ndim != 2:
        raise ValueError("%s: a depth image has one channel (got shape %s)" % (path, raw.shape))
    return raw.astype(np.float32) * np.float32(depth_scale)


def vsd_errors(counts) -> np.ndarray:
    """counts int [n, 2 + ntau] (cp_vsd_counts_i32: union, intersection, one count per tau) -> float64 [n, ntau]:
    (count_k + union - intersection) / union, 1.0 where the union is empty."""
    c = np.asarray(counts).astype(np.int64)
    if c.ndim != 2 or c.shape[1] < 3:
        raise ValueError("counts must be [n, 2 + ntau] with ntau >= 1 (got %s)" % (c.shape,))
    uni, inter = c[:, 0:1], c[:, 1:2]
    out = np.ones((c.shape[0], c.shape[1] - 2), np.float64)
    np.divide((c[:, 2:] + uni - inter).astype(np.float64), uni.astype(np.float64), out=out, where=uni != 0)
    return out


class DeviceVsdScorer:
    """verts, faces: one [V, 3] and one [T, 3] array per object (object_index in `counts` indexes them), uploaded once.  `near`, `far`
    (millimetres) and `sample_offset` go to the renderer; 0.0 puts pixel centres at integer coordinates, BOP's convention."""

    def __init__(self, verts: Sequence, faces: Sequence, device, near: float = DEFAULT_NEAR, far: float = DEFAULT_FAR, sample_offset: float = 0.0,
                 workspace_cap: Optional[int] = None):
        from .. import _lib
        from ..data_handler.bop_converter import DEFAULT_WORKSPACE_CAP, R_DROPPED, MaskRenderer

        if len(verts) != len(faces) or len(verts) < 1:
            raise ValueError("verts and faces hold one array per object (got %d and %d)" % (len(verts), len(faces)))
        self._lib_module, self._lib = _lib, _lib.load()
        self.objects = len(verts)
        self.renderer = MaskRenderer(device, {i: (verts[i], faces[i]) for i in range(self.objects)},
                                     DEFAULT_WORKSPACE_CAP if workspace_cap is None else workspace_cap)
        self.device = self.renderer.device
        self.near, self.far, self.sample_offset = float(near), float(far), float(sample_offset)
        self._r_dropped = R_DROPPED
        self.last_dropped = 0      # triangles dropped at the near plane by the last counts() call, over all renders
        self.last_chunks = 0       # render + count launches of the last counts() call
        self.last_renders = 0      # planes rendered by the last counts() call

    # ---- one chunk: whole images of one size --------------------------------------------------------------------------------------------
    def prepare(self, images: Sequence[dict], H: int, W: int, imax: int, delta: float, taus: np.ndarray) -> dict:
        """Render the slots of `images` (dicts of cam, depth, slots [(object, pose)], pairs [(pair, slot_e, slot_g, diameter)]) and upload what
        the kernel reads -> the device arrays of one cp_vsd_counts_i32 call."""
        import torch

        r, dev = self.renderer, self.device
        frames, table, where, diam = [], [], [], []
        for m, im in enumerate(images):
            first = len(frames)
            for lo in range(0, len(im["slots"]), imax):
                frames.append(dict(cam=im["cam"], instances=[(o, 1, pose) for o, pose in im["slots"][lo:lo + imax]]))
            plane = lambda s: (first + s // imax) * imax + s % imax   # noqa: E731
            for pair, se, sg, d in im["pairs"]:
                table.append((m, plane(se), plane(sg), 0))
                where.append(pair)
                diam.append(d)
        stream = torch.cuda.current_stream(dev).cuda_stream
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        size = int(self._lib.cp_render_masks_workspace_bytes(len(frames), imax, H, W))
        workspace = torch.empty(size, dtype=torch.uint8, device=dev)
        packed = {k: up(a) for k, a in r.pack(frames, imax).items()}
        _, records = r._render(r.d_mesh, packed, len(frames), H, W, self.near, self.far, self.sample_offset, workspace, size, dev, stream)
        return dict(planes=workspace, records=records, nplanes=len(frames) * imax, H=H, W=W,
                    depth=up(np.stack([np.asarray(im["depth"], np.float32) for im in images])),
                    cams=up(np.asarray([im["cam"] for im in images], np.float64).reshape(-1, 4)), images=len(images),
                    pairs=up(np.asarray(table, np.int32).reshape(-1, 4)), diameters=up(np.asarray(diam, np.float64)), npairs=len(table),
                    delta=float(delta), taus=up(taus), ntau=len(taus), where=np.asarray(where, np.int64),
                    counts=torch.empty((len(table), 2 + len(taus)), dtype=torch.int32, device=dev))

    def launch(self, job: dict, split: int = DEFAULT_SPLIT) -> None:
        """cp_vsd_counts_i32 on the current stream over a prepared chunk; the counts stay on the device in job["counts"]"""
        import torch

        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._lib_module.check(self._lib.cp_vsd_counts_i32(job["planes"].data_ptr(), job["records"].data_ptr(), job["nplanes"], job["H"], job["W"],
                                                           job["depth"].data_ptr(), job["cams"].data_ptr(), job["images"], job["pairs"].data_ptr(),
                                                           job["diameters"].data_ptr(), job["npairs"], job["delta"], job["taus"].data_ptr(), job["ntau"],
                                                           int(split), job["counts"].data_ptr(), stream), "cp_vsd_counts_i32")

    # ---- all pairs --------------------------------------------------------------------------------------------------------------------------
    def counts(self, est, gt, K, object_index, image_index, depths: Sequence, diameters, delta: float = VSD_DELTA, taus: Sequence[float] = VSD_TAUS,
               workspace_cap: Optional[int] = None, split: int = DEFAULT_SPLIT) -> np.ndarray:
        """-> int32 [n, 2 + ntau].  est, gt [n, 3, 4] (or [n, 12]) float64; K [n, 3, 3] or one [3, 3], of which fx, fy, cx, cy are read;
        object_index [n] into the meshes; image_index [n] into `depths`, float32 [H, W] millimetre images that may differ in size; diameters
        [n].  Per image every distinct (object, pose) among its estimates and ground truths is rendered once; the pairs of an image go to the
        kernel together with it, images of one size share launches, and launches are cut where the depth planes would pass the workspace cap."""
        import torch

        if self.device is None:
            raise self._lib_module.CasaposeHipError("DeviceVsdScorer was built without a device; there is no host fall-back")
        est, gt = _np(est, np.float64).reshape(-1, 12), _np(gt, np.float64).reshape(-1, 12)
        obj = _np(object_index, np.int64).reshape(-1)
        img = _np(image_index, np.int64).reshape(-1)
        dia = _np(diameters, np.float64).reshape(-1)
        taus = np.ascontiguousarray(np.asarray(taus, np.float64).reshape(-1))
        n = len(obj)
        if not 1 <= len(taus) <= MAX_TAUS:
            raise ValueError("ntau must lie in [1, %d] (got %d)" % (MAX_TAUS, len(taus)))
        if not (len(est) == len(gt) == len(img) == len(dia) == n):
            raise ValueError("est, gt, object_index, image_index and diameters must have one entry per pair")
        if n and (obj.min() < 0 or obj.max() >= self.objects):
            raise ValueError("object_index must lie in [0, %d)" % self.objects)
        if n and (img.min() < 0 or img.max() >= len(depths)):
            raise ValueError("image_index must lie in [0, %d)" % len(depths))
        cams = _np(K, np.float64)
        cams = np.broadcast_to(cams.reshape(-1, 3, 3), (n, 3, 3)) if n else cams.reshape(-1, 3, 3)
        out = np.zeros((n, 2 + len(taus)), np.int32)
        self.last_dropped = self.last_chunks = self.last_renders = 0

        images: Dict[int, dict] = {}
        for p in range(n):
            im = images.get(int(img[p]))
            if im is None:
                k = cams[p]
                im = images[int(img[p])] = dict(cam=(k[0, 0], k[1, 1], k[0, 2], k[1, 2]), depth=depths[int(img[p])], slots=[], index={}, pairs=[])
            slot = []
            for pose in (est[p], gt[p]):
                key = (int(obj[p]), pose.tobytes())
                if key not in im["index"]:
                    im["index"][key] = len(im["slots"])
                    im["slots"].append((int(obj[p]), pose.reshape(3, 4)))
                slot.append(im["index"][key])
            im["pairs"].append((p, slot[0], slot[1], dia[p]))
        by_size: Dict[Tuple[int, int], List[dict]] = {}
        for im in images.values():
            shape = np.shape(im["depth"])
            if len(shape) != 2:
                raise ValueError("a depth image is [H, W] (got %s)" % (shape,))
            by_size.setdefault((int(shape[0]), int(shape[1])), []).append(im)

        from ..data_handler.bop_converter import MAX_INSTANCES

        with torch.cuda.device(self.device):
            for (H, W), members in by_size.items():
                imax = min(MAX_INSTANCES, max(len(im["slots"]) for im in members))
                frames_of = [-(-len(im["slots"]) // imax) for im in members]
                step = self.renderer.chunk_frames(sum(frames_of), imax, H, W, workspace_cap)
                chunk: List[dict] = []
                used = 0
                for im, f in list(zip(members, frames_of)) + [(None, 0)]:
                    if im is not None and f > step:
                        raise ValueError("an image with %d render slots needs %d frames of depth planes, the workspace cap allows %d"
                                         % (len(im["slots"]), f, step))
                    if chunk and (im is None or used + f > step):
                        job = self.prepare(chunk, H, W, imax, delta, taus)
                        self.launch(job, split)
                        out[job["where"]] = job["counts"].cpu().numpy()
                        self.last_dropped += int(job["records"][..., self._r_dropped].sum().item())
                        self.last_chunks += 1
                        self.last_renders += sum(len(c["slots"]) for c in chunk)
                        chunk, used = [], 0
                    if im is not None:
                        chunk.append(im)
                        used += f
        return out


class BopVsd:
    """What `bop_scores.score(..., vsd=...)` takes: a DeviceVsdScorer whose mesh o is object object_ids[o] of the score call, and
    depth_of(scene_id, im_id) -> float32 [H, W] millimetres (`read_depth`), called once per image that has pairs."""

    def __init__(self, scorer, depth_of: Callable[[int, int], np.ndarray], delta: float = VSD_DELTA, taus: Sequence[float] = VSD_TAUS):
        self.scorer, self.depth_of, self.delta, self.taus = scorer, depth_of, float(delta), tuple(taus)

    def errors(self, est, gt, K, object_index, image_keys: Sequence[Tuple[int, int]], diameters) -> np.ndarray:
        """-> float64 [n, ntau]: e_VSD of every pair at every tau"""
        index: Dict[Tuple[int, int], int] = {}
        for key in image_keys:
            index.setdefault((int(key[0]), int(key[1])), len(index))
        depths = [self.depth_of(*key) for key in index]
        counts = self.scorer.counts(est, gt, K, object_index, [index[(int(k[0]), int(k[1]))] for k in image_keys], depths, diameters, self.delta, self.taus)
        return vsd_errors(counts)


def images_with_pairs(results: Dict[str, np.ndarray], gts: Dict[Tuple[int, int], List[dict]], targets: Optional[Iterable[dict]] = None) -> List[Tuple[int, int]]:
    """The (scene_id, im_id) whose depth image `bop_scores.score` will ask for: those with a target that has a candidate instance and a row of
    the result file that is an estimate, sorted."""
    wanted = select_targets(gts, targets)
    real = is_estimate(results["score"], results["pose"])
    out = set()
    for i in range(len(results["score"])):
        key = (int(results["scene_id"][i]), int(results["im_id"][i]), int(results["obj_id"][i]))
        if real[i] and key in wanted and wanted[key][1]:
            out.add(key[:2])
    return sorted(out)


def depth_path(split_path: str, scene_folder: str, depth_folder: str, im_id: int) -> str:
    return os.path.join(split_path, scene_folder, depth_folder, "%06d.png" % int(im_id))


def match_and_recall_vsd(groups: Iterable[Tuple[int, int, np.ndarray]]) -> dict:
    """groups: one (obj_id, inst_count, e [estimates, instances, ntau]) per (scene, image, object) that holds targets, the estimates in
    descending order of score.  For every tau and every theta the estimates are matched greedily (`greedy_matches`, correct when e < theta);
    recall = matched targets / targets; AR_VSD = the mean over all ntau x 10 recalls.  -> {"targets", "AR_VSD", "recall_vsd" [tau][theta],
    "vsd_thresholds", "objects": {str(obj_id): {"targets", "AR_VSD", "recall_vsd"}}}, plain Python numbers."""
    total: Dict[int, int] = {}
    hits: Dict[int, np.ndarray] = {}
    ntau = None
    for obj, count, e in groups:
        obj, e = int(obj), np.asarray(e, np.float64)
        if e.ndim != 3:
            raise ValueError("a group's errors are [estimates, instances, ntau] (got %s)" % (e.shape,))
        if ntau is None:
            ntau = e.shape[2]
        if e.shape[2] != ntau:
            raise ValueError("groups disagree about ntau (%d and %d)" % (ntau, e.shape[2]))
        total[obj] = total.get(obj, 0) + int(count)
        h = hits.setdefault(obj, np.zeros((ntau, len(VSD_THRESHOLDS)), np.int64))
        for t in range(ntau):
            for i, theta in enumerate(VSD_THRESHOLDS):
                h[t, i] += greedy_matches(e[:, :, t], theta)
    ntau = len(VSD_TAUS) if ntau is None else ntau

    def entry(n, h):
        rec = [[float(x) / n if n else 0.0 for x in row] for row in h]
        return {"targets": int(n), "AR_VSD": sum(sum(row) for row in rec) / float(ntau * len(VSD_THRESHOLDS)), "recall_vsd": rec}

    out = entry(sum(total.values()), sum(hits.values()) if hits else np.zeros((ntau, len(VSD_THRESHOLDS)), np.int64))
    out["vsd_thresholds"] = list(VSD_THRESHOLDS)
    out["objects"] = {str(obj): entry(total[obj], hits[obj]) for obj in sorted(total)}
    return out


def add_vsd_scores(out: dict, vsd: dict, taus: Sequence[float] = VSD_TAUS) -> dict:
    """`match_and_recall`'s dict with `match_and_recall_vsd`'s merged in: AR_VSD, recall_vsd and AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3, over all
    objects and per object (both list the same objects: they come from the same groups)."""
    for dst, src in [(out, vsd)] + [(out["objects"][o], vsd["objects"][o]) for o in out["objects"]]:
        dst["AR_VSD"], dst["recall_vsd"] = src["AR_VSD"], src["recall_vsd"]
        dst["AR"] = (dst["AR_VSD"] + dst["AR_MSSD"] + dst["AR_MSPD"]) / 3.0
    out["vsd_taus"], out["vsd_thresholds"] = [float(t) for t in taus], vsd["vsd_thresholds"]
    return out


__all__ = ["VSD_DELTA", "VSD_TAUS", "VSD_THRESHOLDS", "DEFAULT_NEAR", "DEFAULT_FAR", "read_depth", "vsd_errors", "DeviceVsdScorer", "BopVsd",
           "images_with_pairs", "depth_path", "match_and_recall_vsd", "add_vsd_scores"]
