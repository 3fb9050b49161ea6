"""Refine estimated poses against the network's own label map: contour alignment on the GPU.

The filtered label map of the inference path (`CoordLSVotingWeighted.last_labels`) gives each object's visible silhouette and tells which part
of its boundary borders background and which part borders another object.  Per chunk the squared distance to the trusted boundary -- towards
background only -- is computed once per (image, label) (cp_mask_edt_u16); then per iteration every estimate is rendered to a depth plane (the
mask renderer, csrc/masks.hip, at the label map's sample offset) and one 2-D Gauss-Newton step moves the rendered silhouette's contour pixels along the
distance's gradient (cp_contour_step_f64, csrc/mask_contour.hip, rules in csrc/contour_math.h).  The step rewrites the renderer's own device
pose array, so a chunk's loop is one upload, one distance transform, `iterations` x (render, step), one last (render, step without update)
on the current stream with no host synchronisation in between, then one copy back.

The keep rule and the status names are depth_refine's.  There is no host fall-back: without a device `refine` raises `CasaposeHipError` unless
it is asked for `host=True`, which drives the same loop through the host twins (the same bytes, for tests and machines without a GPU)."""
from __future__ import annotations

import contextlib
import os
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .bop_vsd import DEFAULT_FAR, DEFAULT_NEAR
from .depth_refine import DEFAULT_SPLIT, MAX_SPLIT, REFINED, STATUS_NAMES, keep_rule
from .pose_evaluation import _np
from .refine_common import ChunkedRefiner, mask_refine_enabled, result_info

# Starting points, not optima: picked on the synthetic block scenes of tests/contour_cases.py, where an object is about 25 pixels across, a
# start is up to 3 pixels off and a contour has 60 to 80 pixels.  A rendered contour pixel farther than `gate` pixels from the trusted boundary
# is left out, which is what keeps the part of the render that lies under an occluder from pulling; a gate much above the start's error lets
# that part in.  Larger images want both numbers scaled with the object's size in pixels.
DEFAULT_GATE = 3
DEFAULT_MIN_PIXELS = 24
MAX_GATE = 255


class DeviceMaskRefiner(ChunkedRefiner):
    """verts, faces: one [V, 3] and one [T, 3] array per object (object_index in `refine` indexes them), uploaded once.  `near`, `far` (in the
    meshes' unit) bound the rendered depths; `workspace_cap` bounds the bytes of depth planes, distance fields and step records of one chunk.
    `sample_offset` is where a pixel of the label map was sampled: 0.5, the convention of the reader's masks (data_handler/bop_converter.py)."""

    def __init__(self, verts: Sequence, faces: Sequence, device, near: float = DEFAULT_NEAR, far: float = DEFAULT_FAR,
                 workspace_cap: Optional[int] = None, sample_offset: float = 0.5):
        super().__init__(verts, faces, device, near, far, workspace_cap, sample_offset)
        self.last_fields = 0       # distance fields computed by the last refine() call
        self.last_info = None      # refine_estimates: the info of its last call

    def _chunk_bytes(self, slots: int, H: int, W: int) -> int:
        """the step records of `slots` jobs and as many distance fields with their row pass: what a render frame adds to its depth planes"""
        return int(self._lib.cp_contour_step_workspace_bytes(slots, H, W)) + 2 * int(self._lib.cp_mask_edt_workspace_bytes(slots, H, W))

    # ---- one chunk -------------------------------------------------------------------------------------------------------------------------
    def prepare(self, frames: List[dict], labels, images: int, cams: np.ndarray, jobs: np.ndarray, fields: np.ndarray, imax: int, H: int, W: int,
                passes: int, host: bool = False) -> dict:
        """Upload a chunk: frames of `imax` render slots, the label maps uint8 [images, H, W] (already where the chunk runs) with `cams`
        [images, 4], jobs int32 [n, 4] (image, slot, field, gate) and fields int32 [f, 2] (image, label) -> the arrays `distance`, `render`,
        `step` and `finish` work on."""
        from .. import twin

        c = self.buffers(frames, len(jobs), imax, H, W, passes, host)
        dev = c["device"]
        nf = len(fields)
        step_size = int(self._lib.cp_contour_step_workspace_bytes(len(jobs), H, W))
        edt_size = int(self._lib.cp_mask_edt_workspace_bytes(nf, H, W))
        work = twin.alloc(dict(step=((step_size // 8,), np.float64), fields=((nf, H, W), np.uint16), rows=((edt_size // 2,), np.uint16),
                               field_status=((nf,), np.int32)), dev)
        c.update(step_work=work["step"], step_bytes=step_size, fields=work["fields"], nfields=nf, rows=work["rows"], rows_bytes=edt_size,
                 field_status=work["field_status"], labels=labels, images=images, cams=twin.array(cams, np.float64, dev),
                 jobs=twin.array(jobs, np.int32, dev), field_jobs=twin.array(fields, np.int32, dev))
        return c

    def distance(self, c: dict, gate: int) -> None:
        """cp_mask_edt_u16 (or its host twin): the chunk's distance fields"""
        from .. import twin

        twin.call("cp_mask_edt_u16", c["labels"], c["images"], c["H"], c["W"], c["field_jobs"], c["nfields"], int(gate), c["fields"], c["field_status"],
                  c["rows"], c["rows_bytes"], host=c["device"] is None, stream=c["stream"])

    def step(self, c: dict, it: int, update: int, damping: float, min_pixels: int, split: int = DEFAULT_SPLIT) -> None:
        """cp_contour_step_f64 (or its host twin) over the chunk's last render; stats and status go to row `it`"""
        from .. import twin

        n = c["njobs"]
        twin.call("cp_contour_step_f64", c["planes"], c["records"], c["slots"], c["H"], c["W"], c["fields"], c["nfields"], c["cams"], c["images"], c["jobs"],
                  n, self.sample_offset, float(damping), int(min_pixels), int(update), int(split), c["packed"]["poses"], c["stats"][it * n * 4:(it + 1) * n * 4],
                  c["status"][it * n:(it + 1) * n], c["step_work"], c["step_bytes"], host=c["device"] is None, stream=c["stream"])

    # ---- all estimates ---------------------------------------------------------------------------------------------------------------------
    def refine(self, poses, K, object_index, image_index, labels, label_of, iterations: int = 8, gate: int = DEFAULT_GATE, damping: float = 1e-6,
               min_pixels: int = DEFAULT_MIN_PIXELS, host: bool = False, split: int = DEFAULT_SPLIT,
               workspace_cap: Optional[int] = None) -> Tuple[np.ndarray, dict]:
        """-> (poses float64 [n, 3, 4], info).  poses [n, 3, 4] (or [n, 12]) float64, model -> camera in the meshes' unit; K [n, 3, 3] or one
        [3, 3], of which fx, fy, cx, cy are read (one camera per image: the first estimate's); object_index [n] into the meshes; image_index
        [n] into `labels`, a uint8 [images, H, W] device tensor (a NumPy array with host=True) in the frame of K, 0 = background;
        label_of [n]: the label value of each estimate's object, 1 .. 255.

        `gate` is in whole pixels, 1 .. 255: a rendered contour pixel counts where it and its four neighbours lie within `gate` pixels of the
        label's boundary towards background.  `damping` is relative to the diagonal of the normal matrix.  `gate` and `min_pixels` default to
        DEFAULT_GATE and DEFAULT_MIN_PIXELS: starting points that worked on synthetic scenes, not measured optima on any dataset.

        info: as DeviceDepthRefiner.refine's -- "status" int32 [n] (index into "status_names"; 0 = the refined pose was kept, anything else =
        the input pose is returned), "pixels_first", "pixels_last", "rms_first", "rms_last" [n] of the first and the last pass (used contour
        pixels; RMS distance in pixels), "step_status" int32 [iterations + 1, n] and "step_stats" float64 [iterations + 1, n, 4] (used pixels,
        RMS, contour pixels, sum of squared distances) of every pass.

        The estimates are packed into render frames of up to 256 and cut into chunks under `workspace_cap` (depth planes, distance fields
        and step records); no result depends on the cut."""
        if not host and self.device is None:
            raise self._lib_module.CasaposeHipError("DeviceMaskRefiner was built without a device; there is no host fall-back (ask for host=True)")
        est = _np(poses, np.float64).reshape(-1, 12)
        obj = _np(object_index, np.int64).reshape(-1)
        img = _np(image_index, np.int64).reshape(-1)
        lab = _np(label_of, np.int64).reshape(-1)
        n = len(obj)
        if not (len(est) == len(img) == len(lab) == n):
            raise ValueError("poses, object_index, image_index and label_of must have one entry per estimate")
        if int(iterations) < 1:
            raise ValueError("iterations must be at least 1 (got %d)" % iterations)
        if int(gate) != gate or not 1 <= int(gate) <= MAX_GATE:
            raise ValueError("gate must be a whole number of pixels in [1, %d] (got %r)" % (MAX_GATE, gate))
        if not (damping >= 0.0 and np.isfinite(damping)):
            raise ValueError("damping must be finite and not negative (got %g)" % damping)
        if int(min_pixels) < 1:
            raise ValueError("min_pixels must be at least 1 (got %d)" % min_pixels)
        if not 1 <= int(split) <= MAX_SPLIT:
            raise ValueError("split must lie in [1, %d] (got %d)" % (MAX_SPLIT, split))
        if len(np.shape(labels)) != 3 or str(labels.dtype).split(".")[-1] != "uint8":
            raise ValueError("labels is a uint8 [images, H, W] array (got %s %s)" % (str(labels.dtype), tuple(np.shape(labels))))
        if host != isinstance(labels, np.ndarray):
            raise ValueError("labels is a device tensor, or a NumPy array with host=True")
        images, H, W = (int(s) for s in np.shape(labels))
        if n and (obj.min() < 0 or obj.max() >= self.objects):
            raise ValueError("object_index must lie in [0, %d)" % self.objects)
        if n and (img.min() < 0 or img.max() >= images):
            raise ValueError("image_index must lie in [0, %d)" % images)
        if n and (lab.min() < 1 or lab.max() > 255):
            raise ValueError("label_of must lie in [1, 255]")
        cams = _np(K, np.float64)
        cams = np.broadcast_to(cams.reshape(-1, 3, 3), (n, 3, 3)) if n else cams.reshape(-1, 3, 3)
        passes = int(iterations) + 1
        out = est.copy()
        step_status = np.zeros((passes, n), np.int32)
        step_stats = np.zeros((passes, n, 4), np.float64)
        self.last_chunks = self.last_renders = self.last_fields = 0

        members: Dict[int, List[int]] = {}
        for p in range(n):
            members.setdefault(int(img[p]), []).append(p)
        image_cams = np.zeros((images, 4), np.float64)
        for m, rows in members.items():
            k = cams[rows[0]]
            image_cams[m] = (k[0, 0], k[1, 1], k[0, 2], k[1, 2])
        cap = self.workspace_cap if workspace_cap is None else int(workspace_cap)
        on_device = contextlib.nullcontext()
        if not host:
            import torch

            on_device = torch.cuda.device(self.device)      # the launches go to the calling thread's current device
            labels = labels.to(self.device).contiguous()
        else:
            labels = np.ascontiguousarray(labels)
        if n:
            imax, chunks = self.frame_chunks(members, H, W, lambda slots: self._chunk_bytes(slots, H, W), cap,
                                             "depth planes, distance fields and step records")
        for part in chunks if n else []:
            field_of: Dict[Tuple[int, int], int] = {}
            for m, rows in part:
                for p in rows:
                    field_of.setdefault((m, int(lab[p])), len(field_of))
            rframes = [dict(cam=tuple(image_cams[m]), instances=[(int(obj[p]), 1, est[p].reshape(3, 4)) for p in rows]) for m, rows in part]
            jobs = np.asarray([(m, f * imax + k, field_of[m, int(lab[p])], int(gate)) for f, (m, rows) in enumerate(part) for k, p in enumerate(rows)],
                              np.int32)
            where = np.asarray([p for _, rows in part for p in rows], np.int64)
            with on_device:
                c = self.prepare(rframes, labels, images, image_cams, jobs, np.asarray(list(field_of), np.int32).reshape(-1, 2), imax, H, W, passes, host)
                self.distance(c, int(gate))
                for it in range(passes):
                    self.render(c)
                    self.step(c, it, int(it + 1 < passes), damping, min_pixels, split)
                got_poses, got_stats, got_status = self.finish(c)
            out[where] = got_poses[jobs[:, 1]]
            step_stats[:, where], step_status[:, where] = got_stats, got_status
            self.last_chunks += 1
            self.last_renders += passes * len(where)
            self.last_fields += len(field_of)
        status = keep_rule(step_status, step_stats, int(min_pixels))
        out[status != REFINED] = est[status != REFINED]
        return out.reshape(n, 3, 4), result_info(step_status, step_stats, status, STATUS_NAMES)


# ---- the inference scripts (test_casapose.py, util_scripts/test_minimal.py) under CASAPOSE_MASK_REFINE=1 ----------------------------------------
def require_image_frame(offsets, what: str = "CASAPOSE_MASK_REFINE=1") -> None:
    """The label map is in the network's frame and the camera matrix in the image's: the refinement (and the verification, pose_verify.py) needs
    them to be one frame.  offsets [b, 10] or [10] (h_crop, w_crop, -, -, dx, dy, angle, scale, W, H) of a batch; anything but the identity raises
    before any device work, naming `what` -- the switch that asked."""
    o = _np(offsets, np.float64).reshape(-1, 10)
    if not (np.all(o[:, [0, 1, 4, 5, 6]] == 0.0) and np.all(o[:, 7] == 1.0)):
        raise ValueError("%s needs frames that reach the network as they are: the batch's offsets hold a crop, shift, rotation or scale "
                         "(h_crop, w_crop, dx, dy, angle, scale = %s), so the label map and the camera matrix do not share a frame"
                         % (what, o[0, [0, 1, 4, 5, 6, 7]].tolist()))


def mesh_file(path_meshes: str, name: str) -> Optional[str]:
    """the mesh file VectorfieldDataset.load_meshes reads for an object"""
    for ext in (".obj", ".ply"):
        model = os.path.join(path_meshes, name, name + ext)
        if os.path.exists(model):
            return model
    return None


def gather_meshes(verts, counts, path_meshes: str, objects: Sequence[str], what: str = "CASAPOSE_MASK_REFINE=1"):
    """What a renderer over the objects of an inference script needs: verts [oc, Vmax, 3] with counts [oc, 1], the vertices the scripts evaluate
    with (in the keypoints' frame; VectorfieldDataset.generate_object_vertex_array), and the faces of the same mesh files under `path_meshes`
    -> (one [V, 3] array per object, one [T, 3] array per object, the largest coordinate).  Missing files or meshes without faces raise before
    any device work, naming `what` -- the switch that asked."""
    from ..data_handler.vectorfield_dataset import read_faces

    if not path_meshes or not os.path.isdir(str(path_meshes)) or verts is None or counts is None:
        raise ValueError("%s needs the objects' mesh files under --datameshes (got %r)" % (what, path_meshes))
    verts, counts = _np(verts, np.float32), _np(counts, np.int64).reshape(-1)
    faces = []
    for i, name in enumerate(objects):
        model = mesh_file(path_meshes, name)
        if model is None or i >= len(counts) or int(counts[i]) == 0:
            raise ValueError("%s needs a mesh for every object: %s has none under %s" % (what, name, path_meshes))
        f = read_faces(model)
        if len(f) == 0:
            raise ValueError("%s needs meshes with faces to render: %s holds vertices only" % (what, model))
        faces.append(f)
    vs = [np.asarray(verts[i, :int(counts[i])], np.float32) for i in range(len(objects))]
    return vs, faces, max(float(np.abs(v).max()) for v in vs)


def refiner_for_meshes(verts, counts, path_meshes: str, objects: Sequence[str], device) -> "DeviceMaskRefiner":
    """A refiner over the objects of an inference script (gather_meshes says what it takes)."""
    vs, faces, reach = gather_meshes(verts, counts, path_meshes, objects)
    return DeviceMaskRefiner(vs, faces, device, near=1e-2 * reach, far=1e4 * reach)          # the depth range in the meshes' own unit, whatever it is


def refiner_for_dataset(dataset, path_meshes: str, objects: Sequence[str], device) -> "DeviceMaskRefiner":
    """refiner_for_meshes over a VectorfieldDataset's evaluation vertices"""
    if not hasattr(dataset, "generate_object_vertex_array"):
        raise ValueError("CASAPOSE_MASK_REFINE=1 needs the objects' mesh files under --datameshes (got %r)" % (path_meshes,))
    verts, counts = dataset.generate_object_vertex_array()
    return refiner_for_meshes(verts, counts, path_meshes, objects, device)


_refiners: Dict[tuple, object] = {}     # refiner_from_environment: a refiner; refine_voted_poses: (weak reference to its dataset, refiner)


def refiner_from_environment(opt, evaluation_points, object_points_3d_count, device) -> Optional["DeviceMaskRefiner"]:
    """What training.test_step asks (test_casapose.py): None unless CASAPOSE_MASK_REFINE=1; then the one refiner kept for the script's meshes --
    `opt.datameshes`, `opt.object` and the evaluation vertices the script hands to every step."""
    if not mask_refine_enabled():
        return None
    objects = [x.strip() for x in str(getattr(opt, "object", "")).split(",") if x.strip()]
    key = ("opt", str(getattr(opt, "datameshes", "")), tuple(objects), str(device))
    if key not in _refiners:
        _refiners[key] = refiner_for_meshes(evaluation_points, object_points_3d_count, getattr(opt, "datameshes", ""), objects, device)
    return _refiners[key]


def refine_voted_poses(poses, points_estimated, camera_data, device) -> np.ndarray:
    """What pose_evaluation.poses_pnp asks under CASAPOSE_MASK_REFINE=1 (util_scripts/test_minimal.py holds only the keypoints): the voter that
    just returned `points_estimated` still has its label map, and the VectorfieldDataset the script built last names the meshes and has the
    offsets of the annotated frame the camera matrix came from.  -> the poses, refined."""
    from ..data_handler.vectorfield_dataset import VectorfieldDataset
    from .voting_layers_2d import voter_of

    voter = voter_of(points_estimated)
    if voter is None:
        raise ValueError("poses_pnp: CASAPOSE_MASK_REFINE=1 needs the keypoints tensor as CoordLSVotingWeighted returned it: this call has no label "
                         "map to align with")
    dataset = VectorfieldDataset.last_instance() if VectorfieldDataset.last_instance is not None else None
    if dataset is None:
        raise ValueError("poses_pnp: CASAPOSE_MASK_REFINE=1 needs the objects' mesh files under --datameshes: no VectorfieldDataset names them")
    if dataset.last_offsets is None:      # no annotated frame was drawn: nothing says that the camera matrix is the label map's
        raise ValueError("poses_pnp: CASAPOSE_MASK_REFINE=1 needs the offsets of the annotated frame the camera matrix came from: the dataset has "
                         "drawn no sample yet")
    require_image_frame(dataset.last_offsets)
    key = ("dataset", str(device))
    kept = _refiners.get(key)
    if kept is None or kept[0]() is not dataset:     # the refiner belongs to this very dataset, not to one that had its id before
        kept = _refiners[key] = (weakref.ref(dataset), refiner_for_dataset(dataset, dataset.path_meshes, dataset.objectsofinterest, device))
    return refine_estimates(kept[1], poses, voter.last_labels, camera_data)


def refine_estimates(refiner: "DeviceMaskRefiner", poses, labels, camera_matrix, **kw) -> np.ndarray:
    """The PnP poses of a batch, refined.  poses [b, oc, 1, 3, 4] or [b, oc, 3, 4] (the zero pose = not found, passed through); labels: the
    voter's `last_labels`, uint8 [b, h, w] on the device, in which object o has the value o + 1; camera_matrix [b, 3, 3] or [3, 3].
    -> an array of the shape and type of `poses`; `refiner.last_info` holds the info of the call (None when nothing was found)."""
    given = np.asarray(poses)
    b, oc = given.shape[:2]
    flat = given.reshape(b, oc, 3, 4)
    found = np.argwhere(np.abs(flat).sum(axis=(2, 3)) > 0)
    refiner.last_info = None
    if len(found) == 0:
        return given
    cams = _np(camera_matrix, np.float64).reshape(-1, 3, 3)
    K = cams[found[:, 0]] if len(cams) == b else cams[0]
    got, refiner.last_info = refiner.refine(flat[found[:, 0], found[:, 1]].astype(np.float64), K, found[:, 1], found[:, 0], labels, found[:, 1] + 1, **kw)
    out = flat.copy()
    out[found[:, 0], found[:, 1]] = got.astype(given.dtype)
    return out.reshape(given.shape)


__all__ = ["DEFAULT_GATE", "DEFAULT_MIN_PIXELS", "DeviceMaskRefiner", "mask_refine_enabled", "require_image_frame", "gather_meshes", "refiner_for_meshes", "refiner_for_dataset",
           "refiner_from_environment", "refine_voted_poses", "refine_estimates"]
