"""Refine estimated poses against the sensor's depth image: projective point-to-plane ICP on the GPU.

Per iteration every estimate is rendered to a depth plane (the mask renderer, csrc/masks.hip, at BOP's sample offset 0.0) and one Gauss-Newton
step is taken on the pixels where the render and the sensor agree within a gate (cp_depth_icp_step_f64, csrc/depth_icp.hip, rules in
csrc/icp_math.h).  The step rewrites the renderer's own device pose array, so a chunk's loop is `iterations` x (render, step) and one last
(render, step without update) on the current stream with no host synchronisation in between, then one copy back.

A refined pose is kept only if every iteration solved, the last pass used at least max(min_pixels, first-pass pixels / 2) pixels and its RMS
residual is not above the first pass's; otherwise the input pose comes back unchanged and `info["status"]` says why.  There is no host
fall-back: without a device `refine` raises `CasaposeHipError` unless it is asked for `host=True`, which drives the same loop through the
renderer's and the step's host twins (the same bytes, for tests and machines without a GPU)."""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .bop_vsd import DEFAULT_FAR, DEFAULT_NEAR
from .pose_evaluation import _np
from .refine_common import ChunkedRefiner, result_info

# info["status"]: 0-3 are the step's own (csrc/icp_math.h), 4 and 5 the loop's
REFINED, FEW_PIXELS, SINGULAR, REFUSED, LOST_PIXELS, RMS_ROSE = range(6)
STATUS_NAMES = ("refined", "few_pixels", "singular", "refused", "lost_pixels", "rms_rose")
DEFAULT_SPLIT = 4      # blocks per job in the accumulation: 2 .. 12 are within 1 % of each other in tools/depth_icp_probe.py
MAX_SPLIT = 64


def keep_rule(status, stats, min_pixels: int) -> np.ndarray:
    """status int [passes, n] and stats float [passes, n, 4] of a loop's passes (the last one without update) -> int32 [n]: REFINED or why the
    input pose is kept -- the first pass that did not solve gives its status; then LOST_PIXELS when the last pass used fewer than
    max(min_pixels, first-pass pixels / 2) pixels; then RMS_ROSE when the last pass's RMS residual is above the first's."""
    status, stats = np.asarray(status), np.asarray(stats)
    out = np.zeros(status.shape[1], np.int32)
    for n in range(status.shape[1]):
        bad = np.flatnonzero(status[:, n] != 0)
        if len(bad):
            out[n] = status[bad[0], n]
        elif stats[-1, n, 0] < max(float(min_pixels), stats[0, n, 0] / 2.0):
            out[n] = LOST_PIXELS
        elif stats[-1, n, 1] > stats[0, n, 1]:
            out[n] = RMS_ROSE
    return out


class DeviceDepthRefiner(ChunkedRefiner):
    """verts, faces: one [V, 3] and one [T, 3] array per object (object_index in `refine` indexes them), uploaded once.  `near`, `far`
    (millimetres) bound the rendered depths; `workspace_cap` bounds the bytes of depth planes plus step records of one chunk."""

    def __init__(self, verts: Sequence, faces: Sequence, device, near: float = DEFAULT_NEAR, far: float = DEFAULT_FAR,
                 workspace_cap: Optional[int] = None):
        super().__init__(verts, faces, device, near, far, workspace_cap)

    # ---- one chunk: frames of one image size ---------------------------------------------------------------------------------------------
    def prepare(self, frames: List[dict], depths: List[np.ndarray], cams: np.ndarray, jobs: np.ndarray, gates: np.ndarray, imax: int, H: int, W: int,
                passes: int, host: bool = False) -> dict:
        """Upload a chunk: frames of `imax` render slots (dicts of cam and instances [(object, label, pose)]), the `depths` and `cams` of its
        images, jobs int32 [n, 4] (image, slot, 0, 0) with their gates in millimetres -> the arrays `render`, `step` and `finish` work on, on
        the device or (host) as NumPy arrays.  Poses, stats and status share one buffer, so that `finish` is one copy."""
        from .. import twin

        c = self.buffers(frames, len(jobs), imax, H, W, passes, host)
        dev = c["device"]
        icp_size = int(self._lib.cp_depth_icp_workspace_bytes(len(jobs), H, W))
        c.update(icp=twin.alloc(dict(icp=((icp_size // 8,), np.float64)), dev)["icp"], icp_bytes=icp_size,
                 depth=twin.array(np.stack([np.asarray(a, np.float32) for a in depths]), np.float32, dev), images=len(depths),
                 cams=twin.array(cams, np.float64, dev), jobs=twin.array(jobs, np.int32, dev), gates=twin.array(gates, np.float64, dev))
        return c

    def step(self, c: dict, it: int, update: int, jump: float, damping: float, min_pixels: int, split: int = DEFAULT_SPLIT) -> None:
        """cp_depth_icp_step_f64 (or its host twin) over the chunk's last render; stats and status go to row `it`"""
        from .. import twin

        n = c["njobs"]
        twin.call("cp_depth_icp_step_f64", c["planes"], c["records"], c["slots"], c["H"], c["W"], c["depth"], c["cams"], c["images"], c["jobs"], c["gates"],
                  n, float(jump), float(damping), int(min_pixels), int(update), int(split), c["packed"]["poses"], c["stats"][it * n * 4:(it + 1) * n * 4],
                  c["status"][it * n:(it + 1) * n], c["icp"], c["icp_bytes"], host=c["device"] is None, stream=c["stream"])

    # ---- all estimates ---------------------------------------------------------------------------------------------------------------------
    def refine(self, poses, K, object_index, image_index, depths: Sequence, diameters, iterations: int = 8, gate: float = 0.25, jump: float = 0.75,
               damping: float = 1e-6, min_pixels: int = 32, host: bool = False, split: int = DEFAULT_SPLIT,
               workspace_cap: Optional[int] = None) -> Tuple[np.ndarray, dict]:
        """-> (poses float64 [n, 3, 4], info).  poses [n, 3, 4] (or [n, 12]) float64, model -> camera in millimetres; K [n, 3, 3] or one
        [3, 3], of which fx, fy, cx, cy are read (one camera per image: the first estimate's); object_index [n] into the meshes; image_index
        [n] into `depths`, float32 [H, W] millimetre images (0 = no measurement) that may differ in size; diameters [n].

        `gate` is in object diameters: a pixel counts where sensor and render differ by less than gate x diameter.  `jump` is in gates: a
        pixel whose rendered neighbours differ by jump x gate x diameter or more is a depth step and is skipped.  `damping` is relative to
        the diagonal of the normal matrix.  The defaults are starting points that worked on synthetic scenes (a 165 mm object at a 40 mm
        gate and a 30 mm jump), not measured optima on any dataset.

        info: "status" int32 [n] (index into STATUS_NAMES; 0 = the refined pose was kept, anything else = the input pose is returned),
        "status_names", "pixels_first", "pixels_last", "rms_first", "rms_last" [n] of the first and the last pass, "step_status" int32
        [iterations + 1, n] and "step_stats" float64 [iterations + 1, n, 4] of every pass.

        The estimates of one image size are packed into render frames of up to 256 and cut into chunks under `workspace_cap` (depth planes
        plus step records); no result depends on the cut."""
        if not host and self.device is None:
            raise self._lib_module.CasaposeHipError("DeviceDepthRefiner was built without a device; there is no host fall-back (ask for host=True)")
        est = _np(poses, np.float64).reshape(-1, 12)
        obj = _np(object_index, np.int64).reshape(-1)
        img = _np(image_index, np.int64).reshape(-1)
        dia = _np(diameters, np.float64).reshape(-1)
        n = len(obj)
        if not (len(est) == len(img) == len(dia) == n):
            raise ValueError("poses, object_index, image_index and diameters must have one entry per estimate")
        if int(iterations) < 1:
            raise ValueError("iterations must be at least 1 (got %d)" % iterations)
        if not (gate > 0.0 and jump > 0.0):
            raise ValueError("gate and jump must be positive (got %g, %g)" % (gate, jump))
        if not (damping >= 0.0 and np.isfinite(damping)):
            raise ValueError("damping must be finite and not negative (got %g)" % damping)
        if int(min_pixels) < 1:
            raise ValueError("min_pixels must be at least 1 (got %d)" % min_pixels)
        if not 1 <= int(split) <= MAX_SPLIT:
            raise ValueError("split must lie in [1, %d] (got %d)" % (MAX_SPLIT, split))
        if n and (obj.min() < 0 or obj.max() >= self.objects):
            raise ValueError("object_index must lie in [0, %d)" % self.objects)
        if n and (img.min() < 0 or img.max() >= len(depths)):
            raise ValueError("image_index must lie in [0, %d)" % len(depths))
        if n and not (dia > 0.0).all():
            raise ValueError("diameters must be positive")
        cams = _np(K, np.float64)
        cams = np.broadcast_to(cams.reshape(-1, 3, 3), (n, 3, 3)) if n else cams.reshape(-1, 3, 3)
        passes = int(iterations) + 1
        out = est.copy()
        step_status = np.zeros((passes, n), np.int32)
        step_stats = np.zeros((passes, n, 4), np.float64)
        self.last_chunks = self.last_renders = 0

        by_size: Dict[Tuple[int, int], Dict[int, List[int]]] = {}
        for p in range(n):
            shape = np.shape(depths[int(img[p])])
            if len(shape) != 2:
                raise ValueError("a depth image is [H, W] (got %s)" % (shape,))
            by_size.setdefault((int(shape[0]), int(shape[1])), {}).setdefault(int(img[p]), []).append(p)
        cap = self.workspace_cap if workspace_cap is None else int(workspace_cap)
        on_device = contextlib.nullcontext()
        if not host:
            import torch

            on_device = torch.cuda.device(self.device)      # the launches go to the calling thread's current device
        for (H, W), members in by_size.items():
            imax, chunks = self.frame_chunks(members, H, W, lambda slots: self._lib.cp_depth_icp_workspace_bytes(slots, H, W), cap,
                                             "depth planes and step records")
            for part in chunks:
                local: Dict[int, int] = {}
                for m, _ in part:
                    local.setdefault(m, len(local))
                cam_of = {}
                for m, rows in part:
                    k = cams[rows[0]]
                    cam_of.setdefault(m, (k[0, 0], k[1, 1], k[0, 2], k[1, 2]))
                image_cams = np.asarray([cam_of[m] for m in local], np.float64).reshape(-1, 4)
                rframes = [dict(cam=cam_of[m], instances=[(int(obj[p]), 1, est[p].reshape(3, 4)) for p in rows]) for m, rows in part]
                jobs = np.asarray([(local[m], f * imax + k, 0, 0) for f, (m, rows) in enumerate(part) for k in range(len(rows))], np.int32)
                where = np.asarray([p for _, rows in part for p in rows], np.int64)
                with on_device:
                    c = self.prepare(rframes, [depths[m] for m in local], image_cams, jobs, float(gate) * dia[where], imax, H, W, passes, host)
                    for it in range(passes):
                        self.render(c)
                        self.step(c, it, int(it + 1 < passes), jump, damping, min_pixels, split)
                    got_poses, got_stats, got_status = self.finish(c)
                out[where] = got_poses[jobs[:, 1]]
                step_stats[:, where], step_status[:, where] = got_stats, got_status
                self.last_chunks += 1
                self.last_renders += passes * len(where)
        status = keep_rule(step_status, step_stats, int(min_pixels))
        out[status != REFINED] = est[status != REFINED]
        info = result_info(step_status, step_stats, status, STATUS_NAMES)
        return out.reshape(n, 3, 4), info


__all__ = ["REFINED", "FEW_PIXELS", "SINGULAR", "REFUSED", "LOST_PIXELS", "RMS_ROSE", "STATUS_NAMES", "keep_rule", "DeviceDepthRefiner"]
