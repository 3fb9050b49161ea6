"""What the render-and-step pose refiners share (depth_refine.DeviceDepthRefiner, mask_refine.DeviceMaskRefiner): the mask renderer with its
meshes uploaded once, the packing of estimates into render frames and chunks under a workspace cap, the one buffer of poses, stats and
statuses that a step kernel rewrites in place, the render of a chunk and the one copy back."""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np


def mask_refine_enabled() -> bool:
    """CASAPOSE_MASK_REFINE=1 (pose_estimation/mask_refine.py); says `refine: mask contours` the first time it is.  It lives here so that the
    voter can read it without importing the refiner."""
    on = os.environ.get("CASAPOSE_MASK_REFINE", "0") == "1"
    if on and not mask_refine_enabled.said:
        mask_refine_enabled.said = True
        print("refine: mask contours (CASAPOSE_MASK_REFINE=1)")
    return on


mask_refine_enabled.said = False


class ChunkedRefiner:
    """verts, faces: one [V, 3] and one [T, 3] array per object (object_index in `refine` indexes them), uploaded once.  `near`, `far`
    (millimetres) bound the rendered depths; `workspace_cap` bounds the bytes of depth planes plus step workspaces of one chunk;
    `sample_offset` is the renderer's."""

    def __init__(self, verts: Sequence, faces: Sequence, device, near: float, far: float, workspace_cap: Optional[int] = None,
                 sample_offset: float = 0.0):
        from .. import _lib
        from ..data_handler.bop_converter import DEFAULT_WORKSPACE_CAP, MaskRenderer

        if len(verts) != len(faces) or len(verts) < 1:
            raise ValueError("verts and faces hold one array per object (got %d and %d)" % (len(verts), len(faces)))
        self._lib_module, self._lib = _lib, _lib.load()
        self.objects = len(verts)
        self.workspace_cap = int(DEFAULT_WORKSPACE_CAP if workspace_cap is None else workspace_cap)
        self.renderer = MaskRenderer(device, {i: (verts[i], faces[i]) for i in range(self.objects)}, self.workspace_cap)
        self.device = self.renderer.device
        self.near, self.far = float(near), float(far)
        self.sample_offset = float(sample_offset)     # where the renderer samples a pixel: 0.0 is BOP's convention, 0.5 the reader's masks'
        self.last_chunks = 0       # chunks of the last refine() call
        self.last_renders = 0      # planes rendered by it, over all passes

    def frame_chunks(self, members: Dict[int, List[int]], H: int, W: int, step_bytes: Callable[[int], int], cap: int,
                     what: str) -> Tuple[int, List[List[Tuple[int, List[int]]]]]:
        """members {image: its estimates} of one image size -> (imax, chunks): the estimates of an image cut into render frames of up to imax
        = min(256, the most estimates of an image) slots, the frames cut into chunks whose depth planes plus step_bytes(imax) per frame stay
        under `cap`.  A chunk is a list of (image, estimates)."""
        from ..data_handler.bop_converter import MAX_INSTANCES

        imax = min(MAX_INSTANCES, max(len(rows) for rows in members.values()))
        frame_planes = int(self._lib.cp_render_masks_workspace_bytes(1, imax, H, W))
        if frame_planes == 0:
            raise ValueError("the renderer takes H, W in [1, 16384] (got %d x %d)" % (H, W))
        one = frame_planes + int(step_bytes(imax))
        if one > cap:
            raise ValueError("one %d x %d frame with %d estimates needs %d bytes of %s, the workspace cap is %d" % (H, W, imax, one, what, cap))
        step = max(1, min(cap // one, 65535))
        frames = []      # (image, rows): up to imax estimates of one image
        for m, rows in members.items():
            for lo in range(0, len(rows), imax):
                frames.append((m, rows[lo:lo + imax]))
        return imax, [frames[lo:lo + step] for lo in range(0, len(frames), step)]

    def buffers(self, frames: List[dict], njobs: int, imax: int, H: int, W: int, passes: int, host: bool = False) -> dict:
        """Upload a chunk's render frames (dicts of cam and instances [(object, label, pose)], `imax` slots each) -> the arrays `render` and
        `finish` work on, on the device or (host) as NumPy arrays.  Poses, stats [passes, njobs, 4] and status [passes, njobs] share one
        buffer, so that `finish` is one copy."""
        from .. import twin

        r = self.renderer
        dev = None if host else self.device
        packed = r.pack(frames, imax)
        slots = len(frames) * imax
        n_pose, n_stats = slots * 12, passes * njobs * 4
        host_buf = np.zeros(n_pose + n_stats + (passes * njobs + 1) // 2, np.float64)
        host_buf[:n_pose] = packed["poses"].reshape(-1)
        buf = twin.array(host_buf, np.float64, dev)
        tail = buf[n_pose + n_stats:]
        if dev is None:
            stream, status = None, tail.view(np.int32)
        else:
            import torch

            stream, status = torch.cuda.current_stream(dev).cuda_stream, tail.view(torch.int32)
        d = {k: twin.array(a, a.dtype, dev) for k, a in packed.items() if k != "poses"}
        d["poses"] = buf[:n_pose]          # the renderer's pose array is the one the step rewrites
        size = int(self._lib.cp_render_masks_workspace_bytes(len(frames), imax, H, W))
        planes = twin.alloc(dict(planes=((size // 4,), np.uint32)), dev)["planes"]
        return dict(device=dev, stream=stream, mesh=(r.verts, r.vert_counts, r.faces, r.face_counts) if dev is None else r.d_mesh, packed=d,
                    frames=len(frames), slots=slots, njobs=njobs, H=H, W=W, passes=passes, buf=buf, n_pose=n_pose, n_stats=n_stats,
                    stats=buf[n_pose:n_pose + n_stats], status=status, planes=planes, planes_bytes=size, records=None)

    def render(self, c: dict) -> None:
        """every slot of the chunk at its current pose: the planes and c["records"]"""
        _, c["records"] = self.renderer._render(c["mesh"], c["packed"], c["frames"], c["H"], c["W"], self.near, self.far, self.sample_offset, c["planes"],
                                                c["planes_bytes"], c["device"], c["stream"])

    def finish(self, c: dict):
        """the one copy back -> (poses [slots, 12], stats [passes, njobs, 4], status [passes, njobs])"""
        back = c["buf"] if c["device"] is None else c["buf"].cpu().numpy()
        n_pose, n_stats, passes, n = c["n_pose"], c["n_stats"], c["passes"], c["njobs"]
        return (back[:n_pose].reshape(c["slots"], 12), back[n_pose:n_pose + n_stats].reshape(passes, n, 4),
                back[n_pose + n_stats:].view(np.int32)[:passes * n].reshape(passes, n))


def result_info(step_status: np.ndarray, step_stats: np.ndarray, status: np.ndarray, names) -> dict:
    """the `info` of a refine() call from every pass's status [passes, n] and stats [passes, n, 4] and the keep rule's verdict [n]"""
    return dict(status=status, status_names=names, pixels_first=step_stats[0, :, 0].astype(np.int64), pixels_last=step_stats[-1, :, 0].astype(np.int64),
                rms_first=step_stats[0, :, 1].copy(), rms_last=step_stats[-1, :, 1].copy(), step_status=step_status, step_stats=step_stats)
