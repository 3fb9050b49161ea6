"""Keypoints and models_info for any set of meshes: what the dataset converter needs per object and neither BOP archives nor BlenderProc output
hold.  Per object: the box centre followed by farthest-point samples of the vertices (the reference's obj_NNNNNN_keypoints.ply, which it ships for
LM and HomebrewedDB only and has no program for), and BOP's models_info entry (diameter = the largest vertex distance, min_*, size_*).

    prep = ModelPrep(device)                      # device=None: the host twin only
    results = prep.prepare({obj: vertices [N, 3]}, no_points=9)        # csrc/models.hip: all objects in one call
    results = prep.prepare_host({obj: vertices [N, 3]}, no_points=9)   # csrc/model_math.h run serially: the same bits
    results[obj] -> keypoints float32 [K, 3], keypoint_indices int32 [K - 1], diameter float, diameter_sq float, min / max float32 [3],
                    size float64 [3], vertices int

The definitions (fp32 box, fp64 centre and squared distances without FMA, lowest index on ties) are listed in csrc/model_math.h.  With a device
requested and no GPU present ModelPrep raises; it never falls back to the host."""
from __future__ import annotations

import contextlib
import json
import os
import re
from typing import Dict, Optional

import numpy as np

from .. import _lib, twin

MIN_POINTS, MAX_POINTS = 2, 32       # cp_model::MIN_POINTS, MAX_POINTS of csrc/model_math.h: the centre counts
MAX_VERTICES = 1 << 22
MAX_OBJECTS = 1024                   # per library call; larger sets go in several calls
ST_OK, ST_BAD_COUNT, ST_TOO_FEW = 0, 1, 2


class ModelPrep:
    def __init__(self, device):
        import torch

        self.lib = _lib.load()
        self.device = None if device is None else torch.device(device)
        if self.device is not None and not torch.cuda.is_available():
            raise _lib.CasaposeHipError("ModelPrep(device=%s) needs a ROCm GPU; the host twin is ModelPrep(None).prepare_host" % (device,))

    # ---- packing ----------------------------------------------------------------------------------
    @staticmethod
    def pack(meshes: Dict[object, np.ndarray], ids) -> Dict[str, np.ndarray]:
        """the vertices of `ids` back to back (a flat array with offsets: no padding that could be taken for a point)"""
        arrays = []
        for obj in ids:
            v = np.asarray(meshes[obj])
            if v.ndim != 2 or v.shape[1] != 3:
                raise ValueError("object %s: vertices are [N, 3] (got %s)" % (obj, v.shape))
            arrays.append(np.ascontiguousarray(v, np.float32))
        counts = np.array([len(v) for v in arrays], np.int64)
        offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        verts = np.concatenate(arrays + [np.zeros((1, 3), np.float32)])   # never empty; the extra row lies outside `total`
        return dict(verts=verts, total=int(counts.sum()), offsets=offsets, counts=np.minimum(counts, 2 ** 31 - 1).astype(np.int32))

    @staticmethod
    def _outputs(objects: int, K: int, device=None) -> dict:
        """the library's output arrays, zeroed: tensors on `device`, or NumPy arrays"""
        return twin.alloc(dict(diameter_sq=((objects,), np.float64), box=((objects, 6), np.float32), keypoints=((objects, K, 3), np.float32),
                               indices=((objects, K - 1), np.int32), status=((objects,), np.int32)), device, zero=True)

    @staticmethod
    def _results(ids, out) -> Dict[object, dict]:
        results, counts = {}, out["counts"]
        for i, obj in enumerate(ids):
            st = int(out["status"][i])
            if st == ST_BAD_COUNT:
                raise ValueError("object %s: %d vertices, the vertex count must lie in [1, %d]" % (obj, int(counts[i]), MAX_VERTICES))
            if st == ST_TOO_FEW:
                raise ValueError("object %s: too few distinct vertices for %d keypoints (the centre and %d different vertices are needed)"
                                 % (obj, out["keypoints"].shape[1], out["keypoints"].shape[1] - 1))
            if st != ST_OK:
                raise _lib.CasaposeHipError("object %s: unknown status %d" % (obj, st))
            mn, mx = out["box"][i, :3].copy(), out["box"][i, 3:].copy()
            results[obj] = dict(keypoints=out["keypoints"][i].copy(), keypoint_indices=out["indices"][i].copy(),
                                diameter=float(np.sqrt(out["diameter_sq"][i])), diameter_sq=float(out["diameter_sq"][i]), min=mn, max=mx,
                                size=mx.astype(np.float64) - mn.astype(np.float64), vertices=int(counts[i]))
        return results

    @staticmethod
    def _check_points(no_points) -> int:
        K = int(no_points)
        if not MIN_POINTS <= K <= MAX_POINTS:
            raise ValueError("no_points counts the centre and must lie in [%d, %d] (got %d)" % (MIN_POINTS, MAX_POINTS, K))
        return K

    # ---- the library call, host twin or device ---------------------------------------------------------
    def outputs(self, meshes: Dict[object, np.ndarray], no_points: int = 9, host: bool = False) -> Dict[str, np.ndarray]:
        """The library's arrays for the objects of `meshes` in its order, statuses included and nothing raised for them: diameter_sq [n], box [n, 6],
        keypoints [n, K, 3], indices [n, K - 1], status [n], counts [n].  host: the serial twin; otherwise the kernels (no fall-back)."""
        import torch

        if not host and self.device is None:
            raise _lib.CasaposeHipError("this ModelPrep was built without a device; there is no fall-back to the host twin (call prepare_host)")
        K, ids, parts = self._check_points(no_points), list(meshes), []
        for lo in range(0, len(ids), MAX_OBJECTS):
            part = ids[lo:lo + MAX_OBJECTS]
            p = self.pack(meshes, part)
            with contextlib.nullcontext() if host else torch.cuda.device(self.device):
                d = self._arrays(p, len(part), K, None if host else self.device)
                self.launch(d, len(part), p["total"], K, None if host else torch.cuda.current_stream(self.device).cuda_stream)
                parts.append(dict({k: twin.array(d[k], None) for k in self._outputs(0, K)}, counts=p["counts"]))   # a download synchronises
        if not parts:
            return dict(self._outputs(0, K), counts=np.zeros(0, np.int32))
        return {k: np.concatenate([part[k] for part in parts]) for k in parts[0]}

    def _arrays(self, p: Dict[str, np.ndarray], objects: int, K: int, device) -> Dict[str, object]:
        """the packed inputs, zeroed outputs and the workspace where the call runs: tensors on `device`, or NumPy arrays"""
        size = max(int(self.lib.cp_model_prep_workspace_bytes(objects, p["total"])), 8)
        d = {k: twin.array(p[k], p[k].dtype, device) for k in ("verts", "offsets", "counts")}
        return dict(d, **self._outputs(objects, K, device), **twin.alloc(dict(workspace=((size,), np.uint8)), device))

    def upload(self, p: Dict[str, np.ndarray], objects: int, K: int) -> Dict[str, object]:
        """the packed inputs, zeroed outputs and the workspace as device tensors"""
        return self._arrays(p, objects, K, self.device)

    def launch(self, d: Dict[str, object], objects: int, total: int, K: int, stream: Optional[int]):
        """one cp_model_prep_f32 call on `upload`'s tensors (tools/model_prep_times.py times this); stream None: the host twin on NumPy arrays"""
        twin.call("cp_model_prep_f32", d["verts"], total, d["offsets"], d["counts"], objects, K, d["diameter_sq"], d["box"], d["keypoints"],
                  d["indices"], d["status"], d["workspace"], len(d["workspace"]), host=stream is None, stream=stream)

    def prepare(self, meshes: Dict[object, np.ndarray], no_points: int = 9) -> Dict[object, dict]:
        return self._results(list(meshes), self.outputs(meshes, no_points, host=False))

    def prepare_host(self, meshes: Dict[object, np.ndarray], no_points: int = 9) -> Dict[object, dict]:
        return self._results(list(meshes), self.outputs(meshes, no_points, host=True))

    def run(self, meshes: Dict[object, np.ndarray], no_points: int = 9, renderer: str = "device") -> Dict[object, dict]:
        """`renderer` as in the converter's settings: "device" or "host", never one for the other"""
        if renderer not in ("device", "host"):
            raise ValueError("renderer must be 'device' or 'host' (got %r)" % (renderer,))
        return self.prepare(meshes, no_points) if renderer == "device" else self.prepare_host(meshes, no_points)


def model_prep_for(renderer: str) -> ModelPrep:
    """the ModelPrep of a converter run: "device" needs a GPU, "host" builds the twin"""
    if renderer not in ("device", "host"):
        raise ValueError("settings['renderer'] must be 'device' or 'host' (got %r)" % (renderer,))
    if renderer == "host":
        return ModelPrep(None)
    import torch

    if not torch.cuda.is_available():
        raise _lib.CasaposeHipError("generating keypoints or models_info on the device needs a ROCm GPU; renderer = 'host' asks for the serial host "
                                    "twin instead")
    return ModelPrep(torch.device("cuda", torch.cuda.current_device()))


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
def write_keypoints_ply(path, keypoints) -> None:
    """The ASCII layout of the reference's keypoint files.  %.9g prints a float32 with enough digits to read back to the same float32."""
    kp = np.asarray(keypoints, np.float32).reshape(-1, 3)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(kp))
        for p in kp:
            f.write("%.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])))


def _existing_entry(existing: Optional[dict], stem: str) -> dict:
    if not existing:
        return {}
    if stem in existing:
        return existing[stem]
    digits = re.findall(r"\d+", stem)
    if digits:
        for key in (str(int(digits[0])), int(digits[0])):
            if key in existing:
                return existing[key]
    return {}


def write_models_info(path, results: Dict[str, dict], existing: Optional[dict] = None) -> dict:
    """models_info.json keyed by the mesh file's stem (what VectorfieldDataset looks up): BOP's diameter, min_x/y/z and size_x/y/z from
    `results` ({stem: a ModelPrep result}); every other field of the object's entry in `existing` (found under the stem or under BOP's integer
    key) is carried over.  Returns what it wrote."""
    info = {}
    for stem, r in results.items():
        entry = {"diameter": float(r["diameter"])}
        for a, axis in enumerate("xyz"):
            entry["min_" + axis] = float(r["min"][a])
        for a, axis in enumerate("xyz"):
            entry["size_" + axis] = float(r["size"][a])
        for key, value in _existing_entry(existing, str(stem)).items():
            entry.setdefault(key, value)
        info[str(stem)] = entry
    with open(path, "w") as f:
        json.dump(info, f, indent=2)
    return info


def find_meshes(folder: str) -> Dict[str, str]:
    """{stem: mesh file} of a model folder in BOP's flat layout (<folder>/<stem>.ply, else .obj) or the reader's (<folder>/<stem>/<stem>.obj, else
    .ply); *_keypoints.ply files are no meshes"""
    found = {}
    for name in sorted(os.listdir(folder)):
        full = os.path.join(folder, name)
        stem, ext = os.path.splitext(name)
        if os.path.isdir(full):
            for e in (".obj", ".ply"):
                if os.path.isfile(os.path.join(full, name + e)):
                    found.setdefault(name, os.path.join(full, name + e))
                    break
        elif ext.lower() == ".ply" and not stem.endswith("keypoints"):
            found[stem] = full
    if not found:
        found = {os.path.splitext(n)[0]: os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.lower().endswith(".obj")}
    return found


__all__ = ["ModelPrep", "model_prep_for", "write_keypoints_ply", "write_models_info", "find_meshes"]
