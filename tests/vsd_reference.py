"""BOP's Visible Surface Discrepancy in fp64 NumPy, written from the definitions (Hodan et al., BOP Challenge 2019/2020: VSD with the BOP19
visibility masks and the step cost), not from csrc/vsd_math.h.

  distance image  dist = sqrt((x d / fx)^2 + (y d / fy)^2 + d^2) with x = j - cx, y = i - cy for depth d at pixel (row i, column j)
  visibility      V_g = {D_g hit and (D_t missing or dist_g - dist_t <= delta)};  V_e likewise, plus the pixels of V_g the estimate hits
  cost            c = |dist_g - dist_e| / diameter on V_g & V_e, step: 1 where c >= tau
  error           e(tau) = (|{c >= tau}| + |V_g u V_e| - |V_g & V_e|) / |V_g u V_e|, 1 where the union is empty

The rendered depths are the planes cp_render_masks_host_u8 leaves in its workspace: existing tests hold that twin equal to
tests/raster_reference.py and to the device byte for byte.  A sensor depth that is not > 0 is missing.

Besides the integers, `pair_counts` returns the number of *undecided* pixels: those with a comparison whose two sides are within 1e-9 mm (against
delta, or against tau * diameter) or within 1e-12 after the division by the diameter.  The device's z * c and the formula above differ by a few
fp64 ulps, about 1e-13 mm at one metre, so every other pixel must be decided alike."""
import numpy as np

EMPTY = 0xFFFFFFFF
DELTA = 15.0
TAUS = [0.05 * i for i in range(1, 11)]
THETAS = [0.05 * i for i in range(1, 11)]
MM_MARGIN, RATIO_MARGIN = 1e-9, 1e-12


def render_planes(renderer, frames, H, W, near, far, sample_offset=0.0):
    """(planes uint32 [frames, instances_max, H, W], records int32 [frames, instances_max, 11]) of the renderer's host twin.  The twin clears
    only the planes of a frame's own instances, so the workspace starts as EMPTY."""
    p = renderer.pack(frames)
    n, imax = len(frames), p["inst_obj"].shape[1]
    size = int(renderer.lib.cp_render_masks_workspace_bytes(n, imax, H, W))
    workspace = np.full(size // 4, EMPTY, np.uint32)
    _, records = renderer._render((renderer.verts, renderer.vert_counts, renderer.faces, renderer.face_counts), p, n, H, W, near, far, sample_offset,
                                  workspace, size, None, None)
    return workspace.reshape(n, imax, H, W), records


def distance_image(depth, cam):
    fx, fy, cx, cy = (float(c) for c in cam)
    H, W = depth.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = depth.astype(np.float64)
    return np.sqrt(((x - cx) * d / fx) ** 2 + ((y - cy) * d / fy) ** 2 + d ** 2)


def plane_depth(plane):
    hit = plane != EMPTY
    return hit, np.where(hit, plane.view(np.float32).astype(np.float64), 0.0)


def pair_counts(plane_e, plane_g, sensor, cam, diameter, delta=DELTA, taus=TAUS):
    """-> (int64 [2 + ntau]: union, intersection, per tau the intersection pixels with cost >= tau; the number of undecided pixels)"""
    hit_e, z_e = plane_depth(np.ascontiguousarray(plane_e))
    hit_g, z_g = plane_depth(np.ascontiguousarray(plane_g))
    sensor = np.asarray(sensor, np.float32)
    valid = sensor > 0
    d_e, d_g, d_t = distance_image(z_e, cam), distance_image(z_g, cam), distance_image(np.where(valid, sensor, 0).astype(np.float64), cam)
    vis_g = hit_g & (~valid | (d_g - d_t <= delta))
    vis_e = hit_e & (~valid | (d_e - d_t <= delta) | vis_g)
    inter, union = vis_g & vis_e, vis_g | vis_e
    diff = np.abs(d_g - d_e)
    cost = diff / diameter
    counts = [union.sum(), inter.sum()] + [(inter & (cost >= tau)).sum() for tau in taus]
    undecided = (hit_g & valid & (np.abs((d_g - d_t) - delta) <= MM_MARGIN)) | (hit_e & valid & (np.abs((d_e - d_t) - delta) <= MM_MARGIN))
    for tau in taus:
        undecided |= hit_e & hit_g & ((np.abs(diff - tau * diameter) <= MM_MARGIN) | (np.abs(cost - tau) <= RATIO_MARGIN))
    return np.asarray(counts, np.int64), int(undecided.sum())


def errors_of(counts):
    """float64 [ntau] from one pair's integers"""
    c = [int(x) for x in counts]
    return np.array([1.0 if c[0] == 0 else (c[2 + k] + c[0] - c[1]) / c[0] for k in range(len(c) - 2)])


class Scene:
    """Meshes [(vertices, faces)] and a cache of host renders keyed by (object, pose, camera, size): `counts` gives a pair's integers."""

    def __init__(self, meshes, near, far, sample_offset=0.0):
        from casapose_amd.data_handler.bop_converter import MaskRenderer

        self.renderer = MaskRenderer(None, {i: m for i, m in enumerate(meshes)})
        self.near, self.far, self.sample_offset = near, far, sample_offset
        self.cache = {}

    def plane(self, obj, pose, cam, H, W):
        pose = np.asarray(pose, np.float64).reshape(3, 4)
        key = (int(obj), pose.tobytes(), tuple(float(c) for c in cam), H, W)
        if key not in self.cache:
            planes, _ = render_planes(self.renderer, [dict(cam=cam, instances=[(int(obj), 1, pose)])], H, W, self.near, self.far, self.sample_offset)
            self.cache[key] = planes[0, 0].copy()
        return self.cache[key]

    def counts(self, obj, est, gt, cam, sensor, diameter, delta=DELTA, taus=TAUS):
        H, W = sensor.shape
        return pair_counts(self.plane(obj, est, cam, H, W), self.plane(obj, gt, cam, H, W), sensor, cam, diameter, delta, taus)


def check_counts(got, want, undecided, where=""):
    """The gate: where a pair has no undecided pixel all its integers are equal, elsewhere each lies within +- the undecided pixels; at most 2 %
    of the pairs may have undecided pixels.  -> the number of pairs with undecided pixels"""
    got, want, undecided = np.asarray(got, np.int64), np.asarray(want, np.int64), np.asarray(undecided, np.int64)
    assert got.shape == want.shape and len(undecided) == len(want), (where, got.shape, want.shape)
    loose = undecided > 0
    assert loose.sum() <= 0.02 * len(want), "%s: %d of %d pairs have undecided pixels" % (where, loose.sum(), len(want))
    assert np.array_equal(got[~loose], want[~loose]), "%s: first differing pair %s" % (where, np.argwhere((got != want).any(axis=1) & ~loose)[:3].tolist())
    assert (np.abs(got[loose] - want[loose]) <= undecided[loose, None]).all(), where
    return int(loose.sum())


def count_matches(err, thr):
    used, n = set(), 0
    for row in err:
        best, bj = np.inf, None
        for j, e in enumerate(row):
            if j not in used and e < best:
                best, bj = e, j
        if bj is not None and best < thr:
            used.add(bj)
            n += 1
    return n


def recall(groups, ntau=10):
    """groups [(obj, targets, e [estimates, instances, ntau])] -> {"AR_VSD", "recall_vsd" [tau][theta], "targets", "objects": {...}}"""
    total, hit = {}, {}
    for obj, count, e in groups:
        total[obj] = total.get(obj, 0) + count
        h = hit.setdefault(obj, np.zeros((ntau, len(THETAS))))
        for t in range(ntau):
            for i, theta in enumerate(THETAS):
                h[t, i] += count_matches(np.asarray(e)[:, :, t] if np.size(e) else [], theta)

    def entry(n, h):
        rec = (h / n).tolist()
        return {"targets": n, "recall_vsd": rec, "AR_VSD": sum(sum(row) for row in rec) / float(ntau * len(THETAS))}

    out = entry(sum(total.values()), sum(hit.values()))
    out["objects"] = {str(o): entry(total[o], hit[o]) for o in sorted(total)}
    return out
