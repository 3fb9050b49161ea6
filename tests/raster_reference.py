"""References for the mask renderer (csrc/masks.hip, csrc/mask_math.h); a helper, not a test module.

render_reference   the renderer's eight rules restated in NumPy int64 / fp64 from their specification (not from the header): camera points with
                   the sums in a fixed order, vertices snapped to 1/256 pixel, exact integer edge functions with closed edges and both
                   windings, fp64 perspective depth rounded once to fp32, near-plane triangles dropped whole, arg-min over the instances with the
                   lowest index on a tie, counts and boxes.  One addition completes rule 6 so that int64 never overflows: a vertex whose
                   |256 u| or |256 v| exceeds 2^28 drops its triangle as well.
ray_cast           an independent un-snapped fp64 ray / triangle intersector (Moller-Trumbore, nearest hit) per pixel sample.
edge_band          the pixels an un-snapped and a snapped rasteriser may disagree on: within 2/256 px of a projected edge line.
icosphere          the test mesh: an icosahedron subdivided n times onto the unit sphere (20 * 4^n triangles, outward winding).

A scene is (meshes, frames, H, W, near, far): meshes = [(vertices fp32 [V, 3], faces int32 [T, 3])], a frame = dict(cam=(fx, fy, cx, cy),
instances=[(mesh index, label, pose [3, 4])])."""
import numpy as np

RECORD = 11   # px_count_all, px_count_visib, bbox_obj (x, y, w, h), bbox_visib (x, y, w, h), dropped_triangles


def icosphere(subdivisions):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        cache, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                cache[key] = len(verts) - 1
            return cache[key]

        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts, np.float64), np.array(faces, np.int32)


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def pose_at(cam, u, v, z, R=None):
    """[3, 4]: rotation R, the model origin projecting to pixel coordinate (u, v) at depth z"""
    fx, fy, cx, cy = cam
    return np.concatenate([np.eye(3) if R is None else R, np.array([[(u - cx) * z / fx], [(v - cy) * z / fy], [z]])], axis=1)


# ---- rule 1 and 2 -----------------------------------------------------------------------------------------------------------------------
def camera_points(verts, pose):
    x, y, z = (np.asarray(verts, np.float32).astype(np.float64)[:, c] for c in range(3))
    P = np.asarray(pose, np.float64)
    return tuple(((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3))


def snapped(verts, pose, cam, near):
    """(U, V int64, Z, ok): ok is False for a vertex that drops its triangles"""
    fx, fy, cx, cy = (float(c) for c in cam)
    X, Y, Z = camera_points(verts, pose)
    with np.errstate(all="ignore"):
        ok = Z >= near
        Zs = np.where(ok, Z, 1.0)
        su, sv = 256.0 * ((fx * X) / Zs + cx), 256.0 * ((fy * Y) / Zs + cy)
        ok = ok & (np.abs(su) <= 2.0 ** 28) & (np.abs(sv) <= 2.0 ** 28)
        U = np.rint(np.where(ok, su, 0.0)).astype(np.int64)
        V = np.rint(np.where(ok, sv, 0.0)).astype(np.int64)
    return U, V, Z, ok


def _box(mask):
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return [-1, -1, -1, -1]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]


def render_reference(meshes, frames, H, W, near, far, sample_offset):
    """(labels uint8 [F, H, W], records int32 [F, max(1, most instances), 11])"""
    S = int(np.rint(256.0 * sample_offset))
    imax = max([1] + [len(f["instances"]) for f in frames])
    labels = np.zeros((len(frames), H, W), np.uint8)
    records = np.zeros((len(frames), imax, RECORD), np.int32)
    records[:, :, 2:10] = -1
    for f, frame in enumerate(frames):
        n = len(frame["instances"])
        depth = np.full((n + 1, H, W), np.inf, np.float32)   # plane n: the background, so that the arg-min exists for n = 0
        for k, (obj, label, pose) in enumerate(frame["instances"]):
            verts, faces = meshes[obj]
            U, V, Z, ok = snapped(verts, pose, frame["cam"], near)
            for a, b, c in np.asarray(faces).tolist():
                if min(a, b, c) < 0 or max(a, b, c) >= len(verts) or not (ok[a] and ok[b] and ok[c]):
                    records[f, k, 10] += 1
                    continue
                xs, ys, zs = [int(U[i]) for i in (a, b, c)], [int(V[i]) for i in (a, b, c)], [float(Z[i]) for i in (a, b, c)]
                j0, j1 = max(0, -((S - min(xs)) // 256)), min(W - 1, (max(xs) - S) // 256)   # ceil and floor of (x - S) / 256
                i0, i1 = max(0, -((S - min(ys)) // 256)), min(H - 1, (max(ys) - S) // 256)
                if j0 > j1 or i0 > i1:
                    continue
                px = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + S)[None, :]
                py = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + S)[:, None]
                E = []
                for p, q in ((1, 2), (2, 0), (0, 1)):
                    E.append((xs[q] - xs[p]) * (py - ys[p]) - (ys[q] - ys[p]) * (px - xs[p]))
                A = E[0] + E[1] + E[2]
                cover = (A != 0) & (((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)))
                with np.errstate(all="ignore"):
                    z = A.astype(np.float64) / ((E[0].astype(np.float64) / zs[0] + E[1].astype(np.float64) / zs[1]) + E[2].astype(np.float64) / zs[2])
                    zf = z.astype(np.float32)
                    keep = cover & (zf.astype(np.float64) >= near) & (zf.astype(np.float64) <= far)
                sub = depth[k, i0:i1 + 1, j0:j1 + 1]
                sub[keep] = np.minimum(sub[keep], zf[keep])
        winner = np.argmin(depth, axis=0)   # the first of equal minima: the lowest instance index, the background only where nothing was hit
        for k, (obj, label, pose) in enumerate(frame["instances"]):
            own = np.isfinite(depth[k])
            visible = own & (winner == k)
            labels[f][visible] = label
            records[f, k, 0], records[f, k, 1] = own.sum(), visible.sum()
            records[f, k, 2:6], records[f, k, 6:10] = _box(own), _box(visible)
    return labels, records


# ---- the independent ray caster ------------------------------------------------------------------------------------------------------------
def ray_cast(meshes, frame, H, W, near, far, sample_offset):
    """(label uint8 [H, W], depths fp64 [instances, H, W] with inf where an instance is not hit): per pixel the nearest Moller-Trumbore hit of
    the ray through its sample point, nothing snapped, nothing dropped (a hit outside [near, far] is no hit)."""
    fx, fy, cx, cy = (float(c) for c in frame["cam"])
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(jj + sample_offset - cx) / fx, (ii + sample_offset - cy) / fy, np.ones_like(jj)], axis=-1).reshape(-1, 1, 3)   # [P, 1, 3]
    depths = np.full((len(frame["instances"]), H * W), np.inf)
    for k, (obj, label, pose) in enumerate(frame["instances"]):
        verts, faces = meshes[obj]
        cam = np.stack(camera_points(verts, pose), axis=1)
        v0, v1, v2 = (cam[np.asarray(faces)[:, c]] for c in range(3))
        e1, e2 = (v1 - v0)[None], (v2 - v0)[None]          # [1, T, 3]
        with np.errstate(all="ignore"):
            pvec = np.cross(d, e2)
            det = (e1 * pvec).sum(-1)
            tvec = -v0[None]                                  # the ray starts at the camera centre
            u = (tvec * pvec).sum(-1) / det
            qvec = np.cross(tvec, e1)
            v = (d * qvec).sum(-1) / det
            t = (e2 * qvec).sum(-1) / det
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= near) & (t <= far)
        depths[k] = np.where(hit, t, np.inf).min(axis=1)
    depths = depths.reshape(-1, H, W)
    label = np.zeros((H, W), np.uint8)
    if len(depths):
        winner, any_hit = np.argmin(depths, axis=0), np.isfinite(depths).any(axis=0)
        label = np.where(any_hit, np.array([lab for _, lab, _ in frame["instances"]], np.uint8)[winner], 0).astype(np.uint8)
    return label, depths


def edge_band(meshes, frame, H, W, near, sample_offset, band=2.0 / 256.0, grow=4.0 / 256.0):
    """bool [H, W]: True where the pixel's sample lies closer than `band` px to a projected edge line of a triangle whose snapped bounding box,
    grown by `grow` px, contains the sample"""
    out = np.zeros((H, W), bool)
    fx, fy, cx, cy = (float(c) for c in frame["cam"])
    for obj, label, pose in frame["instances"]:
        verts, faces = meshes[obj]
        X, Y, Z = camera_points(verts, pose)
        U, V, _, ok = snapped(verts, pose, frame["cam"], near)
        with np.errstate(all="ignore"):
            pu, pv = fx * X / Z + cx, fy * Y / Z + cy
        for tri in np.asarray(faces).tolist():
            if not all(ok[i] for i in tri):
                continue
            lo_x, hi_x = min(U[i] for i in tri) / 256.0 - grow, max(U[i] for i in tri) / 256.0 + grow
            lo_y, hi_y = min(V[i] for i in tri) / 256.0 - grow, max(V[i] for i in tri) / 256.0 + grow
            j0, j1 = max(0, int(np.ceil(lo_x - sample_offset))), min(W - 1, int(np.floor(hi_x - sample_offset)))
            i0, i1 = max(0, int(np.ceil(lo_y - sample_offset))), min(H - 1, int(np.floor(hi_y - sample_offset)))
            if j0 > j1 or i0 > i1:
                continue
            sx = (np.arange(j0, j1 + 1) + sample_offset)[None, :]
            sy = (np.arange(i0, i1 + 1) + sample_offset)[:, None]
            for p, q in ((0, 1), (1, 2), (2, 0)):
                ax, ay, bx, by = pu[tri[p]], pv[tri[p]], pu[tri[q]], pv[tri[q]]
                length = np.hypot(bx - ax, by - ay)
                if length == 0:
                    dist = np.hypot(sx - ax, sy - ay)
                else:
                    dist = np.abs((bx - ax) * (sy - ay) - (by - ay) * (sx - ax)) / length
                out[i0:i1 + 1, j0:j1 + 1] |= dist < band
    return out
