"""Reference for the shaded mesh renderer (csrc/shade.hip, csrc/shade_math.h); a helper, not a test module.

render_shaded_reference   rules 2-6 and 8 of shade_math.h restated in NumPy int64 / fp64 from their specification, on top of raster_reference.py
                          (which restates rules 1-6 of mask_math.h): one 64-bit key per pixel (depth bits, instance, triangle; the smallest
                          wins), perspective-correct vertex colours from the winning triangle's edge functions, the flat two-sided face
                          normal from the camera points, s = ambient + diffuse * max(0, n . l), the supplied or the procedural background,
                          clip(., 0, 1) * 2 - 1 rounded once to fp32.  No noise: rule 7 is the device's and the twin's Philox stream.

A scene is raster_reference's; colors = per mesh uint8 [V, 3] or None for all; flat = fp32 [meshes, 3]; lights = fp64 [frames, 8]."""
import numpy as np

import raster_reference as RR

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys_reference(meshes, frames, H, W, near, far, sample_offset):
    """uint64 [F, H, W] and the dropped triangles int32 [F]"""
    S = int(np.rint(256.0 * sample_offset))
    keys = np.full((len(frames), H, W), EMPTY, np.uint64)
    dropped = np.zeros(len(frames), np.int32)
    for f, frame in enumerate(frames):
        for k, (obj, label, pose) in enumerate(frame["instances"]):
            verts, faces = meshes[obj]
            U, V, Z, ok = RR.snapped(verts, pose, frame["cam"], near)
            for t, (a, b, c) in enumerate(np.asarray(faces).tolist()):
                if min(a, b, c) < 0 or max(a, b, c) >= len(verts) or not (ok[a] and ok[b] and ok[c]):
                    dropped[f] += 1
                    continue
                xs, ys, zs = [int(U[i]) for i in (a, b, c)], [int(V[i]) for i in (a, b, c)], [float(Z[i]) for i in (a, b, c)]
                j0, j1 = max(0, -((S - min(xs)) // 256)), min(W - 1, (max(xs) - S) // 256)
                i0, i1 = max(0, -((S - min(ys)) // 256)), min(H - 1, (max(ys) - S) // 256)
                if j0 > j1 or i0 > i1:
                    continue
                px = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + S)[None, :]
                py = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + S)[:, None]
                E = [(xs[q] - xs[p]) * (py - ys[p]) - (ys[q] - ys[p]) * (px - xs[p]) for p, q in ((1, 2), (2, 0), (0, 1))]
                A = E[0] + E[1] + E[2]
                cover = (A != 0) & (((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)))
                with np.errstate(all="ignore"):
                    z = A.astype(np.float64) / ((E[0].astype(np.float64) / zs[0] + E[1].astype(np.float64) / zs[1]) + E[2].astype(np.float64) / zs[2])
                    zf = z.astype(np.float32)
                    keep = cover & (zf.astype(np.float64) >= near) & (zf.astype(np.float64) <= far)
                key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64((k << 24) | t)
                sub = keys[f, i0:i1 + 1, j0:j1 + 1]
                sub[keep] = np.minimum(sub[keep], key[keep])
    return keys, dropped


def render_shaded_reference(meshes, colors, flat, frames, lights, H, W, near, far, sample_offset, background=None):
    """dict(keys uint64, label uint8, depth fp32, dropped int32, img fp32 [F, H, W, 3], albedo and shade fp64 (0 on background))"""
    S = int(np.rint(256.0 * sample_offset))
    keys, dropped = keys_reference(meshes, frames, H, W, near, far, sample_offset)
    F = len(frames)
    label, depth = np.zeros((F, H, W), np.uint8), np.zeros((F, H, W), np.float32)
    albedo, shade, value = np.zeros((F, H, W, 3)), np.zeros((F, H, W)), np.zeros((F, H, W, 3))
    lights = np.asarray(lights, np.float64).reshape(F, 8)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for f, frame in enumerate(frames):
        l, ambient, diffuse, crop_row, crop_col = lights[f, 0:3], lights[f, 3], lights[f, 4], lights[f, 6], lights[f, 7]
        if background is not None:
            value[f] = np.asarray(background, np.uint8).reshape(F, H, W, 3)[f].astype(np.float64) / 255.0
        else:
            xs, ys = (jj + crop_col) + 0.5, (ii + crop_row) + 0.5
            value[f] = (0.35 + (0.1 * np.sin(xs / 37.0)) * np.cos(ys / 53.0))[..., None]
        hit = keys[f] != EMPTY
        depth[f][hit] = (keys[f][hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        for word in np.unique(keys[f][hit] & np.uint64(0xFFFFFFFF)).tolist():
            k, t = int(word) >> 24, int(word) & 0xFFFFFF
            obj, lab, pose = frame["instances"][k]
            verts, faces = meshes[obj]
            a, b, c = (int(v) for v in faces[t])
            U, V, Z, _ = RR.snapped(verts, pose, frame["cam"], near)
            X, Y, Zc = RR.camera_points(verts, pose)
            at = hit & ((keys[f] & np.uint64(0xFFFFFFFF)) == np.uint64(word))
            i, j = np.nonzero(at)
            px, py = 256 * j.astype(np.int64) + S, 256 * i.astype(np.int64) + S
            xs, ys = [int(U[n]) for n in (a, b, c)], [int(V[n]) for n in (a, b, c)]
            E = [(xs[q] - xs[p]) * (py - ys[p]) - (ys[q] - ys[p]) * (px - xs[p]) for p, q in ((1, 2), (2, 0), (0, 1))]
            q = [E[n].astype(np.float64) / float(Z[v]) for n, v in enumerate((a, b, c))]
            total = (q[0] + q[1]) + q[2]
            lam = [q[n] / total for n in range(3)]
            if colors is not None:
                col = [colors[obj][v].astype(np.float64) / 255.0 for v in (a, b, c)]
                alb = (lam[0][:, None] * col[0][None] + lam[1][:, None] * col[1][None]) + lam[2][:, None] * col[2][None]
            else:
                alb = np.broadcast_to(np.asarray(flat, np.float32)[obj].astype(np.float64), (len(i), 3))
            P = [np.array([X[v], Y[v], Zc[v]]) for v in (a, b, c)]
            e1, e2 = P[1] - P[0], P[2] - P[0]
            n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            ndl = 0.0
            if length > 0:
                n = n / length
                if (n[0] * P[0][0] + n[1] * P[0][1]) + n[2] * P[0][2] > 0:
                    n = -n
                ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2]
            s = ambient + diffuse * max(ndl, 0.0)
            albedo[f][at], shade[f][at], label[f][at] = alb, s, lab
            value[f][at] = alb * s
    img = (np.clip(value, 0.0, 1.0) * 2.0 - 1.0).astype(np.float32)
    return dict(keys=keys, label=label, depth=depth, dropped=dropped, img=img, albedo=albedo, shade=shade)
