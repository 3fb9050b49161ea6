"""fp64 NumPy restatement of the BOP scores (MSSD and MSPD with object symmetries, targets, matching, recall), written from the definitions and
importing nothing from casapose_amd.  The tests feed it the same fp32-rounded inputs as the device.

    e_MSSD = min_S max_x |P^ x - P_ S x|,   e_MSPD = min_S max_x |proj_K(P^ x) - proj_K(P_ S x)|
"""
import math

import numpy as np


def symmetry_set(entry, step=0.01):
    """[S, 3, 4]: identity and the discrete transforms (D); with continuous entries, every c of C (n = ceil(pi / step) rotations about the
    normalised axis, t = offset - R offset) applied after every d of D, d-major."""
    D = [np.eye(4)]
    for m in entry.get("symmetries_discrete", []):
        d = np.eye(4)
        d[:3, :4] = np.asarray(m, np.float64).reshape(4, 4)[:3, :4]
        D.append(d)
    C = []
    n = int(math.ceil(math.pi / step))
    for sym in entry.get("symmetries_continuous", []):
        a = np.asarray(sym["axis"], np.float64)
        a = a / np.linalg.norm(a)
        off = np.asarray(sym["offset"], np.float64)
        A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        for k in range(n):
            th = 2.0 * math.pi * k / n
            c = np.eye(4)
            c[:3, :3] = np.eye(3) + math.sin(th) * A + (1.0 - math.cos(th)) * (A @ A)
            c[:3, 3] = off - c[:3, :3] @ off
            C.append(c)
    S = [c @ d for d in D for c in C] if C else D
    return np.stack(S)[:, :3, :]


def _project(K, cam):
    uvw = cam @ K.T
    w = uvw[..., 2:3]
    safe = np.where(w == 0, 1.0, w)
    return np.where(w == 0, 0.0, uvw[..., :2] / safe)


def per_symmetry_errors(mesh, est, gt, K, syms):
    """mesh [n, 3], est and gt [3, 4], K [3, 3], syms [S, 3, 4] -> (mssd [S], mspd [S], largest |camera coordinate|, smallest camera z)"""
    X, est, gt, K, syms = (np.asarray(a, np.float64) for a in (mesh, est, gt, K, syms))
    pe = X @ est[:, :3].T + est[:, 3]
    G = np.eye(4)
    G[:3] = gt
    e3, e2 = np.empty(len(syms)), np.empty(len(syms))
    big, zmin = np.abs(pe).max(), pe[:, 2].min()
    ue = _project(K, pe)
    for s, sym in enumerate(syms):
        S4 = np.eye(4)
        S4[:3] = sym
        M = (G @ S4)[:3]
        pg = X @ M[:, :3].T + M[:, 3]
        e3[s] = np.linalg.norm(pe - pg, axis=1).max()
        e2[s] = np.linalg.norm(ue - _project(K, pg), axis=1).max()
        big, zmin = max(big, np.abs(pg).max()), min(zmin, pg[:, 2].min())
    return e3, e2, big, zmin


def pair_errors(mesh, est, gt, K, syms):
    """-> (e_MSSD, e_MSPD); (+inf, +inf) for the zero pose (|sum of the 12 entries| < 1e-4)"""
    if abs(np.asarray(est, np.float64).sum()) < 1e-4:
        return np.inf, np.inf
    e3, e2, _, _ = per_symmetry_errors(mesh, est, gt, K, syms)
    return e3.min(), e2.min()


MSSD_T = [0.05 * i for i in range(1, 11)]
MSPD_T = [5.0 * i for i in range(1, 11)]


def targets_of(gts, targets=None):
    """{(scene, im, obj): (count, [instance indices])}; gts {(scene, im): [{"id", "R", "t", optional "visib_fract"}]}"""
    out = {}
    if targets is not None:
        for t in targets:
            key = (t["scene_id"], t["im_id"], t["obj_id"])
            out[key] = (t["inst_count"], [i for i, g in enumerate(gts.get(key[:2], [])) if g["id"] == key[2]])
        return out
    for (scene, im), inst in gts.items():
        for i, g in enumerate(inst):
            if "visib_fract" in g and g["visib_fract"] < 0.1:
                continue
            c, l = out.get((scene, im, g["id"]), (0, []))
            out[(scene, im, g["id"])] = (c + 1, l + [i])
    return out


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


def score(rows, gts, cameras, meshes, syms, diameters, targets=None, image_width=640.0):
    """rows: [(scene, im, obj, score, pose [3, 4])] in file order; meshes, syms, diameters: {obj: ...} -> (dict of scores, [every pair's
    (obj, e_MSSD, e_MSPD)])"""
    want = targets_of(gts, targets)
    r = image_width / 640.0
    total, hit, pairs = {}, {}, []
    for key, (count, cand) in want.items():
        scene, im, obj = key
        mine = [x for x in rows if (x[0], x[1], x[2]) == key and x[3] != 0 and np.abs(x[4]).sum() != 0]
        order = sorted(range(len(mine)), key=lambda i: (-mine[i][3], i))[:count]
        e3 = np.empty((len(order), len(cand)))
        e2 = np.empty((len(order), len(cand)))
        for a, i in enumerate(order):
            for b, j in enumerate(cand):
                g = gts[(scene, im)][j]
                G = np.hstack([np.asarray(g["R"], np.float64).reshape(3, 3), np.asarray(g["t"], np.float64).reshape(3, 1)])
                f = lambda p: np.asarray(p, np.float32).astype(np.float64)  # noqa: E731  (the device's inputs are fp32)
                e3[a, b], e2[a, b] = pair_errors(f(meshes[obj]), f(mine[i][4]), f(G), f(cameras[(scene, im)]), f(syms[obj]))
                pairs.append((obj, e3[a, b], e2[a, b]))
        total[obj] = total.get(obj, 0) + count
        h = hit.setdefault(obj, np.zeros((2, 10)))
        for i in range(10):
            h[0, i] += count_matches(e3, MSSD_T[i] * diameters[obj])
            h[1, i] += count_matches(e2, MSPD_T[i] * r)

    def entry(n, h):
        rec = (h / n).tolist()
        a, b = sum(rec[0]) / 10.0, sum(rec[1]) / 10.0
        return {"targets": n, "recall_mssd": rec[0], "recall_mspd": rec[1], "AR_MSSD": a, "AR_MSPD": b, "AR_MSSD_MSPD": 0.5 * (a + b)}

    out = entry(sum(total.values()), sum(hit.values()))
    out["objects"] = {str(o): entry(total[o], hit[o]) for o in sorted(total)}
    return out, pairs
