"""Contour alignment against a label map in NumPy / SciPy, written from the method's definition, not from csrc/contour_math.h.

The field of a job (label map `labels` [H, W], label l, gate G in whole pixels):
  seeds: pixels of label l with a 4-neighbour inside the image whose label is 0 (another object's label -- an occlusion edge -- and the image
  border make none);  D2 = min(rint(distance_transform_edt(~seeds)^2), G G + 1), G G + 1 everywhere without seeds.
The step, for a rendered depth plane z (the planes cp_render_masks_host_u8 leaves behind, through tests/vsd_reference.py):
  a pixel (x, y) in [1, W-2] x [1, H-2] is a contour pixel when it is hit and one of its four neighbours is not; it is used when z > 0 and D2
  at it and at its four neighbours is <= G G;  e = ((D2(x+1, y) - D2(x-1, y)) / 4, (D2(x, y+1) - D2(x, y-1)) / 4);
  p = ((x + o - cx) z / fx, (y + o - cy) z / fy, z) with o the sample offset the plane was rendered at;  Jpi = [[fx / Z, 0, -fx X / Z^2], [0, fy / Z, -fy Y / Z^2]];  J = Jpi [-[p]x | I];  g = J^T e
  A = sum g g^T / (e . e), b = -sum g over the pixels with e != 0, by plain numpy sums; (A + damping diag(A)) xi = b by numpy.linalg.solve;
  the update, the statuses, the loop and the keep rule are tests/icp_reference.py's."""
import numpy as np
from scipy import ndimage

import icp_reference as IR
import vsd_reference as VR

OK, FEW, SINGULAR, REFUSED, LOST_PIXELS, RMS_ROSE = range(6)
GATE, MIN_PIXELS, DAMPING, ITERATIONS = 3, 24, 1e-6, 8      # the defaults of DeviceMaskRefiner.refine


def seeds_of(labels, l):
    lab = np.asarray(labels)
    H, W = lab.shape
    zero = np.zeros((H + 2, W + 2), bool)
    zero[1:-1, 1:-1] = lab == 0                      # outside the image: not background
    near = zero[1:-1, :-2] | zero[1:-1, 2:] | zero[:-2, 1:-1] | zero[2:, 1:-1]
    return (lab == l) & near


def field(labels, l, G):
    """uint16 [H, W]"""
    seeds = seeds_of(labels, l)
    if not seeds.any():
        return np.full(seeds.shape, G * G + 1, np.uint16)
    d = ndimage.distance_transform_edt(~seeds)
    return np.minimum(np.rint(d ** 2), G * G + 1).astype(np.uint16)


def skew(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def terms(plane, d2, cam, G, offset=0.5):
    """the contour pixels of one plane -> (g [N, 6], ee [N] of the used pixels in row-major order, the number of contour pixels)"""
    fx, fy, cx, cy = (float(c) for c in cam)
    H, W = plane.shape
    hit, z = VR.plane_depth(np.ascontiguousarray(plane))
    D = np.asarray(d2).astype(np.int64)
    inner = np.zeros((H, W), bool)
    inner[1:H - 1, 1:W - 1] = True
    sh = lambda a, dy, dx: np.roll(a, (-dy, -dx), axis=(0, 1))   # noqa: E731  a[y + dy, x + dx]; the wrap only reaches border pixels
    contour = inner & hit & ~(sh(hit, 0, -1) & sh(hit, 0, 1) & sh(hit, -1, 0) & sh(hit, 1, 0))
    near = (D <= G * G) & (sh(D, 0, -1) <= G * G) & (sh(D, 0, 1) <= G * G) & (sh(D, -1, 0) <= G * G) & (sh(D, 1, 0) <= G * G)
    ys, xs = np.nonzero(contour & near & (z > 0))
    g, ee = np.zeros((len(ys), 6)), np.zeros(len(ys))
    for i, (y, x) in enumerate(zip(ys, xs)):
        e = np.array([(D[y, x + 1] - D[y, x - 1]) / 4.0, (D[y + 1, x] - D[y - 1, x]) / 4.0])
        Z = z[y, x]
        p = np.array([(x + offset - cx) * Z / fx, (y + offset - cy) * Z / fy, Z])
        Jpi = np.array([[fx / Z, 0.0, -fx * p[0] / Z ** 2], [0.0, fy / Z, -fy * p[1] / Z ** 2]])
        J = Jpi @ np.hstack([-skew(p), np.eye(3)])
        g[i], ee[i] = J.T @ e, e @ e
    return g, ee, int(contour.sum())


def sums(g, ee, contour):
    """-> dict: count (used), contour, A [6, 6], b [6], see, and the sums of the terms' magnitudes absA, absb"""
    nz = ee > 0
    gg = g[nz, :, None] * g[nz, None, :] / ee[nz, None, None]
    return dict(count=len(ee), contour=contour, A=gg.sum(0), b=-g[nz].sum(0), rr=float(ee.sum()), absA=np.abs(gg).sum(0), absb=np.abs(g[nz]).sum(0))


def step(plane, d2, cam, pose, G, damping=DAMPING, min_pixels=MIN_PIXELS, offset=0.5):
    """one step from a rendered plane -> (status, new pose (the old one unless OK), stats [used, rms, contour, see], sums)"""
    s = sums(*terms(plane, d2, cam, G, offset))
    status, xi = IR.solve(s, damping, min_pixels)
    rms = float(np.sqrt(s["rr"] / s["count"])) if s["count"] else 0.0
    stats = np.array([s["count"], rms, s["contour"], s["rr"]])
    if status != OK:
        return status, np.asarray(pose, np.float64).reshape(3, 4).copy(), stats, s
    return OK, IR.update(pose, xi), stats, s


def refine(scene, obj, pose, cam, d2, G=GATE, iterations=ITERATIONS, damping=DAMPING, min_pixels=MIN_PIXELS):
    """the loop and the keep / reject rule for one estimate; scene: a vsd_reference.Scene, d2: the field of the estimate's label
    -> (pose [3, 4], status, stats [iterations + 1, 4], the pose after the last step whatever the status)"""
    H, W = np.shape(d2)
    start = np.asarray(pose, np.float64).reshape(3, 4)
    cur, codes, stats = start.copy(), [], []
    for it in range(iterations + 1):
        code, new, st, _ = step(scene.plane(obj, cur, cam, H, W), d2, cam, cur, G, damping, min_pixels, scene.sample_offset)
        codes.append(code), stats.append(st)
        if it < iterations:
            cur = new
    stats = np.stack(stats)
    bad = [c for c in codes if c != OK]
    if bad:
        status = bad[0]
    elif stats[-1, 0] < max(float(min_pixels), stats[0, 0] / 2.0):
        status = LOST_PIXELS
    elif stats[-1, 1] > stats[0, 1]:
        status = RMS_ROSE
    else:
        status = OK
    return (cur if status == OK else start.copy()), status, stats, cur
