"""Projective point-to-plane ICP against a sensor depth image in fp64 NumPy, written from the method's definition, not from csrc/icp_math.h.

For a rendered depth plane z (the planes cp_render_masks_host_u8 leaves behind, through tests/vsd_reference.py) and the sensor depth d:
  a pixel (x, y) in [1, W-2] x [1, H-2] counts when z and its four neighbours are hit, |z_R - z_L| and |z_D - z_U| are below the jump,
  d > 0 and |d - z| is below the gate; p = ((x - cx) z / fx, (y - cy) z / fy, z), n = (p_R - p_L) x (p_D - p_U) normalised (length > 0),
  q = the back-projection at d, r = n . (q - p), J = (p x n, n)
  A = sum J J^T, b = sum J r by plain numpy sums; (A + damping diag(A)) xi = b by numpy.linalg.solve; xi = (omega, v)
  dR = the rotation of the unit quaternion (1, omega / 2) / |.|;  R <- dR R, t <- dR t + v
  a step fails with FEW below min_pixels pixels and with SINGULAR when the damped matrix is not positive definite
  loop: `iterations` steps, then one evaluation; the refined pose is kept only if every pass solved, the last pass used at least
  max(min_pixels, first-pass pixels / 2) pixels and its RMS residual is not above the first pass's."""
import numpy as np

import vsd_reference as VR

OK, FEW, SINGULAR, REFUSED, LOST_PIXELS, RMS_ROSE = range(6)


def terms(plane, sensor, cam, gate, jump):
    """the counted pixels of one plane -> (J [N, 6], r [N], ys, xs) in row-major pixel order; gate and jump in millimetres"""
    fx, fy, cx, cy = (float(c) for c in cam)
    H, W = plane.shape
    hit, z = VR.plane_depth(np.ascontiguousarray(plane))
    d = np.asarray(sensor, np.float32).astype(np.float64)
    inner = np.zeros((H, W), bool)
    inner[1:H - 1, 1:W - 1] = True
    sh = lambda a, dy, dx: np.roll(a, (-dy, -dx), axis=(0, 1))   # noqa: E731  a[y + dy, x + dx]; the wrap only reaches border pixels
    ok = inner & hit & sh(hit, 0, -1) & sh(hit, 0, 1) & sh(hit, -1, 0) & sh(hit, 1, 0)
    ok &= (np.abs(sh(z, 0, 1) - sh(z, 0, -1)) < jump) & (np.abs(sh(z, 1, 0) - sh(z, -1, 0)) < jump)
    with np.errstate(invalid="ignore"):
        ok &= (d > 0) & (np.abs(d - z) < gate)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    bp = lambda depth, dy, dx: np.stack([(xx + dx - cx) * sh(depth, dy, dx) / fx, (yy + dy - cy) * sh(depth, dy, dx) / fy, sh(depth, dy, dx)], -1)   # noqa: E731
    p = bp(z, 0, 0)
    n = np.cross(bp(z, 0, 1) - bp(z, 0, -1), bp(z, 1, 0) - bp(z, -1, 0))
    length = np.linalg.norm(n, axis=-1)
    ok &= length > 0
    ys, xs = np.nonzero(ok)
    p, n = p[ys, xs], n[ys, xs] / length[ys, xs, None]
    q = np.stack([(xs - cx) * d[ys, xs] / fx, (ys - cy) * d[ys, xs] / fy, d[ys, xs]], -1)
    r = np.einsum("ij,ij->i", n, q - p)
    return np.concatenate([np.cross(p, n), n], axis=1), r, ys, xs


def sums(J, r):
    """-> dict: count, A [6, 6], b [6], rr, and the sums of the terms' magnitudes absA, absb (what a summation bound scales with)"""
    JJ = J[:, :, None] * J[:, None, :]
    return dict(count=len(r), A=JJ.sum(0), b=(J * r[:, None]).sum(0), rr=float((r * r).sum()), absA=np.abs(JJ).sum(0),
                absb=np.abs(J * r[:, None]).sum(0))


def damped(A, damping):
    return A + damping * np.diag(np.diag(A))


def solve(s, damping, min_pixels):
    """-> (status, xi or None)"""
    if s["count"] < min_pixels:
        return FEW, None
    M = damped(s["A"], damping)
    try:
        np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return SINGULAR, None
    return OK, np.linalg.solve(M, s["b"])


def delta_rotation(omega):
    q = np.concatenate([[1.0], np.asarray(omega, np.float64) / 2.0])
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def update(pose, xi):
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    dR = delta_rotation(xi[:3])
    return np.hstack([dR @ pose[:, :3], (dR @ pose[:, 3] + xi[3:])[:, None]])


def step(plane, sensor, cam, pose, gate, jump, damping, min_pixels):
    """one step from a rendered plane -> (status, new pose (the old one unless OK), stats [pixels, rms, |omega|, |v|], sums)"""
    J, r, _, _ = terms(plane, sensor, cam, gate, jump)
    s = sums(J, r)
    status, xi = solve(s, damping, min_pixels)
    rms = float(np.sqrt(s["rr"] / s["count"])) if s["count"] else 0.0
    if status != OK:
        return status, np.asarray(pose, np.float64).reshape(3, 4).copy(), np.array([s["count"], rms, 0.0, 0.0]), s
    return OK, update(pose, xi), np.array([s["count"], rms, np.linalg.norm(xi[:3]), np.linalg.norm(xi[3:])]), s


def refine(scene, obj, pose, cam, sensor, diameter, iterations=8, gate=0.25, jump=0.75, damping=1e-6, min_pixels=32):
    """the loop and the keep / reject rule for one estimate; scene: a vsd_reference.Scene -> (pose [3, 4], status, stats [iterations + 1, 4])"""
    H, W = np.shape(sensor)
    start = np.asarray(pose, np.float64).reshape(3, 4)
    g, cur, codes, stats = gate * diameter, start.copy(), [], []
    for it in range(iterations + 1):
        code, new, st, _ = step(scene.plane(obj, cur, cam, H, W), sensor, cam, cur, g, jump * g, damping, min_pixels)
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
    return (cur if status == OK else start.copy()), status, stats


def rotation_error_deg(P, Q):
    c = (np.trace(np.asarray(P)[:, :3] @ np.asarray(Q)[:, :3].T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def translation_error(P, Q):
    return float(np.linalg.norm(np.asarray(P)[:, 3] - np.asarray(Q)[:, 3]))


def mean_vertex_distance(verts, P, Q):
    v = np.asarray(verts, np.float64)
    a = v @ np.asarray(P)[:, :3].T + np.asarray(P)[:, 3]
    b = v @ np.asarray(Q)[:, :3].T + np.asarray(Q)[:, 3]
    return float(np.linalg.norm(a - b, axis=1).mean())
