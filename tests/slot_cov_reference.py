"""The covariance per slot and keypoint (cp_ls_slot_covariance_f32; csrc/ls_cov_math.h has the definition) restated in NumPy on top of
tests/ls_reference.py and tests/robust_ls_reference.py: what every (pixel, keypoint) adds to the five sums (A00, A01, A11, Q, Wall) against an
estimate handed in, their per-slot sums (L.sums), and the fp64 finish.  The pixel terms exist twice, as theirs do: in fp64 throughout, and formed
in fp32 in the header's order -- p = estimate / H, e = p - c, d = e_y n_x - e_x n_y, rho as RL.rho forms it, omega = w * rho, the matrix terms
as L.terms forms them with omega in place of w, q = omega * (d * d) -- and summed in fp64.  NumPy does not contract a multiply and an add; the
device may, so the fp32 variant is the header's order, not the device's bits.

pixel_moments() is the definition on flat lists of lines (anchor c, unit direction n, weight w), moments() applies it to a field record and a
slot map.  Conventions are ls_reference's; estimates are [B, slots, kp, 2] in (y, x) pixels; cov is (sxx, sxy, syy) in (x, y) pixels."""
import numpy as np

import casapose_oracle as O
import ls_reference as L
import robust_ls_reference as RL

KP = L.KP
MIN_KEPT = RL.MIN_KEPT


def biweight(d, scale, dt):
    """Tukey's biweight of d * scale in RL.rho's order"""
    t = d * scale
    u = t * t
    k = dt(1.0) - u
    return np.where(u < 1.0, k * k, dt(0.0)).astype(dt)


def pixel_moments(cy, cx, ny, nx, w, py, px, h, cutoff, dt):
    """[..., 5] in dt: (a00, a01, a11, q, wall) of lines through (cy, cx) along the unit direction (ny, nx) (or (0, 0): no line) with weight w
    against the estimate (py, px); all normalised (pixels / h), all of dtype dt, broadcast against each other.  cutoff: pixels, or None."""
    with np.errstate(invalid="ignore", over="ignore"):
        ey, ex = py - cy, px - cx
        d = ey * nx - ex * ny
        rho = biweight(d, dt(dt(h) / dt(cutoff)), dt) if cutoff else dt(1.0)
        omega = w * rho
        t = np.stack(np.broadcast_arrays((dt(1.0) - ny * ny) * omega, (-ny * nx) * omega, (dt(1.0) - nx * nx) * omega, omega * (d * d), w), -1)
    assert t.dtype == dt
    return np.where(((ny == 0) & (nx == 0))[..., None], dt(0.0), t)


def weights(field, conf_off, sigmoid, dt, kp=KP):
    """the pixel weights [B,H,W,kp] in dt as L.terms forms them"""
    conf = field[..., conf_off:conf_off + kp]
    with np.errstate(over="ignore", invalid="ignore"):
        if sigmoid:
            return (1.0 / (1.0 + np.exp(-conf.astype(np.float64)))).astype(dt)
        return O.softplus(conf.astype(dt)).astype(dt)


def moment_terms(field, dir_off, conf_off, sigmoid, slot_map, est, cutoff, kp=KP):
    """(t32, t64), each [B,H,W,kp,5] float64: the five terms of every pixel against its slot's estimate (whatever for a pixel of slot 0 or of
    a slot above the estimates' rows: sums() never touches one)"""
    b, h, w, _ = field.shape
    lab = np.asarray(slot_map).astype(np.int64)
    lab = np.where(lab > est.shape[1], 0, lab)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = []
    for dt in (np.float32, np.float64):
        ny, nx = RL.normals(field, dir_off, dt, kp)
        p = (np.asarray(est).astype(dt) / dt(h)).astype(dt)
        pp = p[np.arange(b)[:, None, None], np.maximum(lab - 1, 0)]                # [B,H,W,kp,2]
        cy = ((yy.astype(dt) + dt(0.5)) / dt(h)).astype(dt)[None, :, :, None]
        cx = ((xx.astype(dt) + dt(0.5)) / dt(h)).astype(dt)[None, :, :, None]
        t = pixel_moments(cy, cx, ny, nx, weights(field, conf_off, sigmoid, dt, kp), pp[..., 0], pp[..., 1], h, cutoff, dt)
        out.append(t.astype(np.float64))
    return out[0], out[1]


def moments(field, dir_off, conf_off, sigmoid, slot_map, slots, est, cutoff=None, kp=KP):
    """((S32, A32), (S64, A64)): the per-slot sums of the five terms and of their magnitudes, in the fp32 order and in fp64 throughout.  est is
    fp32 (what the device is handed) or fp64."""
    t32, t64 = moment_terms(field, dir_off, conf_off, sigmoid, slot_map, est, cutoff, kp)
    return L.sums(t32, slot_map, slots), L.sums(t64, slot_map, slots)


def well_posed(s):
    """bool [...]: the rank rule and the condition bound of the robust solve on the matrix (s0, s1, s2)"""
    a, b, c = s[..., 0], s[..., 1], s[..., 2]
    rad = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    l1, l2 = 0.5 * (a + c) + rad, 0.5 * (a + c) - rad
    smax = np.maximum(np.abs(l1), np.abs(l2))
    with np.errstate(invalid="ignore"):
        return (smax > 0) & (np.abs(l2) > RL.RCOND * smax) & (np.abs(l1) > RL.RCOND * smax) & (l2 > 0) & (l1 < RL.MAX_COND * l2)


def finish(s, est, h):
    """(cov [..., 3] = (sxx, sxy, syy) in (x, y) pixels, stat [..., 2] = (sigma2, kept), ok [...]) in fp64 from the five sums and the estimates
    they were summed against: three NaNs where ok is False; stat (0, 0) where W is not > 0 or the estimate is not finite."""
    s = np.asarray(s, np.float64)
    a, b, c, q, wall = (s[..., i] for i in range(5))
    fin = np.isfinite(np.asarray(est, np.float64)).all(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = a + c
        live = fin & (w > 0)
        sw = np.where(live, w, 1.0)
        sigma2 = np.where(live, h * h * q / sw, 0.0)
        kept = np.where(live & (wall > 0), w / np.where(wall > 0, wall, 1.0), 0.0)
        ok = live & well_posed(s) & (w >= MIN_KEPT * wall)
        k = h * h * q / np.where(ok, a * c - b * b, 1.0)
        cov = np.where(ok[..., None], np.stack([k * a, -(k * b), k * c], -1), np.nan)
    return cov, np.stack([sigma2, kept], -1), ok


def condition(s):
    return L.condition(s)


# ---- the definition on flat lists of lines, in fp64: what the calibration and the PnP experiment of tests/test_slot_cov_reference.py run ----------
def flat_vote(cy, cx, ny, nx, w, h):
    """the LS estimate [..., 2] (y, x) in pixels of lines [..., n] (pixels / h), fp64: (sum w (I - n n^T))^-1 sum w (I - n n^T) c"""
    r00, r01, r11 = (1.0 - ny * ny) * w, (-ny * nx) * w, (1.0 - nx * nx) * w
    s = np.stack([r00.sum(-1), r01.sum(-1), r11.sum(-1), (r00 * cy + r01 * cx).sum(-1), (r01 * cy + r11 * cx).sum(-1)], -1)
    det = s[..., 0] * s[..., 2] - s[..., 1] ** 2
    return np.stack([(s[..., 2] * s[..., 3] - s[..., 1] * s[..., 4]) / det, (s[..., 0] * s[..., 4] - s[..., 1] * s[..., 3]) / det], -1) * h


def flat_covariance(cy, cx, ny, nx, w, est, h, cutoff=None):
    """finish() of the fp64 sums of pixel_moments over the last axis of the lines, against est [..., 2] in pixels"""
    f = np.float64
    p = np.asarray(est, f) / h
    t = pixel_moments(cy.astype(f), cx.astype(f), ny.astype(f), nx.astype(f), w.astype(f), p[..., :1], p[..., 1:], h, cutoff, f)
    return finish(t.sum(-2), est, h)
