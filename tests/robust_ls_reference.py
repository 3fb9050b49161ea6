"""The robust voter per slot (cp_ls_vote_slots_robust_f32; csrc/ls_robust_math.h has the weight and the solve rule) restated in NumPy on top of
tests/ls_reference.py: the weight rho of every (pixel, keypoint) against an estimate, the reweighted terms and their per-slot sums (L.sums), the
rule that takes or refuses a reweighted system (L.solve, L.condition), and the chain of passes.  Everything exists twice: in fp64 throughout, and
with rho and the terms formed in fp32 in the header's order -- p = estimate / H, e = p - c, t = (e_y n_x - e_x n_y) * (H / cutoff), u = t t,
rho = (1 - u)^2, the term's weight w * rho -- and summed in fp64, as the kernels promise to.  NumPy does not contract a multiply and an add; the
device may, so the fp32 variant is the header's order, not the device's bits.

Conventions are ls_reference's; a slot map is a label map with `slots` labels; estimates and keypoints are [B, slots, kp, 2] in (y, x) pixels."""
from types import SimpleNamespace

import numpy as np

import casapose_oracle as O
import ls_reference as L

KP = L.KP
MIN_KEPT = 0.125        # CP_LS_ROBUST_MIN_KEPT
MAX_COND = 1e6          # CP_LS_ROBUST_MAX_COND
MAX_PASSES = 8
RCOND = 10.0 * 2.0 * np.finfo(np.float64).eps      # the plain solve's rank rule (ls_solve_kernel)


def normals(field, dir_off, dt, kp=KP):
    """(ny, nx) [B,H,W,kp] in dt: d / |d| as L.terms forms it, (0, 0) where d = 0"""
    b, h, w, _ = field.shape
    n = field[..., dir_off:dir_off + 2 * kp].reshape(b, h, w, kp, 2).astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.sqrt((n * n).sum(-1, keepdims=True))
        n = np.where(nrm > 0, n / np.where(nrm > 0, nrm, 1.0), 0.0).astype(dt)
    return n[..., 0], n[..., 1]


def rho(field, dir_off, slot_map, est, h, cutoff, dt, kp=KP):
    """[B,H,W,kp] in dt: Tukey's biweight of the distance of the slot's estimate from the pixel's line, in the header's order; 0 for a zero
    direction; whatever for a pixel of slot 0 (sums() never touches one).  est: [B,slots,kp,2] pixels, of dtype dt or narrower."""
    b, hh, w, _ = field.shape
    assert hh == h
    ny, nx = normals(field, dir_off, dt, kp)
    lab = np.asarray(slot_map).astype(np.int64)
    p = (np.asarray(est).astype(dt) / dt(h)).astype(dt)
    pp = p[np.arange(b)[:, None, None], np.maximum(lab - 1, 0)]                # [B,H,W,kp,2]
    yy, xx = np.meshgrid(np.arange(hh), np.arange(w), indexing="ij")
    cy = ((yy.astype(dt) + dt(0.5)) / dt(h)).astype(dt)[None, :, :, None]
    cx = ((xx.astype(dt) + dt(0.5)) / dt(h)).astype(dt)[None, :, :, None]
    scale = dt(dt(h) / dt(cutoff))
    with np.errstate(invalid="ignore", over="ignore"):
        ey, ex = pp[..., 0] - cy, pp[..., 1] - cx
        t = (ey * nx - ex * ny) * scale
        u = t * t
        k = dt(1.0) - u
        out = np.where(u < 1.0, k * k, dt(0.0))
    out = np.where((ny == 0) & (nx == 0), dt(0.0), out)
    assert out.dtype == dt
    return out


def weighted_terms(field, ld, dir_off, conf_off, sigmoid, h, rho32=None, rho64=None, kp=KP):
    """L.terms with every pixel's weight multiplied by rho BEFORE the terms are formed (ls_add_terms is handed w * rho): (t32, t64).  Without
    rho these are L.terms' values bit for bit (tests/test_robust_ls_reference.py pins that)."""
    b, hh, w, _ = field.shape
    assert field.dtype == np.float32 and field.shape[-1] == ld and hh == h
    conf = field[..., conf_off:conf_off + kp]
    yy, xx = np.meshgrid(np.arange(hh), np.arange(w), indexing="ij")
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for dt, r in ((np.float32, rho32), (np.float64, rho64)):
            if sigmoid:
                wgt = (1.0 / (1.0 + np.exp(-conf.astype(np.float64)))).astype(dt)
            else:
                wgt = O.softplus(conf.astype(dt)).astype(dt)
            if r is not None:
                assert r.dtype == dt
                wgt = wgt * r
            ny, nx = normals(field, dir_off, dt, kp)
            r00, r01, r11 = (1.0 - ny * ny) * wgt, (-ny * nx) * wgt, (1.0 - nx * nx) * wgt
            cy = ((yy.astype(dt) + 0.5) / dt(h)).astype(dt)[None, :, :, None]
            cx = ((xx.astype(dt) + 0.5) / dt(h)).astype(dt)[None, :, :, None]
            q0, q1 = r00 * cy + r01 * cx, r01 * cy + r11 * cx
            t = np.stack([r00, r01, r11, q0, q1], -1)
            assert t.dtype == dt
            out.append(t.astype(np.float64))
    return out[0], out[1]


def trace(s):
    return s[..., 0] + s[..., 2]


def accepted(again, plain):
    """bool [...]: the solve rule's three conditions on the reweighted sums `again` beside the plain sums `plain`"""
    a, b, c = again[..., 0], again[..., 1], again[..., 2]
    rad = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    l1, l2 = 0.5 * (a + c) + rad, 0.5 * (a + c) - rad
    smax = np.maximum(np.abs(l1), np.abs(l2))
    with np.errstate(invalid="ignore"):
        rank = (smax > 0) & (np.abs(l2) > RCOND * smax) & (np.abs(l1) > RCOND * smax)
        return rank & (l2 > 0) & (l1 < MAX_COND * l2) & (trace(again) >= MIN_KEPT * trace(plain))


def step(again, plain, prev, h):
    """keypoints after a reweighted pass: L.solve of the reweighted sums where the rule takes them, `prev` elsewhere"""
    ok = accepted(again, plain)
    return np.where(ok[..., None], L.solve(np.where(ok[..., None], again, 0.0), h), prev), ok


def kept(again, plain):
    """the share of the plain weight in the reweighted sums; 0 for an empty slot"""
    w = trace(plain)
    return np.where(w > 0, trace(again) / np.where(w > 0, w, 1.0), 0.0)


def one_pass(field, ld, dir_off, conf_off, sigmoid, slot_map, slots, est, cutoff, kp=KP):
    """One reweighted pass against the fp32 estimates `est`: ((S32, A32), (S64, A64)), the per-slot sums of the reweighted terms and of their
    magnitudes, in the fp32 order and in fp64 throughout."""
    h = field.shape[1]
    est = np.asarray(est, np.float32)
    t32, t64 = weighted_terms(field, ld, dir_off, conf_off, sigmoid, h, rho(field, dir_off, slot_map, est, h, cutoff, np.float32, kp),
                              rho(field, dir_off, slot_map, est, h, cutoff, np.float64, kp), kp)
    return L.sums(t32, slot_map, slots), L.sums(t64, slot_map, slots)


def device_rounding(kps, h):
    """fp64 keypoints in pixels as ls_solve_kernel stores them: p rounded to fp32, times H in fp32"""
    return (np.asarray(kps, np.float64) / h).astype(np.float32) * np.float32(h)


def run(field, ld, dir_off, conf_off, sigmoid, slot_map, slots, cutoff=4.0, passes=2, order="fp64", kp=KP):
    """The chain: the plain vote, then `passes` reweighted passes.  order "fp64": everything in fp64, the estimates never rounded; "fp32": rho
    and the terms in fp32 in the header's order, summed in fp64, the estimates rounded as the device stores them.
    -> plain (S, A), kps [passes + 1] (kps[0] the plain solve), sums [passes] of (S, A), took [passes] of bool [B,slots,kp]"""
    assert order in ("fp64", "fp32") and 0 <= passes <= MAX_PASSES and np.isfinite(cutoff) and cutoff > 0
    h = field.shape[1]
    pick = 0 if order == "fp32" else 1
    dt = np.float32 if order == "fp32" else np.float64
    store = (lambda k: device_rounding(k, h)) if order == "fp32" else (lambda k: k)
    plain = L.sums(L.terms(field, ld, dir_off, conf_off, sigmoid, h, kp)[pick], slot_map, slots)
    kps, sums, took = [store(L.solve(plain[0], h))], [], []
    for _ in range(passes):
        r = rho(field, dir_off, slot_map, kps[-1], h, cutoff, dt, kp)
        t = weighted_terms(field, ld, dir_off, conf_off, sigmoid, h, r if pick == 0 else None, r if pick == 1 else None, kp)[pick]
        again = L.sums(t, slot_map, slots)
        new, ok = step(again[0], plain[0], kps[-1], h)
        kps.append(np.where(ok[..., None], store(new), kps[-1]))
        sums.append(again)
        took.append(ok)
    return SimpleNamespace(plain=plain, kps=kps, sums=sums, took=took)
