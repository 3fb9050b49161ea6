"""The least-squares voter (csrc/ls_vote.hip) restated stage by stage in plain NumPy, from the semantics of CoordLSVotingWeighted.calc as
oracle/casapose_oracle.py (ls_voting_sums, ls_voting) and oracle/torch_train_ref.py (ls_voting, keypoint_reprojection_loss) state them: the
per-pixel terms, their fp64 sums, the 2x2 solve, the backward's (p, u) table and its per-pixel closed form, the per-image statistics and the
reprojection loss.  The inputs are the voter's fp32 values; everything here is fp64 except terms()'s first result, which forms each term in
fp32 in the reference's order, as the kernels promise to.  tests/test_ls_reference.py pins these functions against the oracle and against fp64
autograd on the CPU, tests/test_gpu_ls_stages.py compares the kernels' intermediate products with them.

Conventions: object o is label o + 1; a record is [.. logits .. | (dy, dx) * kp | conf * kp ..] at seg_off / dir_off / conf_off; pixel centres are
((y + .5) / H, (x + .5) / H), H for both axes."""
from types import SimpleNamespace

import numpy as np

import casapose_oracle as O

KP = 9


def argmax_labels(field, seg_off, objects):
    """Label map of the arg-max dispatches: the first maximum among the objects + 1 logits."""
    return np.argmax(field[..., seg_off:seg_off + objects + 1], axis=-1).astype(np.uint8)


def terms(field, ld, dir_off, conf_off, sigmoid, h, kp=KP):
    """(t32, t64), each [B,H,W,kp,5] float64: r00, r01, r11, q0, q1 of every pixel.  t32 forms them in fp32 in the order of O.ls_voting_sums
    (softplus / sigmoid rounded to fp32, sqrt, divide-no-nan, (v + 0.5) / H) and widens the results; t64 is the same in fp64 throughout.
    Pixels whose record holds NaN give NaN: sums() never touches a pixel outside its object."""
    b, hh, w, _ = field.shape
    assert field.dtype == np.float32 and field.shape[-1] == ld and hh == h
    conf, d = field[..., conf_off:conf_off + kp], field[..., dir_off:dir_off + 2 * kp].reshape(b, hh, w, kp, 2)
    yy, xx = np.meshgrid(np.arange(hh), np.arange(w), indexing="ij")
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for dt in (np.float32, np.float64):
            if sigmoid:
                wgt = (1.0 / (1.0 + np.exp(-conf.astype(np.float64)))).astype(dt)
            else:
                wgt = O.softplus(conf.astype(dt)).astype(dt)
            n = d.astype(dt)
            nrm = np.sqrt((n * n).sum(-1, keepdims=True))
            n = np.where(nrm > 0, n / np.where(nrm > 0, nrm, 1.0), 0.0).astype(dt)
            ny, nx = n[..., 0], n[..., 1]
            r00, r01, r11 = (1.0 - ny * ny) * wgt, (-ny * nx) * wgt, (1.0 - nx * nx) * wgt
            cy = ((yy.astype(dt) + 0.5) / dt(h)).astype(dt)[None, :, :, None]
            cx = ((xx.astype(dt) + 0.5) / dt(h)).astype(dt)[None, :, :, None]
            q0, q1 = r00 * cy + r01 * cx, r01 * cy + r11 * cx
            t = np.stack([r00, r01, r11, q0, q1], -1)
            assert t.dtype == dt
            out.append(t.astype(np.float64))
    return out[0], out[1]


def sums(t, labels, objects):
    """(S, A) [B,objects,kp,5] fp64: the sums of the terms and of their magnitudes over the pixels with label o + 1."""
    b = t.shape[0]
    s, a = np.zeros((b, objects) + t.shape[3:]), np.zeros((b, objects) + t.shape[3:])
    for bi in range(b):
        for o in range(objects):
            sel = t[bi][np.asarray(labels[bi]) == o + 1]
            s[bi, o], a[bi, o] = sel.sum(0), np.abs(sel).sum(0)
    return s, a


def _matrices(s):
    return np.stack([np.stack([s[..., 0], s[..., 1]], -1), np.stack([s[..., 1], s[..., 2]], -1)], -2)


def solve(s, h):
    """Keypoints [..., 2] (y, x) in pixels: pinv([[S00, S01], [S01, S11]]) (T0, T1) * H with TensorFlow's rank cut-off."""
    mat = _matrices(np.asarray(s, np.float64))
    return (np.linalg.pinv(mat, rcond=O.TF_PINV_RCOND) @ s[..., 3:, None])[..., 0] * h


def condition(s):
    """Condition number of the 2x2 system (inf where it is singular or empty)."""
    a, b, c = s[..., 0], s[..., 1], s[..., 2]
    rad = np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    l1, l2 = 0.5 * (a + c) + rad, 0.5 * (a + c) - rad
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l2 > 0, l1 / np.where(l2 > 0, l2, 1.0), np.inf)


def prepare(s, dkp, h):
    """(pu [..., 4], cond [...]): p = A^-1 (T0, T1) (normalised coordinates) and u = A^-1 (dkp * H) by the rule of ls_bwd_prepare_kernel --
    Cramer's rule in fp64, and four zeros where tr <= 0 or |det| <= 1e-12 tr^2."""
    s = np.asarray(s, np.float64)
    a, b, c, t0, t1 = (s[..., i] for i in range(5))
    g0, g1 = np.asarray(dkp, np.float64)[..., 0] * h, np.asarray(dkp, np.float64)[..., 1] * h
    det, tr = a * c - b * b, a + c
    ok = (tr > 0.0) & (np.abs(det) > 1e-12 * tr * tr)
    sd = np.where(ok, det, 1.0)
    pu = np.stack([(c * t0 - b * t1) / sd, (a * t1 - b * t0) / sd, (c * g0 - b * g1) / sd, (a * g1 - b * g0) / sd], -1)
    return np.where(ok[..., None], pu, 0.0), condition(s)


def pixel_grads(field, dir_off, conf_off, labels, reg_labels, conf_coef, pu, h, kp=KP):
    """The closed form above ls_bwd_prepare_kernel in fp64, for the pixels the backward computes anything for.  pu [B,objects,kp,4] is any
    (p, u) table (prepare()'s, or the device's fp32 one read back); reg_labels / conf_coef [B,kp] come together or are both None.
    Returns (idx [n], gd [n,kp,2], gcf [n,kp]): idx lists, ascending, the flat pixels b*H*W + y*W + x with labels > 0 or reg_labels > 0;
        dL/dw = u.e - (u.n)(n.e),  dL/dn = -w (u (e.n) + e (u.n)),  gd = (dL/dn - n (n.dL/dn)) / |d|,  gcf = dL/dw * sigmoid(conf)
    with e = c - p, n = d / |d| (n = 0, gd = 0 where d = 0), on the pixels with a label; plus conf_coef * sigmoid(conf) where reg_labels > 0."""
    b, hh, w, ld = field.shape
    assert (reg_labels is None) == (conf_coef is None) and hh == h
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    rlab = np.zeros_like(lab) if reg_labels is None else np.asarray(reg_labels).reshape(-1).astype(np.int64)
    idx = np.flatnonzero((lab > 0) | (rlab > 0))
    rec = field.reshape(-1, ld)[idx].astype(np.float64)
    lab, rlab = lab[idx], rlab[idx]
    img, y, x = idx // (hh * w), (idx // w) % hh, idx % w
    fg = lab > 0
    with np.errstate(invalid="ignore", over="ignore"):
        cf = rec[:, conf_off:conf_off + kp]
        sg, wgt = 1.0 / (1.0 + np.exp(-cf)), np.logaddexp(0.0, cf)
        d = rec[:, dir_off:dir_off + 2 * kp].reshape(-1, kp, 2)
        tab = np.asarray(pu, np.float64).reshape(b, -1, kp, 4)[img, np.maximum(lab - 1, 0)]          # [n,kp,4]
        e = np.stack([(y + 0.5) / h, (x + 0.5) / h], -1)[:, None, :] - tab[..., :2]
        u = tab[..., 2:]
        nrm = np.sqrt((d * d).sum(-1))
        pos = nrm > 0
        safe = np.where(pos, nrm, 1.0)[..., None]
        n = np.where(pos[..., None], d / safe, 0.0)
        un, en, ue = (u * n).sum(-1), (e * n).sum(-1), (u * e).sum(-1)
        ln = -wgt[..., None] * (u * en[..., None] + e * un[..., None])
        nl = (n * ln).sum(-1)
        gd = np.where(pos[..., None] & fg[:, None, None], (ln - n * nl[..., None]) / safe, 0.0)
        gcf = np.where(fg[:, None], (ue - un * en) * sg, 0.0)
        if conf_coef is not None:
            gcf = gcf + np.where((rlab > 0)[:, None], np.asarray(conf_coef, np.float64)[img] * sg, 0.0)
    return idx, gd, gcf


def kp_stats(field, conf_off, labels, labels_est, classes, kp=KP):
    """(counts [2,B,classes] int64, conf_sums [B,kp] fp64): pixels of every class in labels / labels_est, a label >= classes counted in bin 0,
    and the sums of softplus(conf) over labels > 0."""
    b = labels.shape[0]
    counts, cs = np.zeros((2, b, classes), np.int64), np.zeros((b, kp))
    for bi in range(b):
        for k, m in enumerate((labels, labels_est)):
            v = np.asarray(m[bi]).reshape(-1).astype(np.int64)
            counts[k, bi] = np.bincount(np.where(v < classes, v, 0), minlength=classes)
        cf = field[bi][np.asarray(labels[bi]) > 0][:, conf_off:conf_off + kp].astype(np.float64)
        cs[bi] = np.logaddexp(0.0, cf).sum(0)
    return counts, cs


def kp_reproj_loss(coords_yx, gt_xy, affine, avail, max_err, weight):
    """(value, g_yx [B,objects,kp,2]) of R.keypoint_reprojection_loss without the regulariser, g_yx = weight * d value / d coords_yx:
    crop pixels -> image through the per-image 2x3 affine, distance to gt, smooth L1, soft cap (slope 0.01 above max_err), mean over the
    keypoints, sum over the available objects / their number."""
    p, gt, A, av = (np.asarray(v, np.float64) for v in (coords_yx, gt_xy, affine, avail))
    A = A.reshape(-1, 2, 3)[:, None, None]
    kp = p.shape[2]
    yy, xx = p[..., 0], p[..., 1]
    X = A[..., 0, 0] * xx + A[..., 0, 1] * yy + A[..., 0, 2]
    Y = A[..., 1, 0] * xx + A[..., 1, 1] * yy + A[..., 1, 2]
    a3 = av[..., None]
    dx, dy = (gt[..., 0] - X) * a3, (gt[..., 1] - Y) * a3
    e = np.sqrt(dx * dx + dy * dy)
    l, slope = np.where(e < 1.0, 0.5 * e * e, e - 0.5), np.where(e < 1.0, e, 1.0)
    capped = l > max_err
    l, slope = np.where(capped, max_err + (l - max_err) * 0.01, l), np.where(capped, slope * 0.01, slope)
    na = av.sum()
    if na <= 0:
        return 0.0, np.zeros_like(p)
    value = (l * a3).sum() / (kp * na)
    c = np.where(e > 0, weight * slope * a3 * a3 / (np.where(e > 0, e, 1.0) * kp * na), 0.0)
    gX, gY = -c * dx, -c * dy
    gx, gy = gX * A[..., 0, 0] + gY * A[..., 1, 0], gX * A[..., 0, 1] + gY * A[..., 1, 1]
    return float(value), np.stack([gy, gx], -1)


def reproj_case(seed=5, b=4, objects=8, kp=9):
    """Points on both sides of e = 1, object (0, 1) beyond the soft cap, one point exactly on its target, objects (1, 2) and (3, 7) unavailable.
    The affines are exact in fp32 (multiples of 1/4), the coordinates multiples of 1/8, so the one exact hit is exact on the device too."""
    rng = np.random.default_rng(seed)
    A = np.zeros((b, 2, 3))
    for bi in range(b):
        A[bi] = np.array([[1.0 + 0.25 * bi, 0.25, 3.0 - bi], [-0.25, 0.75 + 0.25 * bi, 2.0 * bi]])
    coords = np.round(rng.uniform(0, 64, (b, objects, kp, 2)) * 8) / 8
    X = A[:, None, None, 0, 0] * coords[..., 1] + A[:, None, None, 0, 1] * coords[..., 0] + A[:, None, None, 0, 2]
    Y = A[:, None, None, 1, 0] * coords[..., 1] + A[:, None, None, 1, 1] * coords[..., 0] + A[:, None, None, 1, 2]
    r = np.where(rng.random((b, objects, kp)) < 0.5, rng.uniform(0.05, 0.95, (b, objects, kp)), rng.uniform(1.1, 9.0, (b, objects, kp)))
    r[0, 1] = rng.uniform(30.0, 60.0, kp)
    r[2, 3, 4] = 0.0
    ang = rng.uniform(0, 2 * np.pi, (b, objects, kp))
    gt = np.stack([X + r * np.cos(ang), Y + r * np.sin(ang)], -1)
    avail = np.ones((b, objects))
    avail[1, 2] = avail[3, 7] = 0.0
    f = np.float32
    return coords.astype(f), gt.astype(f), A.astype(f), avail.astype(f), 12.5


# ---- the scene of the stage tests ---------------------------------------------------------------------------------------------------------------
B, H = 3, 38
RANK_ONE = 5      # with rank_one=True the object with this label has every direction exactly (1, 0)
TINY = 4          # the object whose confidences lie in [-16, -14]
FAR = 0.4
LAYOUTS = {"rec36": dict(ld=36, seg_off=0, dir_off=9, conf_off=27, objects=8),      # the production record
           "rec40": dict(ld=40, seg_off=4, dir_off=13, conf_off=31, objects=8),     # the generic kernels, every offset non-zero
           "rec32": dict(ld=32, seg_off=0, dir_off=5, conf_off=23, objects=5)}      # objects != 8 (given labels only: logit 5 shares a float with dy of keypoint 0)
WIDTHS = (136, 139)


def label_map(w, objects, b=B, h=H):
    """Labels 1..5 (6.. stay absent) on b x 38 x w, w >= 136, against the voter's 64 x 16 strips (columns 0-63, 64-127, 128-; rows 0-15, 16-31,
    32-37):  1 only in the last, partial strip column, down to the last row;  2 on rows 0, 2, 4, .. of columns 70-100, the rows between empty
    over the whole strip column except where 3 reaches in;  3 across the corner (64, 16) of four strips;  4 inside the first strip;  5 through
    the ragged last strip row.  Image bi is shifted by bi columns where that keeps the layout."""
    assert w >= 136 and objects >= 5
    lab = np.zeros((b, h, w), np.uint8)
    for bi in range(b):
        lab[bi, 18 + bi:38, 10:51 - bi] = 5
        lab[bi, 2:15, 5 + bi:41 + bi] = 4
        lab[bi, 0:31:2, 70 + bi:101 + bi] = 2
        lab[bi, 9:24, 58:70] = 3
        lab[bi, 3 + bi:38, 129:w] = 1
    return lab


def scene(w, ld=36, seg_off=0, dir_off=9, conf_off=27, objects=8, argmax=False, rank_one=False, reg=False, seed=0, b=B, h=H, kp=KP):
    """The shared input of the stage tests.  Every float of the record outside the channels a dispatch may read is NaN, and so are the
    directions of every label-0 pixel and the confidences of every pixel that neither map labels; with argmax the logits are finite everywhere
    and their first maximum is the label (3 % of the pixels tie the label's logit with later classes), otherwise they are NaN too.  Directions
    point at a keypoint near the object with lengths in [0.5, 2] and 0.05 rad of noise, 2 % are exactly (0, 0); confidences are N(0, 1.5) with
    5 % uniform in [-20, 20], object 4's all in [-16, -14].  With reg a second map reg_labels differs from labels so that all four classes
    (label, reg label) zero / non-zero occur everywhere."""
    rng = np.random.default_rng([seed, w, ld, objects])
    labels = label_map(w, objects, b, h)
    fg = labels > 0
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    direct = np.zeros((b, h, w, kp, 2))
    for bi in range(b):
        for o in range(1, 6):
            m = labels[bi] == o
            ys, xs = yy[m], xx[m]
            ext = np.array([np.ptp(ys), np.ptp(xs)]) / 2 + 3.0
            far = 0.3 + FAR * np.arange(kp)[:, None]                              # keypoint j lies further out: the later systems are worse conditioned
            kpt = np.array([ys.mean(), xs.mean()]) + rng.uniform(-1, 1, (kp, 2)) * ext * far
            v = kpt[None] - np.stack([ys, xs], -1)[:, None]                       # [n,kp,2] (dy, dx)
            ang = np.arctan2(v[..., 0], v[..., 1]) + rng.normal(0, 0.05, v.shape[:2])
            length = rng.uniform(0.5, 2.0, v.shape[:2])
            direct[bi][m] = np.stack([np.sin(ang), np.cos(ang)], -1) * length[..., None]
    direct[rng.random((b, h, w, kp)) < 0.02] = 0.0
    conf = rng.normal(0, 1.5, (b, h, w, kp))
    wild = rng.random((b, h, w, kp)) < 0.05
    conf = np.where(wild, rng.uniform(-20, 20, conf.shape), conf)
    conf[labels == TINY] = rng.uniform(-16, -14, (int((labels == TINY).sum()), kp))
    if rank_one:
        direct[labels == RANK_ONE] = np.array([1.0, 0.0])
    reg_labels = None
    if reg:
        gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        reg_labels = np.where(fg, np.where((gx + gy) % 3 == 0, 0, labels), np.where((2 * gx + gy) % 5 == 0, 2, 0)).astype(np.uint8)
    field = np.full((b, h, w, ld), np.nan, np.float32)
    field[..., dir_off:dir_off + 2 * kp] = np.where(fg[..., None], direct.reshape(b, h, w, 2 * kp), np.nan)
    used = fg if reg_labels is None else fg | (reg_labels > 0)
    field[..., conf_off:conf_off + kp] = np.where(used[..., None], conf, np.nan)
    if argmax:
        logits = rng.normal(0, 1, (b, h, w, objects + 1)).astype(np.float32)
        top = logits.max(-1) + np.float32(3.0)
        np.put_along_axis(logits, labels[..., None].astype(np.int64), top[..., None], -1)
        tie = (rng.random((b, h, w)) < 0.03)[..., None] & (np.arange(objects + 1) > labels[..., None]) & (rng.random(logits.shape) < 0.5)
        logits = np.where(tie, top[..., None], logits)
        field[..., seg_off:seg_off + objects + 1] = logits
    return SimpleNamespace(field=field, labels=labels, reg_labels=reg_labels, b=b, h=h, w=w, ld=ld, seg_off=seg_off, dir_off=dir_off,
                           conf_off=conf_off, objects=objects, kp=kp, rank_one=rank_one)
