"""A NumPy restatement of the pose verification's rule (casapose_amd/csrc/verify_math.h), integers and fp64: what cp_pose_verify_i32 and its host
twin must give, byte for byte.  It shares no code with them.

counts(...) takes the kernel's arrays as NumPy arrays and returns int32 [njobs, 8]: rendered, hidden, on_label, on_background, on_other,
label_pixels, pairs, inliers."""
import numpy as np

EMPTY = 0xFFFFFFFF
RENDERED, HIDDEN, ON_LABEL, ON_BACKGROUND, ON_OTHER, LABEL_PIXELS, PAIRS, INLIERS = range(8)


def clipped_box(rec, H, W):
    """bbox_obj (x, y, w, h) of a record clipped to the image -> (x0, y0, x1, y1), closed, or None"""
    x, y, w, h = (int(v) for v in rec[2:6])
    if w < 0 or h < 0:
        return None
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W - 1), min(y + h, H - 1)
    return (x0, y0, x1, y1) if x0 <= x1 and y0 <= y1 else None


def job_counts(planes, records, inst_counts, imax, labels, field, dir_off, kp, kps, job, sample_offset, cos_min):
    """one job -> int64 [8]; planes uint32 [nplanes, H, W], records [nplanes, 11], labels uint8 [images, H, W], field float32
    [images, H, W, ld], kps float64 [kp, 2] as (y, x)"""
    out = np.zeros(8, np.int64)
    nplanes, H, W = planes.shape
    m, p, l = (int(v) for v in job[:3])
    if not (0 <= m < len(labels) and 0 <= p < nplanes and 1 <= l <= 255) or p // imax >= len(inst_counts):
        return out
    out[LABEL_PIXELS] = int((labels[m] == l).sum())
    box = clipped_box(records[p], H, W)
    if box is None:
        return out
    x0, y0, x1, y1 = box
    rows, cols = slice(y0, y1 + 1), slice(x0, x1 + 1)
    mine = planes[p, rows, cols].astype(np.int64)
    rendered = mine != EMPTY
    hidden = np.zeros_like(rendered)
    first = (p // imax) * imax
    for q in range(first, min(first + min(max(int(inst_counts[p // imax]), 0), imax), nplanes)):
        other = clipped_box(records[q], H, W)
        if q == p or other is None:
            continue
        ii, jj = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        within = (jj >= other[0]) & (jj <= other[2]) & (ii >= other[1]) & (ii <= other[3])
        theirs = planes[q, rows, cols].astype(np.int64)
        hidden |= rendered & within & ((theirs < mine) | ((theirs == mine) & (q < p)))
    visible = rendered & ~hidden
    lab = labels[m, rows, cols]
    on_label = visible & (lab == l)
    out[RENDERED], out[HIDDEN], out[ON_LABEL] = rendered.sum(), hidden.sum(), on_label.sum()
    out[ON_BACKGROUND], out[ON_OTHER] = (visible & (lab == 0)).sum(), (visible & (lab != 0) & (lab != l)).sum()
    ii, jj = np.nonzero(on_label)
    ci, cj = (ii + y0).astype(np.float64) + float(sample_offset), (jj + x0).astype(np.float64) + float(sample_offset)
    cos2 = np.float64(cos_min) * np.float64(cos_min)
    with np.errstate(all="ignore"):
        for k in range(kp):
            dy = field[m, ii + y0, jj + x0, dir_off + 2 * k].astype(np.float64)
            dx = field[m, ii + y0, jj + x0, dir_off + 2 * k + 1].astype(np.float64)
            ey, ex = np.float64(kps[k, 0]) - ci, np.float64(kps[k, 1]) - cj
            dd, ee, de = dy * dy + dx * dx, ey * ey + ex * ex, dy * ey + dx * ex
            pair = (dd > 0) & np.isfinite(dd) & (ee > 0) & np.isfinite(ee)
            out[PAIRS] += pair.sum()
            out[INLIERS] += (pair & (de >= 0) & (de * de >= (cos2 * dd) * ee)).sum()
    return out


def counts(planes, records, inst_counts, imax, labels, field, dir_off, kp, kp2d, jobs, sample_offset, cos_min):
    jobs = np.asarray(jobs, np.int64).reshape(-1, 4)
    kp2d = np.asarray(kp2d, np.float64).reshape(len(jobs), kp, 2)
    got = [job_counts(planes, records, inst_counts, imax, labels, field, dir_off, kp, kp2d[n], jobs[n], sample_offset, cos_min) for n in range(len(jobs))]
    return np.asarray(got, np.int64).reshape(-1, 8).astype(np.int32)


def score_from_counts(c):
    """-> (iou, agreement, visible, score) float64 [n] from counts [n, 8]; a ratio is 0 where its denominator is 0"""
    c = np.asarray(c, np.float64).reshape(-1, 8)

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b > 0)

    iou = ratio(c[:, ON_LABEL], c[:, LABEL_PIXELS] + c[:, ON_BACKGROUND])
    agreement = ratio(c[:, INLIERS], c[:, PAIRS])
    visible = ratio(c[:, RENDERED] - c[:, HIDDEN], c[:, RENDERED])
    return iou, agreement, visible, iou * agreement
