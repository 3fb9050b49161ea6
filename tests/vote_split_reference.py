"""A NumPy restatement of cp_vote_split_labels' rule (include/casapose_hip.h): np.float32 operation by operation, fp64 for the centroid.  It
shares nothing with the kernels' schedule: rays are walked step by step over all voting pixels at once, peaks come from a sort.  Used only by
the tests (test_vote_split_reference.py pins it by hand on the CPU, test_gpu_vote_split.py compares the kernels with it for equality)."""
import numpy as np

F = np.float32
DEFAULTS = dict(kp_index=0, cell=4, vote_stride=2, min_votes=12, rel_percent=25, nms_radius=2, gate=4.0, min_size=50)


def grid_shape(h, w, cell):
    return -(-h // cell), -(-w // cell)


def accumulate(labels, field, dir_at, objects, cell, vote_stride):
    """step 1 -> acc int32 [n, objects, gh, gw]"""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    gh, gw = grid_shape(h, w, cell)
    acc = np.zeros((n, objects, gh, gw), np.int32)
    for i in range(n):
        ys, xs = np.meshgrid(np.arange(0, h, vote_stride), np.arange(0, w, vote_stride), indexing="ij")
        ys, xs = ys.ravel(), xs.ravel()
        lab = labels[i, ys, xs].astype(np.int64)
        dy, dx = field[i, ys, xs, dir_at].astype(F), field[i, ys, xs, dir_at + 1].astype(F)
        votes = (lab >= 1) & (lab <= objects) & np.isfinite(dy) & np.isfinite(dx) & ~((dy == 0) & (dx == 0))
        ys, xs, lab, dy, dx = ys[votes], xs[votes], lab[votes], dy[votes], dx[votes]
        major_y = np.abs(dy) >= np.abs(dx)
        dmaj, dmin = np.where(major_y, dy, dx), np.where(major_y, dx, dy)
        with np.errstate(all="ignore"):
            m = (dmin / dmaj).astype(F)
        s = np.where(dmaj > 0, F(1), F(-1)).astype(F)
        a0 = (np.where(major_y, ys, xs).astype(F) + F(0.5)).astype(F)
        b0 = (np.where(major_y, xs, ys).astype(F) + F(0.5)).astype(F)
        ea, eb = np.where(major_y, h, w).astype(F), np.where(major_y, w, h).astype(F)
        alive = np.arange(len(ys))
        k = 0
        while len(alive):
            t = (s[alive] * F(cell * k)).astype(F)
            a = (a0[alive] + t).astype(F)
            p = (t * m[alive]).astype(F)
            b = (b0[alive] + p).astype(F)
            inside = (a >= 0) & (a < ea[alive]) & (b >= 0) & (b < eb[alive])
            alive, a, b = alive[inside], a[inside], b[inside]
            ca, cb = np.floor(a / F(cell)).astype(np.int64), np.floor(b / F(cell)).astype(np.int64)
            cy, cx = np.where(major_y[alive], ca, cb), np.where(major_y[alive], cb, ca)
            np.add.at(acc[i], (lab[alive] - 1, cy, cx), 1)
            k += 1
    return acc


def cell_keys(grid):
    gh, gw = grid.shape
    idx = np.arange(gh * gw, dtype=np.uint64).reshape(gh, gw)
    return (grid.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)


def candidate_keys(grid, min_votes, nms_radius):
    """step 2, first half -> uint64 [gh, gw]: a candidate's key, 0 for a cell that is none"""
    gh, gw = grid.shape
    keys = cell_keys(grid)
    out = np.zeros((gh, gw), np.uint64)
    for cy, cx in np.argwhere(grid >= min_votes):
        win = keys[max(cy - nms_radius, 0):cy + nms_radius + 1, max(cx - nms_radius, 0):cx + nms_radius + 1]
        if keys[cy, cx] == win.max():
            out[cy, cx] = keys[cy, cx]
    return out


def peaks(grid, cell, R, min_votes, rel_percent, nms_radius):
    """step 2 for one object's grid -> (inst int32 [R, 4] with pixels = 0, peaks float32 [R, 2], candidate keys)"""
    gh, gw = grid.shape
    cand = candidate_keys(grid, min_votes, nms_radius)
    order = np.sort(cand[cand != 0])[::-1][:R]
    inst = np.tile(np.array([0, 0, -1, -1], np.int32), (R, 1))
    pk = np.zeros((R, 2), F)
    for r, key in enumerate(order):
        votes, at = int(key >> np.uint64(32)), 0xFFFFFFFF - int(key & np.uint64(0xFFFFFFFF))
        top = int(order[0] >> np.uint64(32))
        if votes * 100 < rel_percent * top:
            continue
        cy, cx = divmod(at, gw)
        sv = sy = sx = 0
        for yy in range(max(cy - 1, 0), min(cy + 1, gh - 1) + 1):
            for xx in range(max(cx - 1, 0), min(cx + 1, gw - 1) + 1):
                v = int(grid[yy, xx])
                sv, sy, sx = sv + v, sy + v * (2 * yy + 1), sx + v * (2 * xx + 1)
        inst[r] = (0, votes, cy, cx)
        pk[r] = (F(np.float64(sy) / np.float64(sv) * np.float64(0.5 * cell)), F(np.float64(sx) / np.float64(sv) * np.float64(0.5 * cell)))
    return inst, pk, cand


def dist2(ys, xs, dy, dx, py, px):
    """step 3's distance for arrays of pixels against one peak, float32"""
    with np.errstate(all="ignore"):
        ey = (F(py) - (ys.astype(F) + F(0.5)).astype(F)).astype(F)
        ex = (F(px) - (xs.astype(F) + F(0.5)).astype(F)).astype(F)
        e2 = ((ey * ey).astype(F) + (ex * ex).astype(F)).astype(F)
        n2 = ((dy * dy).astype(F) + (dx * dx).astype(F)).astype(F)
        dot = ((ey * dy).astype(F) + (ex * dx).astype(F)).astype(F)
        cr = ((ey * dx).astype(F) - (ex * dy).astype(F)).astype(F)
        line = ((cr * cr).astype(F) / n2).astype(F)
        use = np.isfinite(n2) & (n2 > 0) & (dot > 0)
    return np.where(use, line, e2).astype(F)


def split_labels(labels, field, dir_off, objects, R, kp_index=0, cell=4, vote_stride=2, min_votes=12, rel_percent=25, nms_radius=2, gate=4.0,
                 min_size=50, stages=False):
    """The whole rule -> (slots uint8 [n,h,w], inst int32 [n,objects,R,4], peaks float32 [n,objects,R,2]); with stages also acc and the
    candidate keys uint64 [n,objects,gh,gw]."""
    labels = np.asarray(labels)
    field = np.asarray(field, F)
    n, h, w = labels.shape
    assert 1 <= R <= 16 and objects * R <= 254 and cell in (2, 4, 8)
    dir_at = dir_off + 2 * kp_index
    acc = accumulate(labels, field, dir_at, objects, cell, vote_stride)
    inst = np.zeros((n, objects, R, 4), np.int32)
    pk = np.zeros((n, objects, R, 2), F)
    keys = np.zeros(acc.shape, np.uint64)
    slots = np.zeros((n, h, w), np.uint8)
    g2 = F(F(gate) * F(gate))
    for i in range(n):
        for o in range(objects):
            inst[i, o], pk[i, o], keys[i, o] = peaks(acc[i, o], cell, R, min_votes, rel_percent, nms_radius)
            ys, xs = np.nonzero(labels[i] == o + 1)
            if not len(ys):
                continue
            dy, dx = field[i, ys, xs, dir_at], field[i, ys, xs, dir_at + 1]
            best = np.full(len(ys), -1, np.int64)
            bd = np.zeros(len(ys), F)
            for r in range(R):
                if inst[i, o, r, 2] < 0:
                    continue
                d2 = dist2(ys, xs, dy, dx, pk[i, o, r, 0], pk[i, o, r, 1])
                take = (d2 <= g2) & ((best < 0) | (d2 < bd))
                best[take], bd[take] = r, d2[take]
            got = best >= 0
            slots[i, ys[got], xs[got]] = o * R + best[got] + 1
            for r in range(R):
                size = int((best == r).sum())
                if size >= min_size:
                    inst[i, o, r, 0] = size
                elif size:
                    slots[i][(slots[i] == o * R + r + 1)] = 0
    return (slots, inst, pk, acc, keys) if stages else (slots, inst, pk)
