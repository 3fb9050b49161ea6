"""Planted scenes for cp_vote_split_labels: discs of one label whose pixels point at their own disc's centre.  A disc (label, cy, cx, radius)
holds the pixels whose centre (y + 0.5, x + 0.5) lies within `radius` of (cy, cx); where two discs overlap the nearer centre wins.  The
direction of a pixel is the unit vector from its centre to its disc's centre, rotated by a normal angle of `sigma` radians drawn from a fixed
seed.  Used by test_vote_split_reference.py (the scenes' conditions, on the reference alone), test_gpu_vote_split.py and the end-to-end test."""
import functools
from types import SimpleNamespace

import numpy as np

import vote_split_reference as VR

SCENES = {
    "touch2": ((48, 64), ((1, 24, 20, 11), (1, 24, 42, 11))),
    "touch3": ((60, 80), ((1, 20, 20, 10), (1, 20, 40, 10), (1, 40, 30, 10))),
    "two_obj": ((48, 64), ((1, 24, 18, 10), (1, 24, 38, 10), (2, 12, 54, 7), (2, 36, 54, 7))),
    "single": ((48, 64), ((1, 24, 32, 14),)),
}
SIGMAS = (0.0, 0.05)
# the issue's parameters for the planted scenes; min_votes goes with the stride
PARAMS = dict(cell=4, rel_percent=25, nms_radius=2, gate=4.0, min_size=50)
R = 4
MIN_VOTES = {1: 20, 2: 6}
MIN_SHARE = 0.94
SEED = 20260


def discs(name):
    """-> (labels uint8 [h, w], owner int [h, w]: the index of the disc a pixel belongs to, -1 for background)"""
    (h, w), items = SCENES[name]
    y, x = np.mgrid[0:h, 0:w]
    best = np.full((h, w), np.inf)
    owner = np.full((h, w), -1, np.int64)
    for i, (_, cy, cx, rad) in enumerate(items):
        d2 = (y + 0.5 - cy) ** 2 + (x + 0.5 - cx) ** 2
        take = (d2 <= rad * rad) & (d2 < best)
        owner[take], best[take] = i, d2[take]
    labels = np.zeros((h, w), np.uint8)
    for i, (label, _, _, _) in enumerate(items):
        labels[owner == i] = label
    return labels, owner


def directions(name, owner, sigma, seed=SEED):
    """float32 [h, w, 2] = (dy, dx): towards the owner's centre, rotated by N(0, sigma) radians; zeros on the background"""
    (h, w), items = SCENES[name]
    y, x = np.mgrid[0:h, 0:w]
    cy = np.array([it[1] for it in items], np.float64)[np.maximum(owner, 0)]
    cx = np.array([it[2] for it in items], np.float64)[np.maximum(owner, 0)]
    ang = np.arctan2(cy - (y + 0.5), cx - (x + 0.5)) + sigma * np.random.default_rng(seed).standard_normal((h, w))
    d = np.stack([np.sin(ang), np.cos(ang)], -1)
    d[owner < 0] = 0.0
    return d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name, sigma, ld=36, dir_off=9, kp_index=0):
    """One planted scene as a batch of one: labels [1,h,w], field [1,h,w,ld] with the direction at dir_off + 2*kp_index and a constant
    elsewhere (so that a kernel reading the wrong floats is caught), owner [h,w] and the objects' count."""
    labels, owner = discs(name)
    h, w = labels.shape
    field = np.full((1, h, w, ld), 0.25, np.float32)
    at = dir_off + 2 * kp_index
    field[0, :, :, at:at + 2] = directions(name, owner, sigma)
    objects = max(it[0] for it in SCENES[name][1])
    for a in (labels, owner, field):
        a.setflags(write=False)
    return SimpleNamespace(name=name, labels=labels[None], field=field, owner=owner, objects=objects, items=SCENES[name][1], ld=ld, dir_off=dir_off,
                           kp_index=kp_index)


def params(stride):
    return dict(PARAMS, vote_stride=stride, min_votes=MIN_VOTES[stride])


@functools.lru_cache(maxsize=None)
def reference(name, sigma, stride):
    """The reference's result on a planted scene, computed once: (slots, inst, peaks, acc, keys)"""
    s = scene(name, sigma)
    out = VR.split_labels(s.labels, s.field, s.dir_off, s.objects, R, stages=True, **params(stride))
    for a in out:
        a.setflags(write=False)
    return out


def shares(name, slots):
    """Per planted disc: (the slot most of its pixels carry, the share of its pixels that carry it)"""
    s = scene(name, 0.0)
    out = []
    for i in range(len(s.items)):
        mine = slots[0][s.owner == i]
        values, counts = np.unique(mine, return_counts=True)
        top = int(np.argmax(counts))
        out.append((int(values[top]), counts[top] / len(mine)))
    return out


# ---- maps that are not planted scenes: several objects, a batch, ragged grids, directions that do not vote ---------------------------------------
def blobs(n, h, w, objects, ld, dir_off, kp_index, seed, radius=(5, 9), per_object=2, spoil=True):
    """n images of `objects` objects with `per_object` discs each at random places (they may touch, overlap or leave the image); a pixel points at
    its disc's centre with 0.1 rad of noise and a length between 0.1 and 3.  With `spoil`, a few pixels get what the rule has to cope with: a zero
    direction, a NaN, an infinity, an axis-aligned or exactly diagonal direction, a label above `objects`; the last image's last object is absent."""
    rng = np.random.default_rng(seed)
    labels = np.zeros((n, h, w), np.uint8)
    field = rng.uniform(-1, 1, (n, h, w, ld)).astype(np.float32)
    at = dir_off + 2 * kp_index
    y, x = np.mgrid[0:h, 0:w]
    for i in range(n):
        for o in range(1, objects + 1):
            if spoil and i == n - 1 and o == objects and objects > 1:
                continue
            for _ in range(per_object):
                cy, cx, rad = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(*radius)
                inside = (y + 0.5 - cy) ** 2 + (x + 0.5 - cx) ** 2 <= rad * rad
                ang = np.arctan2(cy - (y + 0.5), cx - (x + 0.5)) + 0.1 * rng.standard_normal((h, w))
                length = rng.uniform(0.1, 3.0, (h, w))
                labels[i][inside] = o
                field[i, :, :, at][inside] = (np.sin(ang) * length)[inside]
                field[i, :, :, at + 1][inside] = (np.cos(ang) * length)[inside]
        if spoil:
            fg = np.argwhere(labels[i] > 0)
            picks = fg[rng.choice(len(fg), size=min(24, len(fg)), replace=False)]
            specials = [(0.0, 0.0), (np.nan, 1.0), (1.0, np.inf), (-np.inf, np.nan), (0.0, 1.5), (-2.0, 0.0), (0.75, 0.75), (-0.5, 0.5), (1e-30, -1.0),
                        (3e38, 3e38), (1e-42, 1e-42), (-0.0, 0.0)]
            for j, (py, px) in enumerate(picks):
                if j < len(specials):
                    field[i, py, px, at:at + 2] = specials[j]
                elif j < len(specials) + 4:
                    labels[i, py, px] = objects + 1 + j % 3
    return labels, field


CONFIGS = {
    # name: (blobs arguments, objects, R, parameters)
    "ragged_c2": (dict(n=2, h=37, w=50, objects=3, ld=36, dir_off=9, kp_index=0, seed=1), 3, 4, dict(cell=2, vote_stride=1, min_votes=6, min_size=10)),
    "ragged_c4": (dict(n=2, h=37, w=50, objects=3, ld=36, dir_off=9, kp_index=0, seed=2), 3, 16, dict(cell=4, vote_stride=2, min_votes=3, min_size=10)),
    "ragged_c8": (dict(n=2, h=37, w=50, objects=3, ld=20, dir_off=1, kp_index=3, seed=3), 3, 1, dict(cell=8, vote_stride=1, min_votes=6, min_size=10)),
    "narrow_r4": (dict(n=2, h=60, w=80, objects=5, ld=20, dir_off=1, kp_index=3, seed=4, radius=(6, 12)), 5, 4,
                  dict(cell=4, vote_stride=2, min_votes=4, nms_radius=1, gate=3.0, min_size=20, rel_percent=40)),
    "stride3_r16": (dict(n=1, h=48, w=64, objects=2, ld=36, dir_off=9, kp_index=0, seed=5, per_object=5), 2, 16,
                    dict(cell=4, vote_stride=3, min_votes=2, nms_radius=1, rel_percent=0, min_size=5)),
}


@functools.lru_cache(maxsize=None)
def config(name):
    """-> (labels, field, dir_off, objects, R, parameters, the reference's (slots, inst, peaks, acc, keys)), computed once and read-only"""
    if name == "objects_254":            # 254 objects of 2 x 4 pixels on 32 x 64, one instance each: the last slot id a byte holds
        labels = np.zeros((1, 32, 64), np.uint8)
        field = np.full((1, 32, 64, 36), 0.5, np.float32)
        for o in range(254):
            ty, tx = divmod(o, 16)
            labels[0, 2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4] = o + 1
            yy, xx = np.mgrid[2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4]
            field[0, 2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4, 9] = 2 * ty + 1 - (yy + 0.5)
            field[0, 2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4, 10] = 4 * tx + 2 - (xx + 0.5)
        dir_off, objects, r, p = 9, 254, 1, dict(cell=4, vote_stride=1, min_votes=2, nms_radius=1, rel_percent=0, gate=4.0, min_size=4)
    elif name == "production":           # 480 x 640, one object: the LDS grid is the production one (120 x 160), 15 bands of rows
        h, w = 480, 640
        y, x = np.mgrid[0:h, 0:w]
        rng = np.random.default_rng(6)
        labels = np.zeros((1, h, w), np.uint8)
        field = np.full((1, h, w, 36), 0.25, np.float32)
        for cy, cx, rad in ((200, 200, 90), (200, 380, 90), (400, 560, 60)):      # two that touch, one apart and cut by the image's corner
            inside = ((y + 0.5 - cy) ** 2 + (x + 0.5 - cx) ** 2 <= rad * rad) & (labels[0] == 0)
            ang = np.arctan2(cy - (y + 0.5), cx - (x + 0.5)) + 0.05 * rng.standard_normal((h, w))
            labels[0][inside] = 1
            field[0, :, :, 9][inside] = np.sin(ang)[inside]
            field[0, :, :, 10][inside] = np.cos(ang)[inside]
        dir_off, objects, r, p = 9, 1, 4, dict(cell=4, vote_stride=2, min_votes=12, rel_percent=25, nms_radius=2, gate=4.0, min_size=50)
    else:
        args, objects, r, p = CONFIGS[name]
        labels, field = blobs(**args)
        dir_off, p = args["dir_off"], dict(p, kp_index=args["kp_index"])
    want = VR.split_labels(labels, field, dir_off, objects, r, stages=True, **p)
    for a in (labels, field) + tuple(want):
        a.setflags(write=False)
    return labels, field, dir_off, objects, r, p, want


CONFIG_NAMES = tuple(sorted(CONFIGS)) + ("objects_254", "production")
