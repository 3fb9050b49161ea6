"""The inputs tests/test_verify_reference.py, tests/test_verify_twin_host.py and tests/test_gpu_pose_verify.py share: planes written by hand or
drawn from a seeded generator (cp_pose_verify_i32 takes planes as input, so no render is needed), built once and never modified.  A case is a
dict of the kernel's arrays: planes uint32 [nplanes, H, W], records int32 [nplanes, 11], inst_counts int32 [frames], imax, labels uint8
[images, H, W], field float32 [images, H, W, ld], dir_off, kp, kp2d float64 [njobs, kp, 2], jobs int32 [njobs, 4], sample_offset, cos_min."""
import functools

import numpy as np

EMPTY = np.uint32(0xFFFFFFFF)
TILE = 256          # cp_pose_verify_tile(); tests/test_verify_twin_host.py checks that it is


def bits(z):
    return np.float32(z).view(np.uint32)


def frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def record(x0, y0, x1, y1):
    r = np.full(11, -1, np.int32)
    r[2:6] = (x0, y0, x1 - x0, y1 - y0)
    return r


# ---- the 5 x 7 case, worked out by hand ----------------------------------------------------------------------------------------------------
# Plane 0 covers rows 1-3 x columns 1-4 at depth 2, plane 1 rows 2-4 x columns 3-6 at depth 1.5; they overlap in rows 2-3 x columns 3-4.
# There plane 1 is nearer at (2, 4) and (3, 3), has plane 0's very word at (2, 3) -- the lower plane keeps that pixel -- and lies behind at
# (3, 4) (depth 3).  Job A = (plane 0, label 1): 12 rendered, 2 hidden, 10 visible: (1, 1) lies on label 0, (1, 4) on label 2, the other 8 on
# label 1.  Label 1 has 10 pixels in the image (two of them, (0, 0) and (4, 0), outside the render).  With the keypoint at (2.5, 3.5), the
# sample offset 0.5 and cos_min 0.6 the eight on_label pixels hold, in order:
#   (1, 2) e = (1, 1)    d = (2, 2)        on the ray                     pair, inlier
#   (1, 3) e = (1, 0)    d = (-1, 0)       opposite                       pair
#   (2, 1) e = (0, 2)    d = (4-, 3)       cos a hair above 3 / 5         pair, inlier          (4- and 4+: the fp32 neighbours of 4)
#   (2, 2) e = (0, 1)    d = (4+, 3)       cos a hair below 3 / 5         pair
#   (2, 3) e = (0, 0)    d = (1, 0)        the keypoint at the centre     --
#   (3, 1) e = (-1, 2)   d = (0, 0)                                       --
#   (3, 2) e = (-1, 1)   d = (NaN, 1)                                     --
#   (3, 4) e = (-1, -1)  d = (inf, 1)      not finite                     --
# Job B = (plane 1, label 2): 12 rendered, hidden at (2, 3) (equal words, plane 0 is lower) and (3, 4); all 10 visible pixels lie on label 2,
# which has 11 pixels; every direction there is the ray to B's keypoint (0.25, 6.75) itself: 10 pairs, 10 inliers.
HAND_A = (12, 2, 8, 1, 1, 10, 4, 2)
HAND_B = (12, 2, 10, 0, 0, 11, 10, 10)


@functools.lru_cache(maxsize=None)
def hand():
    H, W, ld, dir_off = 5, 7, 4, 1
    planes = np.full((2, H, W), EMPTY, np.uint32)
    planes[0, 1:4, 1:5] = bits(2.0)
    planes[1, 2:5, 3:7] = bits(1.5)
    planes[1, 2, 3] = bits(2.0)
    planes[1, 3, 4] = bits(3.0)
    records = np.stack([record(1, 1, 4, 3), record(3, 2, 6, 4)])
    labels = np.array([[1, 0, 0, 0, 0, 0, 0],
                       [0, 0, 1, 1, 2, 0, 0],
                       [0, 1, 1, 1, 2, 2, 2],
                       [0, 1, 1, 2, 1, 2, 2],
                       [1, 0, 0, 2, 2, 2, 2]], np.uint8)[None]
    kp_a, kp_b = (2.5, 3.5), (0.25, 6.75)
    field = np.full((1, H, W, ld), np.nan, np.float32)
    for i in range(H):
        for j in range(W):
            field[0, i, j, dir_off:dir_off + 2] = (kp_b[0] - (i + 0.5), kp_b[1] - (j + 0.5))
    four = np.float32(4.0)
    below, above = np.nextafter(four, np.float32(0.0)), np.nextafter(four, np.float32(8.0))
    for (i, j), d in {(1, 2): (2, 2), (1, 3): (-1, 0), (2, 1): (below, 3), (2, 2): (above, 3), (2, 3): (1, 0), (3, 1): (0, 0), (3, 2): (np.nan, 1),
                      (3, 4): (np.inf, 1)}.items():
        field[0, i, j, dir_off:dir_off + 2] = d
    return frozen(dict(planes=planes, records=records, inst_counts=np.array([2], np.int32), imax=2, labels=labels, field=field, dir_off=dir_off, kp=1,
                       kp2d=np.array([[kp_a], [kp_b]], np.float64), jobs=np.array([(0, 0, 1, 0), (0, 1, 2, 0)], np.int32), sample_offset=0.5,
                       cos_min=0.6))


# ---- seeded cases --------------------------------------------------------------------------------------------------------------------------
DEPTHS = (1.0, 1.5, 2.0, 2.0, 3.25)      # few values, so that equal words on two planes happen


def drawn(seed, H, W, images, frames, imax, ld, dir_off, kp, boxes=None, label_values=(1, 2, 3), inst_counts=None, cos_min=0.9):
    """frames * imax planes: plane p gets a box (boxes[p], or a random one that may cross the border), an ellipse of hits inside it in patches
    of DEPTHS, and a record holding the box.  Label maps of rectangles of `label_values`; a field of N(0, 1) directions with zeros, NaN and
    infinities sprinkled in, and towards keypoint 0 of job 0 on a third of the pixels; one job per plane (image p % images, the plane's
    own label in turn), keypoints in and around the image, some exactly at a pixel's centre."""
    rng = np.random.default_rng(seed)
    nplanes = frames * imax
    planes = np.full((nplanes, H, W), EMPTY, np.uint32)
    records = np.full((nplanes, 11), -1, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for p in range(nplanes):
        if boxes is not None and p < len(boxes):
            x0, y0, x1, y1 = boxes[p]
        else:
            x0, y0 = int(rng.integers(-3, max(W - 2, 1))), int(rng.integers(-3, max(H - 2, 1)))
            x1, y1 = x0 + int(rng.integers(0, max(W // 2, 2))), y0 + int(rng.integers(0, max(H // 2, 2)))
        records[p] = record(x0, y0, x1, y1)
        cy, cx, ry, rx = (y0 + y1) / 2, (x0 + x1) / 2, (y1 - y0) / 2 + 0.6, (x1 - x0) / 2 + 0.6
        hit = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        depth = np.asarray(DEPTHS, np.float32)[rng.integers(0, len(DEPTHS), (H // 4 + 1, W // 4 + 1))].repeat(4, 0).repeat(4, 1)[:H, :W]
        planes[p][hit] = depth.view(np.uint32)[hit]
    labels = np.zeros((images, H, W), np.uint8)
    for m in range(images):
        for _ in range(6):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            labels[m, y:y + int(rng.integers(1, H // 2 + 2)), x:x + int(rng.integers(1, W // 2 + 2))] = label_values[int(rng.integers(0, len(label_values)))]
    jobs = np.array([(p % images, p, label_values[p % len(label_values)], 0) for p in range(nplanes)], np.int32)
    kp2d = np.stack([rng.uniform(-4, H + 4, (nplanes, kp)), rng.uniform(-4, W + 4, (nplanes, kp))], axis=-1)
    kp2d[::3, 0] = np.floor(kp2d[::3, 0]) + 0.5          # keypoint 0 of every third job: exactly at a pixel's centre
    field = rng.normal(0, 1, (images, H, W, ld)).astype(np.float32)
    towards = rng.random((images, H, W)) < 1 / 3
    centre = np.stack([yy + 0.5, xx + 0.5], axis=-1)
    for k in range(kp):
        ray = (kp2d[0, k] - centre).astype(np.float32)
        field[..., dir_off + 2 * k:dir_off + 2 * k + 2][towards] = np.broadcast_to(ray, (images, H, W, 2))[towards]
    odd = rng.random(field.shape)
    field[odd < 0.02], field[(odd >= 0.02) & (odd < 0.03)], field[(odd >= 0.03) & (odd < 0.04)] = 0.0, np.nan, np.inf
    counts = np.full(frames, imax, np.int32) if inst_counts is None else np.asarray(inst_counts, np.int32)
    return dict(planes=planes, records=records, inst_counts=counts, imax=imax, labels=labels, field=field, dir_off=dir_off, kp=kp, kp2d=kp2d, jobs=jobs,
                sample_offset=0.5, cos_min=cos_min)


@functools.lru_cache(maxsize=None)
def tiles():
    """boxes of TILE - 1, TILE and TILE + 1 pixels (15 x 17, 16 x 16, 257 x 1) and one of 11 steps, overlapping, at a width that is no multiple
    of 64; the generic record ld 20 / dir_off 3 / kp 1"""
    boxes = [(3, 2, 17, 18), (10, 1, 25, 16), (20, 9, 276, 9), (1, 0, 140, 19)]
    return frozen(drawn(1, 20, 300, 1, 1, 4, 20, 3, 1, boxes=boxes))


@functools.lru_cache(maxsize=None)
def production():
    """the production record ld 36 / dir_off 9 / kp 9 over three images and two frames of four planes; the second frame counts three of its four,
    the jobs are shuffled, one plane is named by two jobs (with another label and image), one job is out of range, one label is 255"""
    boxes = [(5, 3, 40, 25), (20, 10, 60, 30), (-3, -2, 30, 20), (35, 5, 80, 40), (10, 5, 50, 30), (25, 8, 70, 36), (0, 15, 40, 36), (30, 0, 74, 20)]
    c = drawn(2, 37, 75, 3, 2, 4, 36, 9, 9, boxes=boxes, label_values=(1, 255, 7), inst_counts=[4, 3])
    c["labels"][1, 12:28, 25:55] = 255                   # under plane 1, whose job names image 1 and label 255
    rng = np.random.default_rng(3)
    jobs = np.concatenate([c["jobs"], [(2, 1, 7, 0), (1, 8, 1, 0)]]).astype(np.int32)       # plane 1 again; plane 8 of 8
    kp2d = np.concatenate([c["kp2d"], c["kp2d"][:2]])
    order = rng.permutation(len(jobs))
    c["jobs"], c["kp2d"] = np.ascontiguousarray(jobs[order]), np.ascontiguousarray(kp2d[order])
    return frozen(c)


@functools.lru_cache(maxsize=None)
def crowd():
    """a frame of 256 planes at 8 x 8: every plane can hide every other"""
    return frozen(drawn(4, 8, 8, 1, 1, 256, 4, 0, 2))


@functools.lru_cache(maxsize=None)
def odd_record():
    """ld 7 / dir_off 2 / kp 2: a record that no 16-byte load can take"""
    return frozen(drawn(5, 19, 23, 2, 2, 3, 7, 2, 2))


CASES = {"hand": hand, "tiles": tiles, "production": production, "256 planes": crowd, "ld 7": odd_record}
