"""The inputs of the pose-loss stage tests (test_gpu_loss_stages.py on the GPU, test_loss_reference.py against the oracles on the CPU).  Every case
is built deterministically for properties the kernels branch on; `check(case, ref)` asserts those properties on the REFERENCE (tests/loss_reference.py),
so a case that no longer has them fails before any kernel output is looked at.  All float inputs are float32 arrays: the fp64 reference and the
kernels read the same numbers.  `out` is the tight record [b,h,w,K + 2kp] (merged) or [b,h,w,K + (K-1)*2kp] (separated); the GPU tests re-lay it."""
import functools
from types import SimpleNamespace

import numpy as np

import loss_reference as R

MERGED_GRID_CAP = 512 * 256       # cp_pose_loss_f32: at most 512 blocks of 256 threads per image
SEP_GRID_CAP = 1024 * 256         # grid_x() of csrc/loss_functional.hip
RECORD_SHAPES = ((2, 9), (5, 9), (13, 4), (32, 16))      # (K, kp) of the layout sweep


def cell_labels(b, h, w, K, rng, keep=0.85):
    """objects 1..K-1 on a grid of cells, each cell filled raggedly (a fraction `keep` of its pixels), different per image"""
    objects = K - 1
    cols = int(np.ceil(np.sqrt(objects)))
    rows = -(-objects // cols)
    lab = np.zeros((b, h, w), np.uint8)
    for o in range(objects):
        r, c = divmod(o, cols)
        y0, y1 = r * h // rows, (r + 1) * h // rows
        x0, x1 = c * w // cols, (c + 1) * w // cols
        lab[:, y0:y1, x0:x1] = (o + 1) * (rng.random((b, y1 - y0, x1 - x0)) < keep)
    return lab


def random_record(lab_ce, K, kp, sep, rng):
    """normal logits, mostly right about lab_ce, and directions at two scales (both smooth-L1 branches of the vertex error)"""
    b, h, w = lab_ce.shape
    nv = (K - 1 if sep else 1) * 2 * kp
    out = rng.standard_normal((b, h, w, K + nv)).astype(np.float32)
    out[..., :K] += 3.0 * np.eye(K, dtype=np.float32)[lab_ce] * (rng.random((b, h, w, 1)) < 0.7)
    out[..., K:] *= np.where(rng.random((b, h, w, 1)) < 0.5, 0.3, 3.0).astype(np.float32)
    return out


def random_keypoints(b, K, kp, h, w, rng):
    return rng.uniform(-10.0, max(h, w) + 8.0, (b, K - 1, kp, 2)).astype(np.float32)


def sure_logits(out, K, where, lab):
    """make the arg-max prediction equal `lab` on the pixels `where`, by a wide margin"""
    out[where, :K] = (6.0 * np.eye(K, dtype=np.float32)[lab[where]] - 3.0)


def _case(name, out, labels_ce, labels_fg, kpts, K, kp, sep, check, **extra):
    for a in (out, kpts):
        assert a.dtype == np.float32 and np.isfinite(a).all()
    for a in (labels_ce, labels_fg):
        assert a.dtype == np.uint8 and a.max() < K
    for a in (out, labels_ce, labels_fg, kpts):
        a.setflags(write=False)
    assert out.shape[-1] == K + (K - 1 if sep else 1) * 2 * kp and kpts.shape == (labels_fg.shape[0], K - 1, kp, 2)
    return SimpleNamespace(name=name, out=out, labels_ce=labels_ce, labels_fg=labels_fg, kpts=kpts, K=K, kp=kp, sep=sep, check=check, **extra)


# ---- 1. labels_fg a proper subset of labels_ce --------------------------------------------------------------------------------------------------
def subset_fg(K=5, kp=9, sep=False, seed=1):
    rng = np.random.default_rng(seed * 1000 + K * 17 + kp)
    b, h, w = 2, 24, 32
    ce = cell_labels(b, h, w, K, rng)
    fg = ce.copy()
    fg[0][ce[0] == 1] = 0                                              # image 0: object 1 erased whole
    part = (ce[1] == K - 1) & (rng.random((h, w)) < 0.5)               # image 1: a ragged half of the last object
    fg[1][part] = 0
    extra = rng.random((b, h, w)) < 0.12                               # and a sprinkle over everything, so that every object differs somewhere
    fg[extra] = 0
    out = random_record(ce, K, kp, sep, rng)

    def check(case, ref):
        differ = case.labels_ce != case.labels_fg
        assert ((case.labels_fg == 0) | (case.labels_fg == case.labels_ce)).all()
        assert differ.sum() >= 0.1 * (case.labels_ce != 0).sum() and differ[0].any() and differ[1].any()
        assert not (case.labels_fg[0] == 1).any() and (case.labels_ce[0] == 1).sum() >= 3

    return _case("subset_fg", out, ce, fg, random_keypoints(b, K, kp, h, w, rng), K, kp, sep, check)


# ---- 2. an image without foreground ----------------------------------------------------------------------------------------------------------------
def empty_image(K=5, kp=9, sep=False):
    rng = np.random.default_rng(200 + K)
    b, h, w = 2, 24, 32
    ce = cell_labels(b, h, w, K, rng)
    fg = ce.copy()
    fg[1] = 0
    out = random_record(ce, K, kp, sep, rng)

    def check(case, ref):
        assert len(np.unique(case.labels_ce[1])) == case.K and not case.labels_fg[1].any() and case.labels_fg[0].any()
        counts = ref(False).count1 if not case.sep else ref(False).counts.sum(1)
        assert counts[1] == 0 and counts[0] > 100

    return _case("empty_image", out, ce, fg, random_keypoints(b, K, kp, h, w, rng), K, kp, sep, check)


# ---- 3. 25 foreground pixels beside 600 -----------------------------------------------------------------------------------------------------------
def unequal_counts(K=5, kp=9, sep=False):
    rng = np.random.default_rng(300 + K)
    b, h, w = 2, 24, 32
    lab = np.zeros((b, h, w), np.uint8)
    lab[0, 9:14, 20:25] = 1
    lab[1] = cell_labels(1, h, w, K, rng, keep=0.9)[0]
    out = random_record(lab, K, kp, sep, rng)
    sure_logits(out, K, lab != 0, lab)                                 # the segmentation filter changes no count

    def check(case, ref):
        for seg in (False, True):
            r = ref(seg)
            counts = r.count1 if not case.sep else r.counts.sum(1)
            assert counts[0] == 25 and counts[1] >= 500, counts

    return _case("unequal_counts", out, lab, lab.copy(), random_keypoints(b, K, kp, h, w, rng), K, kp, sep, check)


# ---- 4. objects of 19, 20 and 21 pixels (merged model, the proxy-error filter) ---------------------------------------------------------------------
def small_objects():
    rng = np.random.default_rng(400)
    b, h, w, K, kp = 2, 24, 32, 5, 9
    lab = np.zeros((b, h, w), np.uint8)
    for n in range(b):
        lab[n, 2:6, 2:7], lab[n, 5, 6] = 1, 0                          # 19
        lab[n, 2:6, 12:17] = 2                                         # 20
        lab[n, 2:6, 22:27], lab[n, 6, 22] = 3, 3                       # 21
        lab[n, 10:22, 4:28] = 4 * (rng.random((12, 24)) < 0.9)
    kpts = random_keypoints(b, K, kp, h, w, rng)
    kpts[:, :3] += np.float32(60.0)                                    # far away: random directions miss them by many pixels
    kpts[:, 3] = (rng.integers(-10, 40, (b, kp, 2)) + 0.5).astype(np.float32)
    out = random_record(lab, K, kp, False, rng)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    for n in range(b):
        # The large object points exactly at its keypoints, and exactly in fp32 as well: its keypoints end in .5, so (ay, ax) are integers and the
        # direction (ay, ax) itself gives num = ay*ax - ax*ay = 0 with exact products.  (Unit vectors rounded to fp32 would leave a proxy distance
        # that is nothing but rounding noise, ~1e-6 px, different noise in fp32 and in fp64: no relative bound can hold on a sum of it.)
        m = lab[n] == 4
        a = kpts[n, 3][None, None] - np.stack([yy, xx], -1).astype(np.float32)[:, :, None, :]
        out[n][m, K:] = a.reshape(h, w, -1)[m]
    sure_logits(out, K, lab != 0, lab)

    def check(case, ref):
        for seg in (False, True):
            r = ref(seg, False)
            assert (r.objcnt[:, :3] == (19, 20, 21)).all() and (r.objcnt[:, 3] >= 200).all()
            assert (r.value[:, 0] == 0).all() and (r.objsum[:, 0] > 5.5 * kp * 19).all()         # large error, but below 20 pixels: value 0, kept
            assert (r.value[:, 1:3] > 5.5).all() and (r.value[:, 3] == 0).all() and (r.objsum[:, 3] == 0).all()
            assert (r.bad == (False, True, True, False)).all()
            f = ref(seg, True)
            assert np.array_equal(f.fg1 != 0, np.isin(case.labels_fg, (1, 4))) and (f.count1 == r.objcnt[:, 0] + r.objcnt[:, 3]).all()

    return _case("small_objects", out, lab, lab.copy(), kpts, K, kp, False, check)


# ---- 5. values on either side of 5 ------------------------------------------------------------------------------------------------------------------
def threshold():
    """direction (1, 0) everywhere on the two objects: the proxy distance of a pixel is |k_x - c_x|, so an object's value is set by where its
    keypoints' x lies: 5 x 6 pixels with c_x = 4.5 .. 9.5 and all k_x = 12.75 give mean(|k_x - c_x|) - 0.5 = 5.25; k_x = 12.25 gives 4.75"""
    rng = np.random.default_rng(500)
    b, h, w, K, kp = 2, 24, 32, 5, 9
    lab = np.zeros((b, h, w), np.uint8)
    lab[:, 3:8, 4:10], lab[:, 12:17, 4:10] = 1, 2
    lab[:, 3:20, 14:30] = 3 + (rng.random((b, 17, 16)) < 0.4)          # two ordinary objects beside them
    kpts = random_keypoints(b, K, kp, h, w, rng)
    kpts[:, 0, :, 1], kpts[:, 1, :, 1] = 12.75, 12.25
    out = random_record(lab, K, kp, False, rng)
    out[(lab == 1) | (lab == 2), K:] = np.tile(np.float32([1.0, 0.0]), kp)
    sure_logits(out, K, lab != 0, lab)

    def check(case, ref):
        for seg in (False, True):
            r = ref(seg, False)
            assert (r.objcnt[:, :2] == 30).all()
            assert (r.value[:, 0] > 5.05).all() and (r.value[:, 0] < 5.5).all() and (r.value[:, 1] < 4.95).all() and (r.value[:, 1] > 4.5).all()
            assert (r.bad[:, 0] == True).all() and (r.bad[:, 1] == False).all()                       # noqa: E712

    return _case("threshold", out, lab, lab.copy(), kpts, K, kp, False, check)


# ---- 6. arg-max ties ----------------------------------------------------------------------------------------------------------------------------------
def ties(K=5, kp=9, sep=False):
    rng = np.random.default_rng(600 + K)
    b, h, w = 2, 24, 32
    lab = cell_labels(b, h, w, K, rng)
    out = random_record(lab, K, kp, sep, rng)
    out[..., :K] = np.minimum(out[..., :K], np.float32(3.5))
    tie = (lab != 0) & (rng.random((b, h, w)) < 0.5)
    other = np.zeros((b, h, w), np.int64)
    for idx in np.argwhere(tie):
        l = int(lab[tuple(idx)])
        m = int(rng.choice([k for k in range(K) if k != l]))           # below the label (the label loses the tie) or above it (it wins)
        other[tuple(idx)] = m
        out[tuple(idx)][[l, m]] = np.float32(4.0)

    def check(case, ref):
        z = case.out[..., :case.K]
        own = np.take_along_axis(z, case.labels_fg[..., None].astype(np.int64), -1)[..., 0]
        oth = np.take_along_axis(z, other[..., None], -1)[..., 0]
        assert (own[tie] == 4.0).all() and (oth[tie] == 4.0).all() and (z.max(-1)[tie] == 4.0).all()
        lower, higher = tie & (other < case.labels_fg), tie & (other > case.labels_fg)
        assert lower.sum() >= 20 and (higher.sum() >= 20 or case.K == 2)
        r = ref(True)
        kept = (r.fg0 if not case.sep else r.fg) != 0
        assert not kept[lower].any() and kept[higher].all()

    return _case("ties", out, lab, lab.copy(), random_keypoints(b, K, kp, h, w, rng), K, kp, sep, check)


# ---- 7. zero directions, keypoints on pixel centres, num == 0 -------------------------------------------------------------------------------------------
def degenerate(K=5, kp=9, sep=False):
    """every keypoint coordinate ends in .5, so (ay, ax) are integers at every pixel; a direction m * (ay, ax) with a small integer m makes
    num = vy*ax - vx*ay a difference of two equal, exactly representable products: 0 in fp32 however it is contracted"""
    rng = np.random.default_rng(700 + K)
    b, h, w = 2, 24, 32
    lab = cell_labels(b, h, w, K, rng, keep=0.95)
    kpts = (rng.integers(-10, 40, (b, K - 1, kp, 2)) + 0.5).astype(np.float32)
    objects = K - 1
    cols = int(np.ceil(np.sqrt(objects)))
    rows = -(-objects // cols)
    for o in range(objects):                                            # keypoints 0 and 1 of every object on pixel centres inside its own cell
        r, c = divmod(o, cols)
        for j in (0, 1):
            kpts[:, o, j] = (r * h // rows + 1 + j + 0.5, c * w // cols + 1 + 2 * j + 0.5)
    out = random_record(lab, K, kp, sep, rng)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    kind = rng.integers(0, 4, (b, h, w, kp))                            # per (pixel, keypoint): 0 random, 1 zero, 2 multiple of (ay, ax), 3 nearly exact
    for n in range(b):
        for o in range(objects):
            m = lab[n] == o + 1
            a = kpts[n, o].astype(np.float64)[None, None] - np.stack([yy, xx], -1)[:, :, None, :]       # [h,w,kp,2], integers
            unit = a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-9)
            ang = rng.normal(0.0, 0.01, unit.shape[:-1])
            near = 1.3 * np.stack([np.cos(ang) * unit[..., 0] - np.sin(ang) * unit[..., 1], np.sin(ang) * unit[..., 0] + np.cos(ang) * unit[..., 1]], -1)
            mult = a * rng.choice([-2, -1, 1, 2, 3], unit.shape[:-1])[..., None]
            base = K + (o * 2 * kp if sep else 0)
            cur = out[n, :, :, base:base + 2 * kp].reshape(h, w, kp, 2)
            new = np.where((kind[n] == 1)[..., None], 0.0, np.where((kind[n] == 2)[..., None], mult, np.where((kind[n] == 3)[..., None], near, cur)))
            out[n, :, :, base:base + 2 * kp][m] = new.reshape(h, w, -1)[m].astype(np.float32)

    def check(case, ref):
        assert (case.kpts * 2 % 2 == 1).all()
        raw = ref(False).raw
        on = raw.on[..., None] & np.ones(raw.n2.shape, bool)
        zero_dir, on_centre = on & (raw.n2 == 0), on & (raw.tn == 0)
        num0 = on & (raw.num == 0) & (raw.n2 > 0) & (raw.tn > 0)
        assert zero_dir.sum() >= 200 and on_centre.sum() >= case.K - 1 and num0.sum() >= 200, (zero_dir.sum(), on_centre.sum(), num0.sum())
        assert (on_centre & (raw.n2 > 0)).any()                                           # a keypoint on the pixel's centre under a non-zero direction
        e = np.concatenate([raw.ey[on], raw.ex[on]])
        d = raw.dist[on & (raw.n2 > 0)]
        branch = ((e < 1).sum(), (e >= 1).sum(), (d < 1).sum(), (d >= 1).sum())
        assert min(branch) >= 200, branch

    return _case("degenerate", out, lab, lab.copy(), kpts, K, kp, sep, check)


# ---- 8. fewer pixels than a wave has lanes ------------------------------------------------------------------------------------------------------------
def one_wave(K=5, kp=9, sep=False):
    rng = np.random.default_rng(800 + K)
    b, h, w = 1, 5, 7
    ce = cell_labels(b, h, w, K, rng, keep=0.9)
    fg = np.where(rng.random((b, h, w)) < 0.8, ce, 0).astype(np.uint8)
    out = random_record(ce, K, kp, sep, rng)

    def check(case, ref):
        assert case.labels_fg.size < 64 and (case.labels_fg != 0).sum() >= 10 and (case.labels_fg != case.labels_ce).any()

    return _case("one_wave", out, ce, fg, random_keypoints(b, K, kp, h, w, rng), K, kp, sep, check)


# ---- 9. the second trip of the grid-stride loops -------------------------------------------------------------------------------------------------------
def _second_trip(name, h, w, cap, sep):
    rng = np.random.default_rng(h)
    b, K, kp = 2, 3, 2
    ce = np.zeros((b, h, w), np.uint8)
    ce[:, 3:40, 10:200] = 1 + (rng.random((b, 37, 190)) < 0.3)         # in the first trip
    ce[0, h - 9:, 37:w - 5] = 2                                         # the last rows: the second trip, raggedly
    ce[1, h - 3:, 60:460] = 1
    ce[:, h - 12:, :] *= rng.random((b, 12, w)) < 0.9
    fg = np.where(rng.random((b, h, w)) < 0.9, ce, 0).astype(np.uint8)
    out = random_record(ce, K, kp, sep, rng)

    def check(case, ref):
        ppi = h * w
        assert ppi > cap and (sep or ppi % 256 != 0)
        r = ref(True)
        kept = ((r.fg if sep else r.fg1) != 0).reshape(b, ppi)
        for n in range(b):
            assert kept[n, :cap].sum() >= 1000 and kept[n, cap:].sum() >= 200, (n, kept[n, :cap].sum(), kept[n, cap:].sum())
        assert kept[0, cap:].sum() != kept[1, cap:].sum()

    return _case(name, out, ce, fg, random_keypoints(b, K, kp, h, w, rng), K, kp, sep, check)


@functools.lru_cache(maxsize=None)
def second_trip_merged():
    return _second_trip("second_trip_merged", 260, 508, MERGED_GRID_CAP, False)


@functools.lru_cache(maxsize=None)
def second_trip_sep():
    return _second_trip("second_trip_sep", 516, 512, SEP_GRID_CAP, True)


BUILDERS = {"subset_fg": subset_fg, "empty_image": empty_image, "unequal_counts": unequal_counts, "small_objects": small_objects,
            "threshold": threshold, "ties": ties, "degenerate": degenerate, "one_wave": one_wave}
MERGED = tuple(BUILDERS)                                               # small cases of cp_pose_loss_f32, at (K, kp) = (5, 9)
SEP = ("subset_fg", "empty_image", "unequal_counts", "ties", "degenerate", "one_wave")       # small cases of cp_pose_loss_sep_f32, K in SEP_K
SEP_K = (2, 4)
WEIGHTS = (1.0, 0.5, 0.015)


@functools.lru_cache(maxsize=None)
def build(name, K=5, kp=9, sep=False):
    if name == "second_trip_merged":
        return second_trip_merged()
    if name == "second_trip_sep":
        return second_trip_sep()
    if name in ("small_objects", "threshold"):
        assert (K, kp, sep) == (5, 9, False)
        return BUILDERS[name]()
    return BUILDERS[name](K=K, kp=kp, sep=sep)


@functools.lru_cache(maxsize=None)
def _reference(name, K, kp, sep, seg_filter, proxy_filter):
    c = build(name, K, kp, sep)
    if sep:
        return R.separated(c.out, c.labels_ce, c.labels_fg, c.kpts, K, kp, seg_filter, WEIGHTS)
    return R.merged(c.out, c.labels_ce, c.labels_fg, c.kpts, K, kp, seg_filter, proxy_filter, WEIGHTS)


@functools.lru_cache(maxsize=None)
def checked(name, K=5, kp=9, sep=False):
    """the case, its properties asserted on the reference; `reference(case, seg_filter, proxy_filter)` gives the (cached) reference results"""
    c = build(name, K, kp, sep)
    c.check(c, lambda seg, prox=False: _reference(name, c.K, c.kp, c.sep, seg, prox and not c.sep))
    return c


def reference(case_name, K=5, kp=9, sep=False, seg_filter=False, proxy_filter=False):
    c = checked(case_name, K, kp, sep)
    return _reference(case_name, c.K, c.kp, c.sep, bool(seg_filter), bool(proxy_filter) and not c.sep)
