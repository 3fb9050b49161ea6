"""The inputs of the instance-loss tests (test_gpu_instance_loss.py on the GPU, test_instance_loss_reference.py on the CPU), in the manner of
tests/loss_cases.py: every case is built deterministically for a property cp_pose_loss_inst_f32 branches on, and `check(case, ref)` asserts
that property on the REFERENCE (tests/instance_loss_reference.py) before any kernel output is looked at.

A condition on the inputs instead of a tolerance: outside the two tie cases the builders draw until, under the nearest-centre rule, the
reference's best and second-best candidates differ by more than MARGIN pixels at every foreground pixel (the centre rule) and at every
(pixel, keypoint) (the proxy minimum).  `checked()` asserts that margin on the reference.  Distances in a 24 x 32 .. 364 x 364 image are below
1e3 px, fp32 resolves them to 1e-4 px at worst, so the fp32 kernel cannot legitimately choose another instance, and no pixel is exempt from the
comparison.  Absent instances (index >= the object's count) hold NaN: they must never reach a result."""
import functools
from types import SimpleNamespace

import numpy as np

import instance_loss_reference as R
import loss_cases as Cs

MARGIN = 1e-3
WEIGHTS = Cs.WEIGHTS
BASE = dict(b=2, h=24, w=32, K=3, kp=9, I=3)


def _case(name, out, ce, fg, kpts, counts, imap, K, kp, check, ties=None):
    b, h, w = fg.shape
    I = kpts.shape[2]
    assert out.dtype == np.float32 and np.isfinite(out).all() and out.shape == (b, h, w, K + 2 * kp)
    assert kpts.dtype == np.float32 and kpts.shape == (b, K - 1, I, kp, 2) and counts.dtype == np.int32 and counts.shape == (b, K - 1)
    assert (counts >= 0).all() and (counts <= I).all()
    present = np.arange(I)[None, None, :] < counts[:, :, None]
    kpts = np.where(present[..., None, None], kpts, np.float32(np.nan))                # NaN in every absent keypoint
    assert np.isfinite(kpts[present]).all()
    for a in (ce, fg) + (() if imap is None else (imap,)):
        assert a.dtype == np.uint8 and a.shape == (b, h, w)
    assert ce.max() < K and fg.max() < K
    for a in (out, ce, fg, kpts, counts) + (() if imap is None else (imap,)):
        a.setflags(write=False)
    return SimpleNamespace(name=name, out=out, labels_ce=ce, labels_fg=fg, kpts=kpts, counts=counts, imap=imap, K=K, kp=kp, I=I, check=check,
                           ties=ties)


def reference_of(c, use_map, seg=False, prox=False):
    return R.merged_instances(c.out, c.labels_ce, c.labels_fg, c.kpts, c.counts, c.imap if use_map else None, c.K, c.kp, seg, prox, WEIGHTS)


def random_scene(rng, b, h, w, K, kp, I, counts, radius=6.5, keep=0.9, half=False):
    """centres (keypoint 0) inside the image, the other keypoints within 12 px of them; a pixel belongs to the (object, instance) whose centre is
    nearest among all present ones, if within `radius`; so the instance map agrees with the nearest-centre rule"""
    objects = K - 1
    kpts = np.zeros((b, objects, I, kp, 2), np.float32)
    kpts[:, :, :, 0] = rng.uniform((3, 3), (h - 3, w - 3), (b, objects, I, 2))
    kpts[:, :, :, 1:] = kpts[:, :, :, :1] + rng.uniform(-12, 12, (b, objects, I, kp - 1, 2))
    kpts = (np.floor(kpts) + 0.5 if half else kpts).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    d = np.hypot(kpts[:, :, :, 0, 0][..., None, None].astype(np.float64) - yy, kpts[:, :, :, 0, 1][..., None, None].astype(np.float64) - xx)
    d = np.where((np.arange(I)[None, None, :] < counts[:, :, None])[..., None, None], d, np.inf).reshape(b, objects * I, h, w)
    slot = d.argmin(1)
    near = np.take_along_axis(d, slot[:, None], 1)[:, 0] <= radius
    near &= rng.random((b, h, w)) < keep
    lab = np.where(near, slot // I + 1, 0).astype(np.uint8)
    imap = np.where(near, slot % I, 0).astype(np.uint8)
    return kpts, lab, imap


def aimed_directions(rng, out, K, kp, kpts, lab, imap, noise=0.02):
    """directions towards the keypoints of the pixel's OWN instance, turned by a little noise, at two scales"""
    b, h, w = lab.shape
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    k = np.nan_to_num(kpts.astype(np.float64))[np.arange(b)[:, None, None], np.maximum(lab.astype(int) - 1, 0), imap.astype(int)]     # [b,h,w,kp,2]
    a = k - np.stack([yy, xx], -1)[None, :, :, None, :]
    u = a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-9)
    ang = rng.normal(0.0, noise, u.shape[:-1])
    s = np.where(rng.random(u.shape[:-1]) < 0.5, 0.4, 2.5)
    v = np.stack([np.cos(ang) * u[..., 0] - np.sin(ang) * u[..., 1], np.sin(ang) * u[..., 0] + np.cos(ang) * u[..., 1]], -1) * s[..., None]
    on = lab != 0
    out[on, K:] = v.reshape(b, h, w, -1)[on].astype(np.float32)


def settle(rng, make, redraw=None, exempt=None, tries=400):
    """make() -> the case's arrays (out writable).  Draw until the nearest-rule reference has its margins: a centre gap at or below MARGIN
    redraws everything, a proxy gap at or below MARGIN redraws that pixel's directions (`redraw(out, where)`; default: fresh normal directions)"""
    for _ in range(tries):
        out, ce, fg, kpts, counts, imap, K, kp = make()
        for _ in range(tries):
            r = R.merged_instances(out, ce, fg, kpts, counts, None, K, kp, False, False, WEIGHTS)
            on = r.raw.on if exempt is None else r.raw.on & ~exempt
            if (r.raw.centre_gap[on] <= 2 * MARGIN).any():
                break
            close = on & (r.raw.proxy_gap <= 2 * MARGIN).any(-1)
            if not close.any():
                return out, ce, fg, kpts, counts, imap, K, kp
            if redraw is None:
                out[close, K:] = (rng.standard_normal((int(close.sum()), 2 * kp)) * 1.5).astype(np.float32)
            else:
                redraw(out, close)
    raise AssertionError("no draw with the margins")


def assert_margins(c, ref, exempt=None):
    on = ref.raw.on if exempt is None else ref.raw.on & ~exempt
    assert (ref.raw.centre_gap[on] > MARGIN).all() and (ref.raw.proxy_gap[on] > MARGIN).all()


def _random_inputs(rng, counts, b, h, w, K, kp, I, aimed=False, **kw):
    kpts, lab, imap = random_scene(rng, b, h, w, K, kp, I, counts, **kw)
    out = Cs.random_record(lab, K, kp, False, rng)
    if aimed:
        aimed_directions(rng, out, K, kp, kpts, lab, imap)
    return out, lab, lab.copy(), kpts, counts, imap, K, kp


# ---- 1. the map agrees with the nearest rule --------------------------------------------------------------------------------------------------
def two_discs():
    """Every keypoint coordinate ends in .5 and a pixel's directions are small integer multiples of (a_y, a_x) towards its OWN instance, so its own
    proxy numerators are exactly 0 in fp32 and in fp64 (loss_cases.degenerate) and the minimum over the instances is the pixel's own instance.
    Pixels where another instance's keypoint comes within the margin of such a line, or whose centres are nearly tied, are taken out of the labels."""
    rng = np.random.default_rng(11)
    b, h, w, K, kp, I = (BASE[k] for k in ("b", "h", "w", "K", "kp", "I"))
    counts = np.int32([[2, 3], [3, 2]])
    kpts, lab, imap = random_scene(rng, b, h, w, K, kp, I, counts, half=True)
    out = Cs.random_record(lab, K, kp, False, rng)
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    own = kpts.astype(np.float64)[np.arange(b)[:, None, None], np.maximum(lab.astype(int) - 1, 0), imap.astype(int)]
    a = own - np.stack([yy, xx], -1)[None, :, :, None, :]
    out[lab != 0, K:] = (a * rng.choice([-2, -1, 1, 2, 3], a.shape[:-1])[..., None]).reshape(b, h, w, -1)[lab != 0].astype(np.float32)
    for _ in range(50):
        r = R.merged_instances(out, lab, lab, kpts, counts, None, K, kp, False, False, WEIGHTS)
        on = r.raw.on
        drop = on & ((r.raw.rv != imap) | (r.raw.rp != imap[..., None]).any(-1) | (r.raw.centre_gap <= 2 * MARGIN) | (r.raw.proxy_gap <= 2 * MARGIN).any(-1))
        if not drop.any():
            break
        lab = np.where(drop, 0, lab).astype(np.uint8)
    imap = np.where(lab != 0, imap, 0).astype(np.uint8)

    def check(c, ref):
        near, mapped = ref(False), ref(True)
        assert_margins(c, near)
        on = near.raw.on
        assert on.sum() >= 300 and np.array_equal(near.raw.rv[on], c.imap[on]) and (near.raw.rp[on] == c.imap[on][:, None]).all()
        assert len(np.unique(c.imap[on])) == 3
        assert np.array_equal(near.grad_dirs, mapped.grad_dirs) and near.vertex == mapped.vertex and near.proxy == mapped.proxy == 0.0

    return _case("two_discs", out, lab, lab.copy(), kpts, counts, imap, K, kp, check)


# ---- 2. the map hands pixels to an instance whose centre is not nearest ------------------------------------------------------------------------
def occluding():
    rng = np.random.default_rng(12)
    counts = np.int32([[3, 2], [2, 3]])
    out, ce, fg, kpts, counts, imap, K, kp = settle(rng, lambda: _random_inputs(rng, counts, **BASE))
    xx = np.arange(BASE["w"])[None, None, :]
    n = np.concatenate([np.zeros((2, 1), np.int64), counts], 1)[np.arange(2)[:, None, None], fg]
    imap = np.where((fg != 0) & (xx % 2 == 0), (imap + 1) % np.maximum(n, 1), imap).astype(np.uint8)     # every other column: the next instance

    def check(c, ref):
        near, mapped = ref(False), ref(True)
        assert_margins(c, near)
        on = near.raw.on
        assert np.array_equal(mapped.raw.on, on) and ((near.raw.rv != mapped.raw.rv) & on).sum() >= 20
        assert np.array_equal(mapped.raw.rv[on], c.imap[on]) and not np.array_equal(near.grad_dirs, mapped.grad_dirs)

    return _case("occluding", out, ce, fg, kpts, counts, imap, K, kp, check)


# ---- 3. absent instances, an object without any ---------------------------------------------------------------------------------------------------
def absent():
    rng = np.random.default_rng(13)
    counts = np.int32([[1, 0], [3, 2]])

    def make():
        out, ce, fg, kpts, c, imap, K, kp = _random_inputs(rng, counts, **BASE)
        ce, fg = ce.copy(), fg.copy()
        ce[0, 2:9, 20:30], fg[0, 2:9, 20:30] = 2, 2                                      # pixels of the object that has no instance in image 0
        return out, ce, fg, kpts, c, imap, K, kp

    out, ce, fg, kpts, counts, imap, K, kp = settle(rng, make)

    def check(c, ref):
        assert np.isnan(c.kpts[0, 0, 1:]).all() and np.isnan(c.kpts[0, 1]).all() and np.isnan(c.kpts[1, 1, 2]).all() and np.isfinite(c.kpts[1, 0]).all()
        for use_map in (False, True):
            for seg in (False, True):
                r = ref(use_map, seg, True)
                assert (c.labels_fg[0] == 2).sum() == 70 and not (r.fg0[0] == 2).any() and r.objcnt[0, 1] == 0
                assert r.count0[0] == (r.fg0[0] == 1).sum() and r.count0[0] >= 50 and r.count0[1] >= 200
                for a in (r.grad_logits, r.grad_dirs, r.objsum, r.value):
                    assert np.isfinite(a).all()
                assert np.isfinite([r.mask, r.vertex, r.proxy]).all()
        assert_margins(c, ref(False))

    return _case("absent", out, ce, fg, kpts, counts, imap, K, kp, check)


# ---- 4. map values at and above the count ---------------------------------------------------------------------------------------------------------
def map_out_of_range():
    rng = np.random.default_rng(14)
    counts = np.int32([[2, 3], [3, 1]])
    out, ce, fg, kpts, counts, imap, K, kp = settle(rng, lambda: _random_inputs(rng, counts, **BASE))
    imap = np.where(rng.random(fg.shape) < 0.4, rng.integers(0, 6, fg.shape), imap).astype(np.uint8)      # also on background: ignored there
    imap[0, 0, 0] = 255

    def check(c, ref):
        r, near = ref(True), ref(False)
        n = np.concatenate([np.zeros((2, 1), np.int64), c.counts], 1)[np.arange(2)[:, None, None], c.labels_fg]
        out_of_range = (c.labels_fg != 0) & (c.imap >= n)
        assert out_of_range[0].sum() >= 20 and out_of_range[1].sum() >= 20 and (c.imap[out_of_range] == n[out_of_range]).any()
        assert not r.fg0[out_of_range].any() and np.array_equal(r.fg0 != 0, (c.labels_fg != 0) & ~out_of_range)
        assert (r.count0 == near.count0 - out_of_range.reshape(2, -1).sum(1)).all()
        assert_margins(c, near)

    return _case("map_out_of_range", out, ce, fg, kpts, counts, imap, K, kp, check)


# ---- 5. a pixel column exactly between two centres --------------------------------------------------------------------------------------------------
def centre_tie():
    """object 1: centres at (10, 8) and (10, 15); the pixels of column 11 have their centres at x = 11.5, 3.5 from both: dy^2 + 3.5^2 is the same
    fp32 number for both, whatever dy.  The first instance wins (tf.argmin)."""
    rng = np.random.default_rng(15)
    b, h, w, K, kp, I = (BASE[k] for k in ("b", "h", "w", "K", "kp", "I"))
    counts = np.int32([[2, 1], [2, 1]])
    kpts = np.zeros((b, K - 1, I, kp, 2), np.float32)
    kpts[:, 0, 0, 0], kpts[:, 0, 1, 0], kpts[:, 1, 0, 0] = (10.0, 8.0), (10.0, 15.0), (19.0, 25.0)
    kpts[:, :, :, 1:] = kpts[:, :, :, :1] + rng.uniform(-12, 12, (b, K - 1, I, kp - 1, 2)).astype(np.float32)
    lab = np.zeros((b, h, w), np.uint8)
    lab[:, 4:16, 4:9], lab[:, 4:16, 11], lab[:, 4:16, 14:19], lab[:, 16:22, 20:30] = 1, 1, 1, 2
    tie = np.zeros((b, h, w), bool)
    tie[:, 4:16, 11] = True

    def make():
        return Cs.random_record(lab, K, kp, False, rng), lab, lab.copy(), kpts, counts, None, K, kp

    out, ce, fg, kpts, counts, imap, K, kp = settle(rng, make, exempt=tie)

    def check(c, ref):
        r = ref(False)
        assert (r.raw.centre_gap[tie] == 0).all() and (r.raw.rv[tie] == 0).all() and tie.sum() == 24
        k32 = c.kpts[0, 0, :2, 0]
        for y in range(4, 16):      # the tie is exact in fp32 as well
            d = [np.float32(y + 0.5 - k32[r_, 0]) ** 2 + np.float32(11.5 - k32[r_, 1]) ** 2 for r_ in (0, 1)]
            assert d[0] == d[1]
        assert (r.raw.rv[:, 4:16, 14:19] == 1).all() and (r.raw.rv[:, 4:16, 4:9] == 0).all()
        assert_margins(c, r, exempt=tie)
        assert (r.raw.proxy_gap[tie] > MARGIN).all()

    return _case("centre_tie", out, ce, fg, kpts, counts, None, K, kp, check, ties=tie)


# ---- 6. two instances' keypoints mirrored about the pixel centre, under the direction (1, 0) ------------------------------------------------------
def proxy_tie():
    """direction (1, 0): num = a_x = k_x - c_x.  Object 1 covers column 9 (c_x = 9.5) only; its two instances' keypoints are 9.5 + d_j and 9.5 - d_j
    with d_j a multiple of 1/4: |num| is the same fp32 number for both, the sign differs, and with it the gradient.  The first instance's is taken."""
    rng = np.random.default_rng(16)
    b, h, w, K, kp, I = (BASE[k] for k in ("b", "h", "w", "K", "kp", "I"))
    counts = np.int32([[2, 1], [2, 1]])
    kpts = rng.uniform(0, 24, (b, K - 1, I, kp, 2)).astype(np.float32)
    dj = (np.arange(kp) * 0.75 + 0.25).astype(np.float32)
    kpts[:, 0, 0, :, 1], kpts[:, 0, 1, :, 1] = 9.5 + dj, 9.5 - dj
    kpts[:, 0, 1, :, 0] = kpts[:, 0, 0, :, 0]
    lab = np.zeros((b, h, w), np.uint8)
    lab[:, 3:20, 9], lab[:, 5:18, 18:28] = 1, 2
    tie = lab == 1
    out = Cs.random_record(lab, K, kp, False, rng)
    out[tie, K:] = np.tile(np.float32([1.0, 0.0]), kp)

    def check(c, ref):
        r = ref(False)
        assert (r.raw.proxy_gap[tie] == 0).all() and (r.raw.rp[tie] == 0).all() and (r.raw.rv[tie] == 0).all() and tie.sum() == 34
        assert (r.raw.dist[tie] == dj.astype(np.float64)).all()
        # the proxy term alone, with the two instances in either order: d/dv_x = -dl * sign(num) * a_y changes its sign with the instance
        other = c.kpts.copy()
        other[:, 0, [0, 1]] = other[:, 0, [1, 0]]
        g, g2 = (R.merged_instances(c.out, c.labels_ce, c.labels_fg, k, c.counts, None, c.K, c.kp, False, False, (0.0, 0.0, 1.0)).grad_dirs.reshape(b, h, w, kp, 2)[tie]
                 for k in (c.kpts, other))
        assert (g[..., 1] == -g2[..., 1]).all() and (g[..., 1] != 0).all() and np.array_equal(g[..., 0], g2[..., 0])

    return _case("proxy_tie", out, lab, lab.copy(), kpts, counts, None, K, kp, check, ties=tie)


# ---- 7. the two filters -----------------------------------------------------------------------------------------------------------------------------
def filters():
    """loss_cases.threshold with an instance axis: direction (1, 0) on 5 x 6 blocks with c_x = 4.5 .. 9.5, so an object's value is
    mean(min over instances |k_x - c_x|) - 0.5.  Image 0: object 1 has instances at k_x = 12.75 and 40 (value 5.25: dropped), object 2 at 41 and
    12.25 (4.75: kept; the nearer one is the SECOND instance).  Image 1: object 1 at 12.25 and 40 (kept), object 2 has 19 pixels and a large error
    (below 20 pixels: value 0, kept).  One whole row of every block has wrong logits: the segmentation filter removes it, and a whole row
    leaves the mean over the columns where it was."""
    rng = np.random.default_rng(17)
    b, h, w, K, kp, I = (BASE[k] for k in ("b", "h", "w", "K", "kp", "I"))
    counts = np.int32([[2, 2], [2, 1]])
    lab = np.zeros((b, h, w), np.uint8)
    lab[:, 3:8, 4:10], lab[0, 12:17, 4:10] = 1, 2
    lab[1, 12:16, 4:9], lab[1, 15, 8] = 2, 0                                              # 19 pixels
    kpts = np.zeros((b, K - 1, I, kp, 2), np.float32)
    kpts[..., 0] = rng.uniform(-10, 40, (b, K - 1, 1, kp))                               # the same rows for every instance: the nearer column decides
    kpts[0, 0, :2, :, 1] = np.float32([12.75, 40.0])[:, None]
    kpts[0, 1, :2, :, 1] = np.float32([41.0, 12.25])[:, None]
    kpts[1, 0, :2, :, 1] = np.float32([12.25, 40.0])[:, None]
    kpts[1, 1, 0, :, 1] = 60.0
    out = Cs.random_record(lab, K, kp, False, rng)
    out[lab != 0, K:] = np.tile(np.float32([1.0, 0.0]), kp)
    Cs.sure_logits(out, K, lab != 0, lab)
    wrong = np.zeros((b, h, w), bool)
    wrong[:, 5, 4:10], wrong[0, 14, 4:10] = True, True
    Cs.sure_logits(out, K, wrong, np.zeros_like(lab))

    def check(c, ref):
        for seg in (False, True):
            r = ref(False, seg, False)
            rows = 4 if seg else 5
            assert r.objcnt.tolist() == [[6 * rows, 6 * rows], [6 * rows, 19]]
            assert 5.05 < r.value[0, 0] < 5.5 and 4.5 < r.value[0, 1] < 4.95 and 4.5 < r.value[1, 0] < 4.95 and r.value[1, 1] == 0 and r.objsum[1, 1] > 5.5 * kp * 19
            assert r.bad.tolist() == [[True, False], [False, False]]
            assert (r.raw.rp[0][r.fg0[0] == 2] == 1).all() and (r.raw.rv[0][r.fg0[0] == 2] == 1).all()
            f = ref(False, seg, True)
            assert not (f.fg1[0] == 1).any() and (f.count1 == [6 * rows, 6 * rows + 19]).all()
            assert_margins(c, r)

    return _case("filters", out, lab, lab.copy(), kpts, counts, None, K, kp, check)


# ---- 8. record shapes and instance counts ---------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = ((3, 9, 1), (3, 9, 2), (3, 9, 16), (13, 4, 1), (13, 4, 2), (13, 4, 16),
                 (13, 9, 16))     # the last: 12 x 16 x 9 x 2 floats, more than the kernel stages in LDS -- its global-memory path


def layouts(K, kp, I):
    rng = np.random.default_rng(1800 + K * 31 + kp * 7 + I)
    b, h, w = 2, 24, 32
    counts = rng.integers(1, I + 1, (b, K - 1)).astype(np.int32)
    counts[0, 0] = I
    out, ce, fg, kpts, counts, imap, K, kp = settle(rng, lambda: _random_inputs(rng, counts, b, h, w, K, kp, I, radius=4.5 if K > 3 else 6.5))

    def check(c, ref):
        r = ref(False, True)
        assert r.raw.on.sum() >= 150 and len(np.unique(r.fg0)) >= min(c.K, 6)
        if c.I > 1:
            assert len(np.unique(r.raw.rv[r.raw.on])) >= 2 and (r.raw.rp[r.raw.on] != r.raw.rv[r.raw.on][:, None]).any()
        assert_margins(c, ref(False))

    return _case("layouts", out, ce, fg, kpts, counts, imap, K, kp, check)


# ---- 9. the second trip of the grid-stride loops -----------------------------------------------------------------------------------------------------
def second_trip():
    """b = 1, 364 x 364: more pixels than 512 blocks of 256 threads.  Object 2's two instances lie in the first trip, object 1's two in the last
    rows, the second trip.  Every keypoint is within 80 px of the pixels that aim at it: the numerator v_y a_x - v_x a_y of an aimed direction is
    the difference of two nearly equal products, whose fp32 rounding is 2^-24 |v| |a|, and where the distance is below 1 px the gradient is
    proportional to it -- so |a| < 80 px keeps that rounding (5e-6 of the block's maximum) well inside the gradient bound of 2e-5, which a
    keypoint 350 px away (2e-5) would not."""
    rng = np.random.default_rng(19)
    b, h, w, K, kp, I = 1, 364, 364, 3, 2, 2
    counts = np.int32([[2, 2]])
    lab = np.zeros((b, h, w), np.uint8)
    imap = np.zeros((b, h, w), np.uint8)
    kpts = np.zeros((b, K - 1, I, kp, 2), np.float32)
    for o, y0, y1 in ((1, 3, 30), (0, h - 6, h)):
        for r, x0 in ((0, 20), (1, 190)):
            lab[0, y0:y1, x0:x0 + 100], imap[0, y0:y1, x0:x0 + 100] = o + 1, r
            kpts[0, o, r, 0] = ((y0 + y1) / 2 + rng.uniform(-2, 2), x0 + 50 + rng.uniform(-5, 5))
            kpts[0, o, r, 1:] = kpts[0, o, r, 0] + rng.uniform(-20, 20, (kp - 1, 2))
    lab[0] *= rng.random((h, w)) < 0.9
    imap *= lab != 0

    def aim(out, where):         # towards the keypoints of the map's instance, so that the proxy-error filter keeps the objects
        tmp = out.copy()
        aimed_directions(rng, tmp, K, kp, kpts, lab, imap, noise=0.005)
        out[where] = tmp[where]

    def make():
        out = Cs.random_record(lab, K, kp, False, rng)
        aim(out, lab != 0)
        return out, lab, lab.copy(), kpts, counts, imap, K, kp

    out, ce, fg, kpts, counts, imap, K, kp = settle(rng, make, aim)

    def check(c, ref):
        assert h * w > Cs.MERGED_GRID_CAP and (h * w) % 256 != 0
        for use_map in (False, True):
            r = ref(use_map, True, True)
            kept = (r.fg1 != 0).reshape(-1)
            assert kept[:Cs.MERGED_GRID_CAP].sum() >= 1000 and kept[Cs.MERGED_GRID_CAP:].sum() >= 200
            for part in (slice(0, Cs.MERGED_GRID_CAP), slice(Cs.MERGED_GRID_CAP, None)):      # both instances in either trip
                assert len(np.unique(r.raw.rv.reshape(-1)[part][kept[part]])) == 2 and not r.bad.any()
        assert_margins(c, ref(False))

    return _case("second_trip", out, ce, fg, kpts, counts, imap, K, kp, check)


BUILDERS = {"two_discs": two_discs, "occluding": occluding, "absent": absent, "map_out_of_range": map_out_of_range, "centre_tie": centre_tie,
            "proxy_tie": proxy_tie, "filters": filters, "second_trip": second_trip}
SMALL = ("two_discs", "occluding", "absent", "map_out_of_range", "centre_tie", "proxy_tie", "filters")


@functools.lru_cache(maxsize=None)
def build(name, *shape):
    return layouts(*shape) if name == "layouts" else BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, shape, use_map, seg, prox):
    return reference_of(build(name, *shape), use_map, seg, prox)


@functools.lru_cache(maxsize=None)
def checked(name, *shape):
    """the case, its properties (and, outside the tie pixels, its margins) asserted on the reference"""
    c = build(name, *shape)
    c.check(c, lambda use_map, seg=False, prox=False: _reference(name, shape, bool(use_map) and c.imap is not None, seg, prox))
    return c


def reference(name, *shape, use_map=False, seg=False, prox=False):
    c = checked(name, *shape)
    return _reference(name, shape, bool(use_map) and c.imap is not None, bool(seg), bool(prox))


def single_instance(c):
    """a case of tests/loss_cases.py with an instance axis of one: what the identity check feeds cp_pose_loss_inst_f32"""
    b = c.labels_fg.shape[0]
    return c.kpts[:, :, None].copy(), np.ones((b, c.K - 1), np.int32)
