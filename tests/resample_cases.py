"""The inputs of the resampling / pooling / label stage tests (test_gpu_resample_stages.py on the GPU, test_resample_reference.py on the CPU).
Every input is chosen for properties that the kernels' shortcuts depend on, and every such property is asserted HERE, on the reference
(tests/resample_reference.py) alone: importing this module evaluates all of them, so a case that lost its property fails before any kernel
output is looked at.  Shapes are (B, H, W, C) of the low-resolution side for the upsamplers and of the input for pooling."""
import functools
from types import SimpleNamespace

import numpy as np

import resample_reference as R

THREADS, GRID_CAP = 256, 2048                  # every kernel here grid-strides over at most 2048 blocks of 256 threads
CAP_ITEMS = THREADS * GRID_CAP                 # 524 288 work items in the first trip of the loop


def past_cap(items):
    """the second trip of the grid-stride loop runs, for at least one partial block"""
    return items >= CAP_ITEMS + THREADS + 1 or (items > CAP_ITEMS + 1 and items % THREADS != 0)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _seed(*key):
    """a generator per case, seeded from the case's name (no hash(): that differs from run to run)"""
    return np.random.default_rng([ord(ch) for ch in str(key)])


# ---- work items per kernel, from the launch line of each extern "C" entry -------------------------------------------------------------------
def items_up_fwd(b, h, w, c):        # cp_upsample_bilinear_x2_f32, cp_guided_upsample_x2_f32, cp_guided_bilinear_upsample_x2_f32
    return b * 4 * h * w * (c // 4)


def items_up_bwd(b, h, w, c):        # the three upsampling adjoints
    return b * h * w * (c // 4)


def items_match_mask(b, h, w):       # low-res size; one item per hi-res pixel
    return b * 2 * h * 2 * w


def items_pool_fwd(b, h, w, c):      # cp_maxpool3x3s2_f32, cp_maxpool3x3s2_idx_f32
    return b * R.pool_size(h) * R.pool_size(w) * (c // 4)


def items_pool_bwd(b, h, w, c):      # cp_maxpool3x3s2_bwd_f32, cp_maxpool3x3s2_bwd_idx_f32: one item per 2x2 input block and channel group
    return b * ((h + 1) // 2) * ((w + 1) // 2) * (c // 4)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
UP_SHAPES = ((1, 1, 1, 4), (1, 1, 5, 4), (2, 5, 1, 12), (2, 3, 4, 12), (2, 7, 9, 64))
CRAFTED_SHAPE = (2, 9, 9, 4)
PYRAMID_SHAPE = (2, 7, 9, 12)
POOL_SHAPES = UP_SHAPES + ((1, 2, 2, 4), (2, 9, 13, 12), (2, 10, 14, 32))
UP_FWD_BIG = (2, 64, 68, 64)          # 557 056 forward items
UP_BWD_BIG = (2, 128, 129, 64)        # 528 384 adjoint items
MASK_BIG = (1, 256, 513)              # 525 312 hi-res pixels
POOL_BIG = (2, 255, 257, 64)          # 128 x 129 outputs and as many 2x2 input blocks: 528 384 items both ways
FLAT_BIG = CAP_ITEMS + 300            # pad 3->4, arg-max, gather, scatter, axpby: one item per pixel / element

assert past_cap(items_up_fwd(*UP_FWD_BIG)) and not past_cap(items_up_bwd(*UP_FWD_BIG))
assert past_cap(items_up_bwd(*UP_BWD_BIG))
assert past_cap(items_match_mask(*MASK_BIG))
assert past_cap(items_pool_fwd(*POOL_BIG)) and past_cap(items_pool_bwd(*POOL_BIG))
assert past_cap(FLAT_BIG)
for _s in UP_SHAPES + (CRAFTED_SHAPE, PYRAMID_SHAPE):
    assert not past_cap(items_up_fwd(*_s))
for _s in POOL_SHAPES:
    assert not past_cap(items_pool_fwd(*_s)) and not past_cap(items_pool_bwd(*_s))


# ---- label pairs for the guided kernels ----------------------------------------------------------------------------------------------------------
def blobs(rng, b, h, w, labels=3):
    """small blobs: a coarse random map, doubled, with a tenth of the pixels redrawn"""
    coarse = rng.integers(0, labels, (b, (h + 1) // 2, (w + 1) // 2))
    m = R.up2(coarse)[:, :h, :w]
    redraw = rng.random((b, h, w)) < 0.1
    return np.where(redraw, rng.integers(0, labels, (b, h, w)), m).astype(np.uint8)


def crafted_labels():
    """(hi, lo) of CRAFTED_SHAPE in which every (mask, sub-pixel) combination that can occur does occur, at every kind of position: a cell whose
    four hi-res pixels carry label 1 and whose taps carry 1 where the mask has a bit and 2 elsewhere.  Cells sit two apart so that their taps
    do not overlap: 16 interior cells, 4 cells in the last column (taps 1 and 3 are padding), 4 in the last row (taps 2 and 3), and the corner
    cell (only tap 0 exists), whose two masks take one image each."""
    b, h, w, _ = CRAFTED_SHAPE
    lo = np.full((b, h, w), 2, np.uint8)
    hi = np.zeros((b, 2 * h, 2 * w), np.uint8)

    def cell(n, y, x, mask):
        hi[n, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = 1
        for j, (dy, dx) in enumerate(R.TAPS):
            if y + dy < h and x + dx < w:
                lo[n, y + dy, x + dx] = 1 if (mask >> j) & 1 else 2

    for n in range(b):
        for m in range(16):
            cell(n, 2 * (m // 4), 2 * (m % 4), m)
        for k, m in enumerate((0, 1, 4, 5)):
            cell(n, 2 * k, w - 1, m)
        for k, m in enumerate((0, 1, 2, 3)):
            cell(n, h - 1, 2 * k, m)
        cell(n, h - 1, w - 1, n)
    return hi, lo


def position_kind(h, w):
    """[2h, 2w]: 0 interior cell, 1 last column, 2 last row, 3 bottom-right corner cell"""
    yy, xx = np.meshgrid(np.arange(2 * h) // 2, np.arange(2 * w) // 2, indexing="ij")
    return (xx == w - 1) * 1 + (yy == h - 1) * 2


POSSIBLE_MASKS = {0: range(16), 1: (0, 1, 4, 5), 2: (0, 1, 2, 3), 3: (0, 1)}     # padding taps never match


def combos(mask):
    """{(kind, mask, sub-pixel)} that occur in one reference mask"""
    _, hh, ww = mask.shape
    kind, sub = position_kind(hh // 2, ww // 2), R.sub_pixel(hh // 2, ww // 2)
    code = (kind[None] * 16 + mask.astype(np.int64)) * 4 + sub[None]
    return {(int(v) // 64, (int(v) // 4) % 16, int(v) % 4) for v in np.unique(code)}


@functools.lru_cache(maxsize=None)
def guided(name):
    """one label pair with everything the guided tests need from the reference: mask, sel, and float data x (low-res), dy (hi-res, small integers)"""
    shape = dict(GUIDED_SHAPES)[name]
    b, h, w, c = shape
    rng = _seed("guided", name)
    if name == "crafted":
        hi, lo = crafted_labels()
    elif name == "pyramid":
        hi = blobs(rng, b, 2 * h, 2 * w)
        lo = hi[:, ::2, ::2]
    else:
        hi, lo = blobs(rng, b, 2 * h, 2 * w), blobs(rng, b, h, w)
    mask, sel = R.match_mask(hi, lo), R.sel_map(hi, lo)
    # what both label rules promise, whatever the map: a padding tap matches nothing, and sel is the lowest set bit of the mask (0 if none)
    kind = position_kind(h, w)
    for k, allowed in POSSIBLE_MASKS.items():
        assert np.isin(mask[:, kind == k], list(allowed)).all(), name
    low_bit = np.array([0] + [(m & -m).bit_length() - 1 for m in range(1, 16)], np.uint8)
    assert np.array_equal(sel, low_bit[mask]), name
    x = rng.standard_normal((b, h, w, c)).astype(np.float32)
    dy = rng.standard_normal((b, 2 * h, 2 * w, c)).astype(np.float32)
    dy_int = rng.integers(-4, 5, (b, 2 * h, 2 * w, c)).astype(np.float32)
    return SimpleNamespace(name=name, shape=shape, hi=_ro(hi), lo=_ro(lo), mask=_ro(mask), sel=_ro(sel), x=_ro(x), dy=_ro(dy), dy_int=_ro(dy_int))


GUIDED_SHAPES = tuple(("independent_%dx%dx%dx%d" % s, s) for s in UP_SHAPES) + (("crafted", CRAFTED_SHAPE), ("pyramid", PYRAMID_SHAPE))
GUIDED_NAMES = tuple(n for n, _ in GUIDED_SHAPES)
INDEPENDENT = tuple(n for n in GUIDED_NAMES if n != "pyramid")          # lo and hi drawn (or crafted) independently
GUIDED_SHAPES += (("big_fwd", UP_FWD_BIG), ("big_bwd", UP_BWD_BIG))     # past the cap: used by the GPU tests only, built on demand


def check_guided_coverage():
    seen = set()
    for name in INDEPENDENT:
        seen |= combos(guided(name).mask)
    want = {(k, m, s) for k, masks in POSSIBLE_MASKS.items() for m in masks for s in range(4)}
    assert len([c for c in want if c[0] == 0]) == 64
    assert want <= seen, sorted(want - seen)
    assert seen <= want
    # with lo = hi[::2, ::2] tap 0 always matches at sub-pixel 0 and the no-match case needs an odd sub-pixel: the pair the engines feed reaches
    # a strict subset, which is why the independent pairs exist
    pyr = combos(guided("pyramid").mask)
    assert pyr < want and all(m & 1 for _, m, s in pyr if s == 0)
    none = [c for c in seen if c[1] == 0]
    assert {s for _, _, s in none} == {0, 1, 2, 3}


check_guided_coverage()


# ---- max-pool inputs ---------------------------------------------------------------------------------------------------------------------------------
POOL_KINDS = ("relu", "negative", "neg_inf")


@functools.lru_cache(maxsize=None)
def pool(shape, kind):
    b, h, w, c = shape
    rng = _seed("pool", shape, kind)
    n = rng.standard_normal((b, h, w, c))
    if kind == "relu":            # post-ReLU, quantised to halves: exact ties and exact zeros are common
        x = np.round(np.maximum(n - 0.5, 0.0) * 2) / 2
    elif kind == "negative":      # strictly negative: the padding wins on the border, the interior maximum stays negative
        x = -(np.round(np.abs(n) * 2) / 2 + 0.5)
    else:                         # -inf entries, a whole interior window of them where the map is large enough
        x = np.round(n * 2) / 2 + 0.0
        x[rng.random(x.shape) < 0.3] = -np.inf
        if h >= 7 and w >= 7:
            x[:, 2:7, 2:7, :] = -np.inf          # windows (2,2) are all -inf: caught cp_maxpool3x3s2_bwd_f32 dropping their gradient
    x = x.astype(np.float32) + np.float32(0.0)    # no -0.0
    assert not np.signbit(x[x == 0]).any()
    ho, wo = R.pool_size(h), R.pool_size(w)
    dy = rng.integers(-4, 5, (b, ho, wo, c)).astype(np.float32)
    dx_prev = rng.integers(-8, 9, (b, h, w, c)).astype(np.float32)
    return SimpleNamespace(shape=shape, kind=kind, x=_ro(x), dy=_ro(dy), dx_prev=_ro(dx_prev))


def pool_conditions(shape, kind):
    """counts, on the reference, of the windows each kind of map exists for"""
    case = pool(shape, kind)
    r = R.maxpool(case.x)
    is_max = r.win == r.val[:, :, :, None, :]
    inside = r.inside[None, :, :, :, None]
    first = r.idx.astype(np.int64)[:, :, :, None, :]
    taps = np.arange(9)[None, None, None, :, None]
    return SimpleNamespace(
        tied_inside=int(((is_max & inside).sum(3) >= 2).sum()),
        pad_first=int(r.pad_wins.sum()),
        pad_later=int((~r.pad_wins & (r.val == 0) & (is_max & ~inside & (taps > first)).any(3)).sum()),
        all_neg_inf=int((r.val == -np.inf).sum()),
        negative_max=int((r.val < 0).sum()))


def check_pool_conditions():
    for shape in POOL_SHAPES:
        for kind in POOL_KINDS:
            pool_conditions(shape, kind)                      # every case evaluates
    for shape in ((2, 7, 9, 64), (2, 9, 13, 12), (2, 10, 14, 32)):
        c = pool_conditions(shape, "relu")
        assert c.tied_inside >= 100 and c.pad_first >= 20, (shape, vars(c))
        # a padded tap comes AFTER an in-image tap only in the last row / column of windows of an odd-sized map (an even size has no padding
        # at the bottom / right, and at the top / left the padding is tap 0)
        assert (c.pad_later >= 20) if shape[1] % 2 and shape[2] % 2 else (c.pad_later == 0), (shape, vars(c))
        c = pool_conditions(shape, "negative")
        assert c.pad_first >= 100 and c.negative_max >= 20, (shape, vars(c))
        c = pool_conditions(shape, "neg_inf")
        assert c.all_neg_inf >= 4 and c.tied_inside >= 20, (shape, vars(c))
    # a single cell: the eight other taps are padding, and tap 0 is one of them
    assert pool_conditions((1, 1, 1, 4), "negative").pad_first == 4


check_pool_conditions()


# ---- arg-max -------------------------------------------------------------------------------------------------------------------------------------------
ARGMAX_CLASSES = (1, 2, 4, 5, 9, 12, 13, 40)
ARGMAX_LDS = (12, 13, 16, 20, 40)              # and ld = classes
ARGMAX_OFFSETS = (0, 1, 4)
ARGMAX_PIXELS = 300                            # two blocks, the second partial
BEYOND = np.float32(3e38)                      # what lies in the record past `classes`: larger than every finite logit


def argmax_configs():
    """(classes, ld, offset): as ops.argmax_labels slices a record, offset + classes <= ld"""
    out = []
    for k in ARGMAX_CLASSES:
        for ld in sorted(set((k,) + ARGMAX_LDS)):
            for off in ARGMAX_OFFSETS:
                if ld >= k and off + k <= ld:
                    out.append((k, ld, off))
    return out


def argmax_route(classes, ld, offset, base_alignment=256):
    """the route rule in the header comment of cp_argmax_labels, for a base pointer aligned to `base_alignment` bytes"""
    aligned = (base_alignment % 16 == 0) and (4 * offset) % 16 == 0
    return "vector" if ld % 4 == 0 and aligned and classes <= 12 and 4 * ((classes + 3) // 4) <= ld else "scalar"


@functools.lru_cache(maxsize=None)
def argmax_case(classes, ld, offset, pixels=ARGMAX_PIXELS):
    """A flat float32 buffer of pixels * ld + offset values; the kernel is handed buffer + offset, so pixel i's logits are
    buffer[offset + i * ld + k], k < classes, and the `ld - classes` values after them (the rest of the record and the head of the next one)
    hold BEYOND, or +inf in the rows that plant +inf.  `planted`: {property: row}."""
    rng = _seed("argmax", classes, ld, offset, pixels)
    rows = np.round(rng.standard_normal((pixels, classes)) * 2) / 2 + 0.0        # quantised: chance ties as well
    planted = {}

    def plant(name, values):
        r = len(planted)
        rows[r] = values
        planted[name] = r

    def tie(a, b):
        v = np.full(classes, -1.0)
        v[[a, b]] = 2.0
        return v

    if classes >= 2:
        plant("tie_first_last", tie(0, classes - 1))
        v = np.full(classes, -1.0)
        v[0], v[1] = -0.0, 0.0
        plant("neg_zero_then_zero", v)
        v = np.full(classes, -1.0)
        v[classes - 2], v[classes - 1] = 0.0, -0.0
        plant("zero_then_neg_zero", v)
        v = np.full(classes, -np.inf)
        v[classes - 1] = -7.0
        plant("finite_among_neg_inf", v)
    if classes >= 5:
        plant("tie_3_4", tie(3, 4))
    if classes >= 9:
        plant("tie_7_8", tie(7, 8))
    v = np.arange(classes, dtype=np.float64)
    plant("max_at_last", v)
    plant("all_neg_inf", np.full(classes, -np.inf))
    v = np.full(classes, 1.0)
    v[[classes // 2, classes - 1]] = np.inf
    plant("pos_inf_twice", v)
    buf = np.empty(pixels * ld + offset, np.float32)
    buf[:offset] = BEYOND
    view = buf[offset:].reshape(pixels, ld)
    view[:, classes:] = BEYOND
    view[planted["pos_inf_twice"], classes:] = np.inf
    view[:, :classes] = rows
    assert not np.isnan(buf).any()
    want = R.argmax_labels(view, classes)
    # the planted properties, on the reference
    assert (view[:, classes:] > np.where(np.isfinite(rows), rows, -1.0).max(1, keepdims=True)).all()
    if classes >= 2:
        assert want[planted["tie_first_last"]] == 0 and want[planted["neg_zero_then_zero"]] == 0
        assert want[planted["zero_then_neg_zero"]] == classes - 2 and want[planted["finite_among_neg_inf"]] == classes - 1
    if classes >= 5:
        assert want[planted["tie_3_4"]] == 3
    if classes >= 9:
        assert want[planted["tie_7_8"]] == 7
    assert want[planted["max_at_last"]] == classes - 1 and want[planted["all_neg_inf"]] == 0 and want[planted["pos_inf_twice"]] == classes // 2
    return SimpleNamespace(classes=classes, ld=ld, offset=offset, pixels=pixels, buffer=_ro(buf), want=_ro(want), planted=planted,
                           route=argmax_route(classes, ld, offset))


def check_argmax_routes():
    by_route = {"vector": set(), "scalar": set()}
    for cfg in argmax_configs():
        case = argmax_case(*cfg)
        by_route[case.route] |= set(case.planted)
        by_route[case.route].add("classes_%d" % case.classes)
    everything = set(argmax_case(40, 40, 0).planted)
    assert by_route["scalar"] == everything | {"classes_%d" % k for k in ARGMAX_CLASSES}      # offsets, odd ld, and more than 12 classes
    assert by_route["vector"] == everything | {"classes_%d" % k for k in ARGMAX_CLASSES if k <= 12}
    assert argmax_route(9, 12, 0) == "vector" and argmax_route(9, 12, 1) == "scalar" and argmax_route(9, 13, 0) == "scalar"
    assert argmax_route(13, 16, 0) == "scalar" and argmax_route(5, 5, 0) == "scalar" and argmax_route(4, 4, 0) == "vector"


check_argmax_routes()


# ---- gather / scatter / axpby / pad ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flat(n):
    """n elements: an injective index into 2n targets with a tenth of the entries -1, integer-valued sources"""
    rng = _seed("flat", n)
    idx = rng.permutation(2 * n)[:n].astype(np.int32)
    idx[rng.random(n) < 0.1] = -1
    assert (n < 100 or (idx == -1).sum() > 0) and len(np.unique(idx[idx >= 0])) == (idx >= 0).sum()
    src = rng.integers(-100, 101, n).astype(np.float32)
    table = rng.integers(-100, 101, 2 * n).astype(np.float32)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    rgb = rng.standard_normal((n, 3)).astype(np.float32)
    return SimpleNamespace(n=n, idx=_ro(idx), src=_ro(src), table=_ro(table), a=_ro(a), b=_ro(b), rgb=_ro(rgb))


FLAT_SIZES = (1, 255, 700, FLAT_BIG)


@functools.lru_cache(maxsize=None)
def mask_big():
    """an independent label pair past the cap of cp_guided_match_mask (labels only: no float data)"""
    b, h, w = MASK_BIG
    rng = _seed("mask_big")
    return SimpleNamespace(hi=_ro(blobs(rng, b, 2 * h, 2 * w)), lo=_ro(blobs(rng, b, h, w)))
