"""The label maps of the connected-component stage tests (test_gpu_ccl_stages.py on the GPU, test_ccl_reference.py against the oracle on the CPU).
Every map is chosen for properties that the kernel's shortcuts depend on; `check(case, ref)` asserts those properties on the REFERENCE result
(tests/ccl_reference.py), so a map that no longer has them fails before any kernel output is looked at.  The kernel's tiles are 64 wide and 16
high; the standard map is 70x200: 5 tile rows by 4 tile columns, the last row 6 pixels high, the last column 8 pixels wide."""
import functools
from types import SimpleNamespace

import numpy as np

import ccl_reference as R

TW, TH = 64, 16
H, W = 70, 200
HW = H * W


def tiles_touched(mask):
    ys, xs = np.nonzero(mask)
    return len(set(zip((ys // TH).tolist(), (xs // TW).tolist())))


def comps_of(ref, n, o=None):
    """[(root, size)] of image n (of object o only, if given), in raster order of the first pixel"""
    lab, root = ref.case.labels[n], ref.root[n]
    m = root >= 0 if o is None else (lab == o) & (root >= 0)
    return [(int(r), int(ref.sizes[r])) for r in np.unique(root[m])]


def largest(ref, n, o=None):
    return max(comps_of(ref, n, o), key=lambda c: (c[1], -c[0]))


def spiral(h, w, pitch):
    """a one-pixel-wide rectangular spiral from the corner inwards, `pitch - 1` free pixels between its turns"""
    m = np.zeros((h, w), bool)
    y = x = d = stuck = 0
    m[0, 0] = True
    while stuck < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        ny, nx = y + dy, x + dx
        free = 0 <= ny < h and 0 <= nx < w and not m[ny, nx]
        for k in range(1, pitch):
            ay, ax = ny + dy * k, nx + dx * k
            free = free and not (0 <= ay < h and 0 <= ax < w and m[ay, ax])
        if free:
            y, x, stuck = ny, nx, 0
            m[y, x] = True
        else:
            d, stuck = (d + 1) % 4, stuck + 1
    return m


# min_size 50 (the voter's) on every map; 1 and 7 as well where the sizes are made for it
MIN_SIZES = {"selection_edges": (50, 1, 7), "objects_254": (1, 50), "objects_1": (1, 50), "objects_254_map_with_one_object": (1, 50)}


def _case(name, labels, objects, check):
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    labels.setflags(write=False)
    return SimpleNamespace(name=name, labels=labels, objects=objects, check=check, min_sizes=MIN_SIZES.get(name, (50,)))


# ---- 1. percolation, one label ----------------------------------------------------------------------------------------------------------------------
PERCOLATION = ((0.59, 0), (0.59, 1), (0.59, 2), (0.62, 0))


def percolation():
    lab = np.stack([np.random.default_rng(seed).random((H, W)) < p for p, seed in PERCOLATION])

    def check(case, ref):
        kept = R.filter(case.labels, 1, 50, 1)
        for n, (p, _) in enumerate(PERCOLATION):
            r, size = largest(ref, n)
            assert tiles_touched(ref.root[n] == r) >= 12 and len(comps_of(ref, n)) >= 300, (n, size)
            background = HW - int((case.labels[n] == 1).sum())
            if p == 0.59:
                assert 50 <= size < background and np.array_equal(kept[n] > 0, ref.root[n] == r), (n, size, background)
            else:
                assert size > background and not kept[n].any(), (n, size, background)

    return _case("percolation", lab, 1, check)


# ---- 2. percolation, three labels; stripes ---------------------------------------------------------------------------------------------------------------
def three_labels():
    rng = np.random.default_rng(20)
    lab = np.zeros((2, H, W), np.uint8)
    lab[0] = (rng.random((H, W)) < 0.9) * rng.integers(1, 4, (H, W))
    lab[1] = 1 + (np.arange(W) % 2)[None, :]          # one-pixel vertical stripes, labels 1 and 2 in turn

    def check(case, ref):
        assert sorted(np.unique(case.labels[0]).tolist()) == [0, 1, 2, 3] and len(comps_of(ref, 0)) >= 300
        stripes = comps_of(ref, 1)
        assert [r - HW for r, _ in stripes] == list(range(W)) and {s for _, s in stripes} == {H}     # every stripe on its own

    return _case("three_labels", lab, 3, check)


# ---- 3. spirals ----------------------------------------------------------------------------------------------------------------------------------------
def spirals():
    lab = np.zeros((2, H, W), np.uint8)
    one = spiral(H, W, 4)
    lab[0][one] = 1
    lab[1][one] = 1
    two = np.zeros((H, W), bool)
    two[2:H - 2, 2:W - 2] = spiral(H - 4, W - 4, 4)     # in the gaps of the first
    assert not (one & two).any()
    lab[1][two] = 2

    def check(case, ref):
        for n, o in ((0, 1), (1, 1), (1, 2)):
            (r, size), = comps_of(ref, n, o)              # a single component ...
            assert tiles_touched(ref.root[n] == r) == 20 and 3000 <= size < HW - size, (n, o, size)   # ... through all tiles, below the background
        assert np.array_equal(R.filter(case.labels, 2, 50, 1), case.labels)     # so every spiral is kept

    return _case("spirals", lab, 2, check)


# ---- 4. combs ------------------------------------------------------------------------------------------------------------------------------------------
def combs():
    lab = np.zeros((3, H, W), np.uint8)
    lab[0, :, 0::2] = 1
    lab[0, H - 1, :] = 1                 # teeth on every second column, joined only by the last row (in the ragged tile row)
    lab[1, :, 0::2] = 1
    lab[1, 0, :] = 1                     # joined only by the first row
    lab[2, 2:, 0::4] = 1
    lab[2, H - 1, :] = 1                 # label 1: joined by the last row ...
    lab[2, :H - 2, 2::4] = 2
    lab[2, 0, :] = 2                     # ... interleaved with label 2, joined by the first row
    joins = {0: [H - 1], 1: [0], 2: [0, H - 1]}

    def check(case, ref):
        for n, objs in ((0, 1), (1, 1), (2, 2)):
            assert len(comps_of(ref, n)) == objs
            cut = np.array(case.labels[n:n + 1])
            cut[0, joins[n], :] = 0
            assert int((R.components(cut, 2)[1] > 0).sum()) >= 90

    return _case("combs", lab, 2, check)


def combs_sideways():
    """200x70 (13 ragged tile rows by 2 tile columns, the last 6 wide): horizontal teeth, joined only by the last / the first column"""
    lab = np.zeros((2, W, H), np.uint8)
    lab[0, 0::2, :] = 1
    lab[0, :, H - 1] = 1
    lab[1, 0::2, :] = 2
    lab[1, :, 0] = 2

    def check(case, ref):
        for n, col in ((0, H - 1), (1, 0)):
            assert len(comps_of(ref, n)) == 1
            cut = np.array(case.labels[n:n + 1])
            cut[0, :, col] = 0
            assert int((R.components(cut, 2)[1] > 0).sum()) >= 90

    return _case("combs_sideways", lab, 2, check)


# ---- 5. U and W shapes inside one tile -------------------------------------------------------------------------------------------------------------
U = np.array([[1, 0, 0, 0, 1]] * 4 + [[1, 1, 1, 1, 1]], bool)                     # two runs per row that meet only in the last row
WW = np.array([[1, 0, 1, 0, 0, 1, 0, 1]] * 2 + [[1, 0, 1, 1, 1, 1, 0, 1]] * 2 + [[1, 0, 0, 1, 0, 0, 0, 1]] + [[1] * 8], bool)   # a U inside a U, joined below
# where the shapes END (row, column, exclusive): at tile corners, at last rows and last columns of tiles, in the ragged last tile, and inside
SHAPE_END = ((6, 8), (9, 38), (16, 64), (6, 64), (26, 78), (32, 128), (56, 192), (70, 200), (70, 108), (43, 72), (54, 9))


def shapes_in_a_tile():
    lab = np.zeros((2, H, W), np.uint8)
    placed = []
    for k, (yb, xb) in enumerate(SHAPE_END):
        for n, s in ((0, U if k % 2 else WW), (1, WW if k % 2 else U)):
            sh, sw = s.shape
            y0, x0 = yb - sh, xb - sw
            assert not lab[n, y0:y0 + sh, x0:x0 + sw].any()
            lab[n, y0:y0 + sh, x0:x0 + sw][s] = 1 + (k + n) % 2
            placed.append((n, y0, x0, sh, sw, int(s.sum())))

    def check(case, ref):
        assert len(comps_of(ref, 0)) == len(comps_of(ref, 1)) == len(SHAPE_END)
        last_row = last_col = 0
        for n, y0, x0, sh, sw, size in placed:
            box = ref.root[n, y0:y0 + sh, x0:x0 + sw]
            assert len(np.unique(box[box >= 0])) == 1 and int((box >= 0).sum()) == size          # one component each
            assert y0 // TH == (y0 + sh - 1) // TH and x0 // TW == (x0 + sw - 1) // TW               # inside one tile
            last_row += (y0 + sh) % TH == 0 or y0 + sh == H
            last_col += (x0 + sw) % TW == 0 or x0 + sw == W
        assert last_row >= 6 and last_col >= 6

    return _case("shapes_in_a_tile", lab, 2, check)


# ---- 6. checkerboard; one label everywhere -----------------------------------------------------------------------------------------------------------
def checkerboard():
    lab = np.zeros((2, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    lab[0] = (yy + xx) % 2 == 0
    lab[1] = 1

    def check(case, ref):
        assert len(comps_of(ref, 0)) == HW // 2 and comps_of(ref, 1) == [(HW, HW)]
        for rank in (1, 2):
            kept = R.filter(case.labels, 1, 50, rank)
            want = np.zeros((H, W), bool)
            want[(0, 0) if rank == 1 else (0, 2)] = True      # every bin below 50: the first (second) pixel in raster order
            assert np.array_equal(kept[0] > 0, want) and not kept[1].any()

    return _case("checkerboard", lab, 1, check)


# ---- 7. selection edges, from boxes ---------------------------------------------------------------------------------------------------------------------
def selection_edges():
    lab = np.zeros((2, H, W), np.uint8)
    lab[0, 2:8, 2:12] = 1            # 60
    lab[0, 40:50, 150:156] = 1       # 60: the first in raster order wins
    lab[0, 2:9, 20:27] = 2           # 49, first in raster order
    lab[0, 30:35, 60:70] = 2         # 50
    lab[0, 2:10, 40:50] = 3          # 80
    lab[0, 20:28, 100:110] = 3       # 80
    lab[0, 60:66, 180:190] = 3       # 60
    lab[0, 12:20, 62:66] = 4         # one component only (32 px, across a tile corner)
    lab[0, 2:4, 120:123] = 5         # 6, first in raster order
    lab[0, 50, 10:17] = 5            # 7
    lab[1, H // 2:, :] = 6           # exactly half of the image in an otherwise empty one

    def check(case, ref):
        sel = lambda n, o, m, rank: R.select(comps_of(ref, n, o), HW, m, rank)      # noqa: E731
        first = lambda n, o: comps_of(ref, n, o)[0][0]                               # noqa: E731
        assert [s for _, s in comps_of(ref, 0, 1)] == [60, 60] and sel(0, 1, 50, 1) == (first(0, 1), 60)
        assert [s for _, s in comps_of(ref, 0, 2)] == [49, 50] and sel(0, 2, 50, 1)[1] == 50 and sel(0, 2, 50, 2) == (first(0, 2), 0)
        assert [s for _, s in comps_of(ref, 0, 3)] == [80, 80, 60] and sel(0, 3, 50, 2) == (comps_of(ref, 0, 3)[1][0], 80)
        assert len(comps_of(ref, 0, 4)) == 1 and sel(0, 4, 50, 2) == (None, 0) and sel(0, 4, 1, 1) == (first(0, 4), 32)
        assert [s for _, s in comps_of(ref, 0, 5)] == [6, 7] and sel(0, 5, 7, 1)[1] == 7 and sel(0, 5, 50, 1) == (first(0, 5), 0)
        assert comps_of(ref, 1, 6) == [(HW + HW // 2, HW // 2)] and sel(1, 6, 50, 1) == (HW + HW // 2, HW // 2)    # bin 0 wins the tie
        assert sel(1, 6, 50, 2) == (None, 0) and sel(1, 1, 50, 1) == (None, 0)

    return _case("selection_edges", lab, 6, check)


# ---- 8. objects at the limit ----------------------------------------------------------------------------------------------------------------------------
def _blocks(cell_labels, h=32, w=64):
    lab = np.zeros((h, w), np.uint8)
    for k, l in cell_labels.items():
        y, x = divmod(k, w // 2)
        lab[2 * y:2 * y + 2, 2 * x:2 * x + 2] = l
    return lab


def objects_254():
    one = {k: k + 1 for k in range(254)}
    one.update({254 + j: 2 * j + 1 for j in range(127)})          # the odd labels have a second block
    lab = np.stack([_blocks(one), _blocks({k: 254 - k for k in range(254)})])

    def check(case, ref):
        assert sorted(np.unique(case.labels).tolist()) == list(range(255))
        for o in range(1, 255):
            assert [s for _, s in comps_of(ref, 0, o)] == [4] * (2 if o % 2 else 1) and [s for _, s in comps_of(ref, 1, o)] == [4], o

    return _case("objects_254", lab, 254, check)


def objects_1():
    lab = np.stack([_blocks({k: 1 for k in range(512) if (k + k // 32) % 2 == 0}), _blocks({k: 1 for k in (0, 5, 300, 511)})])

    def check(case, ref):
        assert len(comps_of(ref, 0)) == 256 and len(comps_of(ref, 1)) == 4 and {s for _, s in comps_of(ref, 0)} == {4}

    return _case("objects_1", lab, 1, check)


# ---- 9. labels above `objects` ---------------------------------------------------------------------------------------------------------------------------
def labels_out_of_range():
    rng = np.random.default_rng(9)
    lab = np.zeros((2, H, W), np.uint8)
    lab[0, 5:30, 10:90] = 1
    lab[0, 5:30, 90:120] = 3         # between two parts of label 1
    lab[0, 5:30, 120:150] = 1
    lab[0, 30:40, 10:150] = 255      # touches 1, 3 and 2
    lab[0, 40:60, 10:150] = 2
    lab[0, 62:70, 190:200] = 255     # the image's last pixels
    lab[1] = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), (H, W), p=[0.2, 0.3, 0.3, 0.1, 0.1])
    lab[1, H - 1, W - 4:] = (3, 255, 254, 255)

    def check(case, ref):
        bad = case.labels > 2
        assert bad[0].sum() > 1000 and bad[1].sum() > 1000 and set(np.unique(case.labels[bad]).tolist()) == {3, 254, 255}
        assert bad[0, 29:31, 90].all() and case.labels[0, 29, 89] == 1 and case.labels[0, 40, 90] == 2       # the regions touch
        zeroed = np.where(bad, 0, case.labels).astype(np.uint8)
        root0, sizes0 = R.components(zeroed, 2)
        assert np.array_equal(ref.root, root0) and np.array_equal(ref.sizes, sizes0) and (ref.root[bad] == -1).all()
        for rank in (1, 2):
            kept = R.filter(case.labels, 2, 50, rank)
            assert np.array_equal(kept, R.filter(zeroed, 2, 50, rank)) and not kept[bad].any()
        assert [s for _, s in comps_of(ref, 0, 1)] == [2000, 750]     # label 3 does not bridge the two parts of label 1

    return _case("labels_out_of_range", lab, 2, check)


def objects_254_map_with_one_object():
    """the 254-label map read with objects = 1: everything but label 1 is out of range"""
    lab = objects_254().labels

    def check(case, ref):
        assert [len(comps_of(ref, n)) for n in (0, 1)] == [2, 1] and int((ref.root >= 0).sum()) == 12

    return _case("objects_254_map_with_one_object", lab, 1, check)


# ---- 10. degenerate geometries ---------------------------------------------------------------------------------------------------------------------------
def degenerate(h, w):
    lab = np.zeros((2, h, w), np.uint8)
    if h == 1 and w == 1:
        lab[0] = 1
    elif h == 1:
        lab[0, 0, 10:81], lab[0, 0, 81:101], lab[0, 0, 120:130] = 1, 2, 1       # runs across x = 64 and x = 128
        lab[1, 0, 0:64], lab[1, 0, 64:128], lab[1, 0, 129] = 2, 1, 2              # runs that end at the tile borders
    elif w == 1:
        lab[0, 3:21, 0], lab[0, 21:36, 0], lab[0, 38:40, 0] = 1, 2, 1           # runs across y = 16 and y = 32
        lab[1, 0:16, 0], lab[1, 16:32, 0], lab[1, 39, 0] = 2, 1, 2
    else:
        rng = np.random.default_rng(h * 1000 + w)
        lab[:] = (rng.random((2, h, w)) < 0.62) * rng.integers(1, 3, (2, h, w))
        lab[0, h - 1, :] = 1
        lab[0, :, w - 1] = 1                                                      # (17, 65): a tile row and a tile column of one pixel
        lab[1, :h - 1, w - 1] = 2

    def check(case, ref):
        sizes = [[s for _, s in comps_of(ref, n)] for n in (0, 1)]
        if (h, w) == (1, 1):
            assert sizes == [[1], []]
        elif h == 1:
            assert sizes == [[71, 20, 10], [64, 64, 1]]
        elif w == 1:
            assert sizes == [[18, 15, 2], [16, 16, 1]]
        else:
            assert len(sizes[0]) >= 20 and len(sizes[1]) >= 20 and largest(ref, 0)[1] >= h + w - 1

    return _case("degenerate_%dx%d" % (h, w), lab, 2, check)


DEGENERATE = ((1, 130), (40, 1), (1, 1), (16, 64), (17, 65))


# ---- 11. the second trip of ccl_flatten_count's grid-stride loop ---------------------------------------------------------------------------------------
GRID_CAP_PIXELS = 256 * 16 * 256      # grid_for() in csrc/ccl.hip: at most 256 * 16 blocks of THREADS = 256
BIG_B, BIG_H, BIG_W = 3, 601, 599     # 1 079 997 pixels; 601 * 599 = 359 999 is odd: the image boundaries fall inside a wave and inside a block


def second_trip():
    h, w, hw = BIG_H, BIG_W, BIG_H * BIG_W
    rng = np.random.default_rng(11)
    lab = np.zeros((BIG_B, h, w), np.uint8)
    lab[0] = rng.random((h, w)) < 0.59
    yy, xx = np.mgrid[0:h, 0:w]
    blob = ((yy - 300) / 290.0) ** 2 + ((xx - 300) / 285.0) ** 2 < 1.0
    lab[1] = (rng.random((h, w)) < 0.5) * rng.integers(1, 4, (h, w))
    lab[1][blob] = 2
    lab[2] = (rng.random((h, w)) < 0.6) * rng.integers(1, 4, (h, w))
    lab[2, h - 30:, 100:500] = 3      # a root that dominates whole blocks, in the pixels of the second trip

    def check(case, ref):
        total = BIG_B * hw
        assert total > GRID_CAP_PIXELS and hw % 64 != 0 and (2 * hw) % 64 != 0 and hw % 256 != 0
        assert len(comps_of(ref, 0)) >= 300 and largest(ref, 0)[1] < hw - int((case.labels[0] > 0).sum())
        assert largest(ref, 1)[1] > 0.6 * hw
        second = ref.root.ravel()[GRID_CAP_PIXELS:]
        assert (second >= 2 * hw).all() or (second == -1).any()
        dominant = np.bincount(second[second >= 0] - 2 * hw).max()
        assert dominant >= 256 * 30 and len(np.unique(second[second >= 0])) >= 1000     # whole blocks of one root, and noise, in the second trip

    return _case("second_trip", lab, 3, check)


BUILDERS = {"percolation": percolation, "three_labels": three_labels, "spirals": spirals, "combs": combs, "combs_sideways": combs_sideways,
            "shapes_in_a_tile": shapes_in_a_tile, "checkerboard": checkerboard, "selection_edges": selection_edges, "objects_254": objects_254,
            "objects_1": objects_1, "labels_out_of_range": labels_out_of_range, "objects_254_map_with_one_object": objects_254_map_with_one_object,
            "second_trip": second_trip}
BUILDERS.update({"degenerate_%dx%d" % hw_: functools.partial(degenerate, *hw_) for hw_ in DEGENERATE})
NAMES = tuple(BUILDERS)
SMALL = tuple(n for n in NAMES if n != "second_trip")       # no larger than 70x200 (or 200x70): what the oracle's Python flood fill can afford


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case with its reference components, its input properties asserted: SimpleNamespace(case, root, sizes)"""
    case = BUILDERS[name]()
    root, sizes = R.components(case.labels, case.objects)
    root.setflags(write=False)
    sizes.setflags(write=False)
    ref = SimpleNamespace(case=case, root=root, sizes=sizes)
    case.check(case, ref)
    return ref
