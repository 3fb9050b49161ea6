"""tests/vote_split_reference.py, the NumPy restatement of cp_vote_split_labels' rule (include/casapose_hip.h), pinned by hand on maps of a few
pixels and on hand-written grids, and the conditions of the planted scenes (tests/vote_split_cases.py) evaluated on the reference alone.  The GPU
test then asks the kernels to equal the reference, which makes these conditions hold on the device.  No GPU."""
import numpy as np
import pytest

import instance_reference as IR
import vote_split_cases as C
import vote_split_reference as VR


def one_pixel(h, w, y, x, dy, dx, label=1):
    labels = np.zeros((1, h, w), np.uint8)
    field = np.zeros((1, h, w, 2), np.float32)
    labels[0, y, x] = label
    field[0, y, x] = (dy, dx)
    return labels, field


def grid_of(cells, gh, gw):
    g = np.zeros((gh, gw), np.int32)
    for (cy, cx), v in cells.items():
        g[cy, cx] = v
    return g


# 8 x 12 at cell 4: a 2 x 3 grid; the pixel (5, 6) lies in cell (1, 1)
@pytest.mark.parametrize("d,cells", [
    ((1.0, 0.0), {(1, 1): 1}),                 # down: a = 5.5, then 9.5 >= 8
    ((-1.0, 0.0), {(1, 1): 1, (0, 1): 1}),     # up: 5.5, 1.5, then -2.5
    ((0.0, 2.0), {(1, 1): 1, (1, 2): 1}),      # right: 6.5, 10.5, then 14.5 >= 12
    ((0.0, -0.5), {(1, 1): 1, (1, 0): 1}),     # left: 6.5, 2.5, then -1.5
    ((-3.0, 3.0), {(1, 1): 1, (0, 2): 1}),     # |dy| == |dx|: y is the major axis, m = -1: (5.5, 6.5), (1.5, 10.5)
    ((3.0, 4.0), {(1, 1): 1}),                 # x major, m = 0.75: (6.5, 5.5), then the minor axis leaves: (10.5, 8.5)
], ids=["down", "up", "right", "left", "diagonal", "minor_leaves"])
def test_one_ray_per_edge(d, cells):
    labels, field = one_pixel(8, 12, 5, 6, *d)
    acc = VR.accumulate(labels, field, 0, 1, 4, 1)
    assert acc.shape == (1, 1, 2, 3) and np.array_equal(acc[0, 0], grid_of(cells, 2, 3))


def test_pixels_that_do_not_vote():
    labels = np.zeros((1, 8, 12), np.uint8)
    field = np.zeros((1, 8, 12, 2), np.float32)
    for y, x, l, d in ((2, 2, 1, (0, 0)), (2, 4, 1, (np.nan, 1)), (2, 6, 1, (1, np.inf)), (4, 4, 3, (1, 0)), (3, 2, 1, (1, 0)), (4, 3, 2, (1, 0))):
        labels[0, y, x], field[0, y, x] = l, d
    # a zero direction, a NaN, an infinity, a label above objects = 2, and two pixels the stride of 2 skips (row 3, column 3)
    assert VR.accumulate(labels, field, 0, 2, 4, 2).sum() == 0
    acc = VR.accumulate(labels, field, 0, 2, 4, 1)        # at stride 1 the last two vote: (3, 2) down -> (0,0), (1,0); (4, 3) of object 2 -> (1,0)
    want = np.zeros((1, 2, 2, 3), np.int32)
    want[0, 0, 0, 0] = want[0, 0, 1, 0] = want[0, 1, 1, 0] = 1
    assert np.array_equal(acc, want)


def test_a_grid_that_does_not_divide_the_image():
    labels, field = one_pixel(5, 7, 4, 6, -1.0, -1.0)      # cell 2 -> 3 x 4: (4.5, 6.5), (2.5, 4.5), (0.5, 2.5), then -1.5
    acc = VR.accumulate(labels, field, 0, 1, 2, 1)
    assert np.array_equal(acc[0, 0], grid_of({(2, 3): 1, (1, 2): 1, (0, 1): 1}, 3, 4))


def test_the_direction_is_read_at_dir_off_plus_two_kp_index():
    labels = np.zeros((1, 8, 12), np.uint8)
    field = np.zeros((1, 8, 12, 20), np.float32)
    labels[0, 5, 6] = 1
    field[0, 5, 6, 7:9] = (-1.0, 0.0)
    slots, inst, pk, acc, keys = VR.split_labels(labels, field, 1, 1, 1, kp_index=3, cell=4, vote_stride=1, min_votes=1, min_size=1, stages=True)
    assert np.array_equal(acc[0, 0], grid_of({(1, 1): 1, (0, 1): 1}, 2, 3))


GRID = {(0, 0): 9, (0, 1): 3, (3, 3): 9, (3, 4): 9, (1, 2): 2}     # 4 x 5


def test_peak_order_plateau_and_clipping():
    g = grid_of(GRID, 4, 5)
    inst, pk, cand = VR.peaks(g, cell=4, R=3, min_votes=3, rel_percent=25, nms_radius=1)
    # (0,0) and (3,3) have equal votes: the smaller cell index ranks first; (3,4) shares (3,3)'s window and has the larger index: a plateau gives one
    # candidate; (0,1) lies in (0,0)'s window; (1,2) is below min_votes
    assert inst.tolist() == [[0, 9, 0, 0], [0, 9, 3, 3], [0, 0, -1, -1]]
    assert np.count_nonzero(cand) == 2 and cand[0, 0] == (9 << 32) | 0xFFFFFFFF and cand[3, 3] == (9 << 32) | (0xFFFFFFFF - 18)
    # the corner: the window and the 3 x 3 centroid are clipped.  y = 12 / 12 * 2, x = (9 * 1 + 3 * 3) / 12 * 2; at (3,3): x = (9 * 7 + 9 * 9) / 18 * 2
    assert pk.tolist() == [[2.0, 3.0], [14.0, 16.0], [0.0, 0.0]] and pk.dtype == np.float32


def test_the_cut_and_more_candidates_than_ranks():
    g = grid_of({**GRID, (3, 3): 8, (3, 4): 0}, 4, 5)
    assert VR.peaks(g, 4, 3, 3, 100, 1)[0].tolist() == [[0, 9, 0, 0], [0, 0, -1, -1], [0, 0, -1, -1]]     # 800 < 900
    assert VR.peaks(g, 4, 3, 3, 88, 1)[0].tolist() == [[0, 9, 0, 0], [0, 8, 3, 3], [0, 0, -1, -1]]        # 800 >= 792
    assert VR.peaks(g, 4, 1, 3, 0, 1)[0].tolist() == [[0, 9, 0, 0]]                                       # two candidates, R = 1
    assert VR.peaks(np.zeros((4, 5), np.int32), 4, 2, 1, 0, 4)[0].tolist() == [[0, 0, -1, -1]] * 2        # an empty grid


def test_the_centroid_is_rounded_once_from_fp64():
    g = grid_of({(1, 1): 3, (1, 2): 4, (2, 1): 0, (0, 0): 0}, 4, 5)
    inst, pk, _ = VR.peaks(g, 8, 1, 1, 0, 1)
    assert inst.tolist() == [[0, 4, 1, 2]]
    assert pk[0, 0] == np.float32(12.0) and pk[0, 1] == np.float32(np.float64(3 * 3 + 4 * 5) / np.float64(7) * 4.0)


def test_assignment_by_hand():
    ys, xs = np.array([10, 10, 10, 13]), np.array([18, 18, 12, 18])
    dy, dx = np.array([0, 0, 0, 0], np.float32), np.array([-1, 1, 0, 1], np.float32)
    left = VR.dist2(ys, xs, dy, dx, 10.5, 10.5)
    right = VR.dist2(ys, xs, dy, dx, 10.5, 30.5)
    # pointing at the peak: 0; pointing away: e2; no direction: e2; the line of sight passes 3 px from the right peak: 9
    assert left.tolist() == [0.0, 64.0, 4.0, 73.0] and right.tolist() == [144.0, 0.0, 324.0, 9.0] and left.dtype == np.float32


@pytest.mark.parametrize("name", sorted(C.SCENES))
@pytest.mark.parametrize("sigma", C.SIGMAS)
@pytest.mark.parametrize("stride", (1, 2))
def test_planted_scenes_on_the_reference(name, sigma, stride):
    """The number of non-empty slots is the number of planted discs, and at least 94 % of each disc's pixels carry one slot of their own.
    Measured with this reference (the smaller disc share per scene over both strides and both sigmas): touch2 98.2 %, touch3 95.9 %, two_obj
    97.8 %, single 100 %."""
    slots, inst, pk, acc, keys = C.reference(name, sigma, stride)
    items = C.SCENES[name][1]
    assert int((inst[..., 0] > 0).sum()) == len(items)
    got = C.shares(name, slots)
    print(name, sigma, stride, ["%d: %.4f" % s for s in got])
    assert len({s for s, _ in got}) == len(items) and all(s > 0 for s, _ in got)
    assert min(share for _, share in got) >= C.MIN_SHARE
    if name == "single":
        assert inst[0, 0, 0, 0] == 616 and int((slots == 1).sum()) == 616
    for i, (label, _, _, _) in enumerate(items):
        slot = got[i][0]
        assert (slot - 1) // C.R == label - 1                     # a slot of the disc's own object


def test_the_component_rule_cannot_separate_touching_discs():
    """The reason cp_vote_split_labels exists: cp_ccl_instance_labels' rule gives touching discs one slot.  touch2: one component of 768 pixels.
    touch3: the two upper discs are one component of 632; the third disc, 22.4 px from either, does not touch them (the planted coordinates
    leave a gap of 2.4 px), so the component rule finds 2 instances where 3 were planted."""
    s = C.scene("touch2", 0.0)
    slots, inst = IR.instance_labels(s.labels, s.objects, C.R, 50)
    assert inst[0, 0, :, 0].tolist() == [768, 0, 0, 0] and set(np.unique(slots)) == {0, 1}
    s = C.scene("touch3", 0.0)
    slots, inst = IR.instance_labels(s.labels, s.objects, C.R, 50)
    assert inst[0, 0, :, 0].tolist() == [632, 316, 0, 0]
    assert len(set(slots[0][s.owner == 0])) == 1 and set(slots[0][s.owner == 0]) == set(slots[0][s.owner == 1])
