"""tests/ccl_reference.py (scipy) against the oracle's flood fill and filter (oracle/casapose_oracle.py, voting_layers_2d.py:43-79) on the small
maps of tests/ccl_cases.py, and the selection rule on hand-worked histograms.  No GPU."""
import numpy as np
import pytest

import casapose_oracle as O
import ccl_cases as Cs
import ccl_reference as R


@pytest.mark.parametrize("name", Cs.SMALL)
def test_components_and_filter_match_the_oracle(name):
    ref = Cs.reference(name)          # asserts the map's own properties
    case = ref.case
    b, h, w = case.labels.shape
    assert h * w <= 70 * 200
    kept = {rank: R.filter(case.labels, case.objects, 50, rank) for rank in (1, 2)}
    for n in range(b):
        present = [int(o) for o in np.unique(case.labels[n]) if 0 < o <= case.objects]
        if case.objects > 8:
            present = present[:3] + present[-3:]       # the 254-object maps: both ends of the range
        absent = [o for o in range(1, case.objects + 1) if o not in present][:1]
        seen = np.zeros((h, w), bool)
        for o in present + absent:
            hot = (case.labels[n] == o).astype(np.float32)
            ids = O.label_components_4(hot > 0)
            on = ids > 0
            uniq, first = np.unique(ids.ravel(), return_index=True)
            assert np.array_equal(uniq[uniq > 0], np.arange(1, ids.max() + 1)) and (np.diff(first[uniq > 0]) > 0).all()   # ids in raster order
            lut = np.zeros(int(ids.max()) + 1, np.int64)
            lut[uniq] = first + n * h * w
            assert np.array_equal(ref.root[n][on], lut[ids[on]]) and (ref.root[n][on] >= 0).all(), (n, o)
            assert np.array_equal(ref.sizes[lut[1:]], np.bincount(ids.ravel())[1:]), (n, o)
            seen |= on
            for rank in (1, 2):
                assert np.array_equal(kept[rank][n] == o, O.largest_component_filter(hot, 50, rank) > 0), (n, o, rank)
        if len(present) == len([o for o in np.unique(case.labels[n]) if 0 < o <= case.objects]):
            assert (ref.root[n][~seen] == -1).all()     # background and labels above `objects`


def test_select_on_hand_worked_histograms():
    hw = 1000
    comps = [(10, 60), (200, 60), (500, 49), (700, 300)]                      # bin 0 = 531
    assert R.select(comps, hw, 50, 1) == (700, 300) and R.select(comps, hw, 50, 2) == (10, 60)
    assert R.select(comps, hw, 61, 2) == (10, 0)                               # zeroed bins keep their raster order
    assert R.select(comps, hw, 1, 2) == (10, 60) and R.select(comps[::-1], hw, 1, 2) == (10, 60)
    assert R.select([(5, 500)], hw, 50, 1) == (5, 500)                         # a tie with bin 0: bin 0 first
    assert R.select([(5, 501)], hw, 50, 1) == ("bin0", 499)
    assert R.select([(5, 1000)], hw, 50, 1) == ("bin0", 0) and R.select([(5, 1000)], hw, 50, 2) == (None, 0)
    assert R.select([], hw, 50, 1) == (None, 0) and R.select([], hw, 50, 2) == (None, 0)
    assert R.select([(3, 4), (9, 7)], hw, 50, 1) == (3, 0) and R.select([(3, 4), (9, 7)], hw, 50, 2) == (9, 0)
    assert R.select([(3, 50), (9, 49)], hw, 50, 1) == (3, 50) and R.select([(3, 49), (9, 50)], hw, 50, 1) == (9, 50)


def test_components_ignore_labels_above_objects():
    lab = np.array([[[1, 1, 3, 1], [0, 2, 3, 1], [2, 2, 255, 255]]], np.uint8)
    root, sizes = R.components(lab, 2)
    assert root.tolist() == [[[0, 0, -1, 3], [-1, 5, -1, 3], [5, 5, -1, -1]]]
    assert sizes.tolist() == [2, 0, 0, 2, 0, 3, 0, 0, 0, 0, 0, 0]
    assert R.filter(lab, 2, 1, 1).tolist() == [[[1, 1, 0, 0], [0, 2, 0, 0], [2, 2, 0, 0]]]
