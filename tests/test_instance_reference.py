"""CPU: the restatement of cp_ccl_instance_labels' rule (tests/instance_reference.py) against maps whose results are written out by hand -- a tie
in size resolved by the root, more eligible components than R, a component of min_size - 1 beside one of min_size, an object that covers more
than half of the image, a label above `objects`, and objects * R = 254 -- and against the one-instance filter's restatement where the two rules
agree."""
import numpy as np
import pytest

import ccl_cases as CC
import ccl_reference as R
import instance_reference as IR


@pytest.mark.parametrize("name", sorted(IR.HAND))
def test_hand_written_maps(name):
    c = IR.HAND[name]()
    slots, inst = IR.instance_labels(c.labels, c.objects, c.max_instances, c.min_size)
    assert slots.dtype == np.uint8 and inst.dtype == np.int32 and inst.shape == (c.labels.shape[0], c.objects, c.max_instances, 2)
    assert np.array_equal(slots, c.slots) and np.array_equal(inst, c.inst)


def test_hand_maps_hold_the_cases_they_are_made_for():
    e = IR.hand_edges()
    assert e.inst[0, 0, 1, 0] == 12 and int((e.labels[0] == 1).sum()) == 44 and not e.slots[0, 20:24, 60:63].any()      # tie, and a third eligible one
    assert int((e.labels[0, 10] == 2).sum()) == e.min_size - 1 and e.inst[0, 1, 0, 0] == e.min_size
    assert int((e.labels[1] == 3).sum()) * 2 > IR.HW and e.slots[1].max() == 5                                        # larger than the rest: kept
    assert e.labels.max() == 7 > e.objects and not e.slots[e.labels == 7].any()
    z = IR.hand_254()
    assert z.objects * z.max_instances == 254 == z.slots.max() and z.inst[1, 63, 0, 1] < z.inst[1, 63, 1, 1]
    b = IR.hand_blocks()
    assert (b.inst[0, 0, :, 0] == (25, 16, 9, 4)).all() and int((b.labels[0] == 1).sum()) == 25 + 16 + 9 + 4 + 4 + 1


def test_fewer_instances_keep_a_prefix():
    """R = 1 keeps instance 0 of R = 2, under the slot ids of R = 1"""
    c = IR.hand_edges()
    one, inst1 = IR.instance_labels(c.labels, c.objects, 1, c.min_size)
    assert np.array_equal(inst1[:, :, 0], c.inst[:, :, 0])
    for o in range(1, c.objects + 1):
        assert np.array_equal(one == o, c.slots == (o - 1) * 2 + 1)


@pytest.mark.parametrize("name", ["selection_edges", "three_labels", "labels_out_of_range", "checkerboard"])
def test_one_instance_equals_the_filter_where_the_rules_agree(name):
    """With R = 1 the slot of object o is o.  Where the largest component has at least min_size pixels and is no larger than the rest of the
    image (bin 0 wins that tie), the reference's histogram rule keeps that very component."""
    ref = CC.reference(name)
    case = ref.case
    b, h, w = case.labels.shape
    slots, inst = IR.instance_labels(case.labels, case.objects, 1, 50, components=(ref.root, ref.sizes))
    kept = R.filter(case.labels, case.objects, 50, 1)
    agree = 0
    for n in range(b):
        for o in range(1, case.objects + 1):
            fg = int((case.labels[n] == o).sum())
            comps = IR.ranked(ref.root[n], ref.sizes, case.labels[n], case.objects)[o]
            if comps and comps[0][1] >= 50 and comps[0][1] <= h * w - fg:
                agree += 1
                assert np.array_equal(slots[n] == o, kept[n] == o), (n, o)
    assert agree > 0 or name == "checkerboard"
