"""tests/verify_reference.py -- the NumPy restatement of the pose verification's rule -- against counts worked out by hand on planes written by
hand (tests/verify_cases.py states the 5 x 7 case and its derivation).  No GPU and no library are needed."""
import numpy as np

import verify_cases as VC
import verify_reference as VR


def reference(case, **change):
    c = dict(case, **change)
    return VR.counts(c["planes"], c["records"], c["inst_counts"], c["imax"], c["labels"], c["field"], c["dir_off"], c["kp"], c["kp2d"], c["jobs"],
                     c["sample_offset"], c["cos_min"])


def test_hand_case_by_hand():
    got = reference(VC.hand())
    assert got.dtype == np.int32 and got.tolist() == [list(VC.HAND_A), list(VC.HAND_B)]


def test_threshold_edges():
    """cos_min 0 takes every pair that does not point away, cos_min 1 only the direction exactly on the ray; the two directions a hair to either
    side of cos = 3 / 5 part at cos_min 0.6 and nowhere else nearby"""
    case = VC.hand()
    assert reference(case, cos_min=0.0)[0].tolist() == [12, 2, 8, 1, 1, 10, 4, 3]
    assert reference(case, cos_min=1.0)[0].tolist() == [12, 2, 8, 1, 1, 10, 4, 1]
    assert reference(case, cos_min=0.59)[0, VR.INLIERS] == 3 and reference(case, cos_min=0.61)[0, VR.INLIERS] == 1


def test_equal_words_go_to_the_lower_plane():
    case = VC.hand()
    planes = case["planes"].copy()
    planes[1, 2, 3] = VC.bits(1.5)                   # no longer equal: plane 1 is nearer at (2, 3) as well
    got = reference(case, planes=planes)
    assert got[0].tolist() == [12, 3, 7, 1, 1, 10, 4, 2] and got[1, VR.HIDDEN] == 1 and got[1, VR.ON_OTHER] == 1     # (2, 3) carries label 1


def test_refusals_instance_counts_and_boxes():
    case = VC.hand()
    jobs = [(1, 0, 1, 0), (-1, 0, 1, 0), (0, 2, 1, 0), (0, -1, 1, 0), (0, 0, 0, 0), (0, 0, 256, 0), (0, 0, 9, 0)]
    got = reference(case, jobs=np.array(jobs, np.int32), kp2d=np.tile(case["kp2d"][:1], (len(jobs), 1, 1)))
    assert not got[:6].any() and got[6].tolist() == [12, 2, 0, 1, 9, 0, 0, 0]
    assert reference(case, inst_counts=np.array([1], np.int32))[0].tolist() == [12, 0, 8, 1, 3, 10, 4, 2]
    assert not reference(case, inst_counts=np.zeros(0, np.int32)).any()           # the frame lies beyond inst_counts
    records = case["records"].copy()
    records[0, 2:6] = -1
    assert reference(case, records=records)[0].tolist() == [0, 0, 0, 0, 0, 10, 0, 0]
    records[0, 2:6] = (-2, -3, 5, 5)
    assert reference(case, records=records)[0].tolist() == [6, 0, 5, 1, 0, 10, 4, 2]
    records = case["records"].copy()
    records[1, 2:6] = (4, 2, 0, 2)                   # plane 1 is read in column 4 only
    assert reference(case, records=records)[0].tolist() == [12, 1, 8, 1, 2, 10, 4, 2]


def test_score_from_counts():
    iou, agreement, visible, score = VR.score_from_counts(np.array([VC.HAND_A, VC.HAND_B, (0,) * 8]))
    assert iou.tolist() == [8 / 11, 10 / 11, 0.0] and agreement.tolist() == [0.5, 1.0, 0.0] and visible.tolist() == [10 / 12, 10 / 12, 0.0]
    assert score.tolist() == [8 / 11 * 0.5, 10 / 11, 0.0]
