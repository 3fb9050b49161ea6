"""What tests/contour_cases.py says about the NumPy restatement (tests/contour_reference.py) alone, before any twin or kernel is held against
it: the conditions on the cases, the measured convergence the thresholds come from, and what the seed rule is for.  No GPU is needed."""
import numpy as np
import pytest

import contour_cases as CC
import contour_reference as CR


def test_defaults_are_the_refiners():
    from casapose_amd.pose_estimation import mask_refine

    assert (CR.GATE, CR.MIN_PIXELS) == (mask_refine.DEFAULT_GATE, mask_refine.DEFAULT_MIN_PIXELS) and CR.ITERATIONS == 8


@pytest.mark.parametrize("size", [(48, 64), (37, 50)])
def test_reference_keeps_the_starts_and_ends_where_it_was_measured(size):
    case = CC.block(*size)
    _, status, stats, last = CC.reference_loop(case)
    small = case["small"]
    assert small == 12 and len(status) == 18
    assert (status[:small] == CR.OK).all() and (status[small:] == CR.OK).sum() >= 5, status
    rot, xy, z = CC.errors(case, last)
    kept = status == CR.OK
    print("%d x %d: worst %.4f degrees, %.4f mm in the image plane, %.4f mm along the axis" % (size + (rot[kept].max(), xy[kept].max(), z[kept].max())))
    assert rot[kept].max() <= CC.MEASURED_DEG and xy[kept].max() <= CC.MEASURED_XY_MM and z[kept].max() <= CC.MEASURED_Z_MM
    start_rot, start_xy, _ = CC.errors(case, case["poses"])
    assert xy.mean() < 0.5 * start_xy.mean() and rot.mean() < start_rot.mean()           # it refines: the image-plane error more than halves


def test_thresholds_are_twice_the_measured_worst_case():
    """the record in tests/contour_cases.py is what the reference does on the two sizes, not a bound chosen beside it"""
    worst = np.zeros(3)
    for size in ((48, 64), (37, 50)):
        case = CC.block(*size)
        _, status, _, last = CC.reference_loop(case)
        worst = np.maximum(worst, [e[status == CR.OK].max() for e in CC.errors(case, last)])
    measured = np.array([CC.MEASURED_DEG, CC.MEASURED_XY_MM, CC.MEASURED_Z_MM])
    assert (worst <= measured).all() and (worst > measured - 1e-3).all(), (worst, measured)
    assert (CC.CONVERGED_DEG, CC.CONVERGED_XY_MM, CC.CONVERGED_Z_MM) == (2 * CC.MEASURED_DEG, 2 * CC.MEASURED_XY_MM, 2 * CC.MEASURED_Z_MM)


@pytest.mark.parametrize("size", [(48, 64), (37, 50)])
def test_occluder_boundary_must_not_be_seeded(size):
    """the block's label map has an occlusion edge: with the occluder relabelled to background that edge is seeded, the rendered contour under
    the occluder is pulled onto it, and the reference ends measurably farther from the truth"""
    right, wrong = CC.block(*size), CC.block(*size, 0)
    assert (right["labels"] == CC.OCCLUDER).sum() > 40 and not (wrong["labels"] == CC.OCCLUDER).any()
    seeds_right, seeds_wrong = CR.seeds_of(right["labels"][0], CC.BLOCK), CR.seeds_of(wrong["labels"][0], CC.BLOCK)
    assert (seeds_wrong & ~seeds_right).sum() >= 8 and not (seeds_right & ~seeds_wrong).any()      # the occlusion edge, and nothing else
    _, status, _, last = CC.reference_loop(right)
    assert CC.inside(right, last)[status == CR.OK].all()
    _, _, _, last_wrong = CC.reference_loop(wrong)
    a, b = CC.mean_vertex_distance(right, last).mean(), CC.mean_vertex_distance(wrong, last_wrong).mean()
    print("%d x %d: mean vertex distance %.3f mm, wrongly seeded %.3f mm" % (size + (a, b)))
    np.testing.assert_allclose((a, b), CC.OCCLUDER_MVD_MM[size], atol=2e-3)
    assert b > CC.OCCLUDER_WORSE * a
