"""The NumPy restatement of the depth refinement (tests/icp_reference.py) alone, on the rasteriser's planes: it converges on the block scene
inside thresholds set from its own measured worst case, the ellipsoids come closer from every start, and the keep / reject rule fires on each
of the cases that must come back unchanged.  No new entry point is called here."""
import numpy as np
import pytest

import icp_cases as IC
import icp_reference as IR


@pytest.mark.parametrize("size", [(48, 64), (37, 50)])
def test_block_converges_from_every_start(size):
    case = IC.block(*size)
    poses, status, stats = IC.reference_loop(case)
    rot, tr = IC.errors(case, poses)
    rot0, tr0 = IC.errors(case, case["poses"])
    print("%d x %d: worst %.4f deg %.4f mm (starts %.1f-%.1f deg, %.1f-%.1f mm)" % (size + (rot.max(), tr.max(), rot0.min(), rot0.max(), tr0.min(), tr0.max())))
    assert (status == IR.OK).all(), status
    # the starts are what the case says: 12 at 3-8 degrees, 6 at 10-15
    assert (rot0[:case["small"]] >= 3.0).all() and (rot0[:case["small"]] <= 8.0).all() and (rot0[case["small"]:] >= 10.0).all() and (rot0[case["small"]:] <= 15.0).all()
    # a wrong restatement must not be met by a wider threshold
    assert IC.MEASURED_DEG <= 0.5 and IC.MEASURED_MM <= 0.5 and IC.CONVERGED_DEG == 2.0 * IC.MEASURED_DEG and IC.CONVERGED_MM == 2.0 * IC.MEASURED_MM
    assert rot.max() < IC.CONVERGED_DEG and tr.max() < IC.CONVERGED_MM, (rot.max(), tr.max())
    assert (stats[:, -1, 1] < stats[:, 0, 1]).all() and (stats[:, -1, 1] < 0.5).all()      # the RMS residual ends at the sensor's rounding


def test_small_starts_are_there_within_four_iterations():
    case = IC.block()
    poses, status, _ = IC.reference_loop(case, iterations=4)
    rot, tr = IC.errors(case, poses)
    n = case["small"]
    assert (status[:n] == IR.OK).all() and rot[:n].max() < IC.CONVERGED_DEG and tr[:n].max() < IC.CONVERGED_MM, (rot[:n].max(), tr[:n].max())


def test_ellipsoids_come_closer_from_every_start():
    case = IC.ellipsoids()
    poses, status, _ = IC.reference_loop(case, min_pixels=IC.ELLIPSOID_MIN_PIXELS)
    assert (status == IR.OK).all(), status
    for i in range(len(poses)):
        verts = case["meshes"][int(case["obj"][i])][0]
        before, after = IR.mean_vertex_distance(verts, case["poses"][i], case["gt"][i]), IR.mean_vertex_distance(verts, poses[i], case["gt"][i])
        assert 4.0 < before < 20.0 and after < 0.25 * before, (i, before, after)


def test_the_default_damping_matters_on_the_ellipsoids():
    """The rotation of an ellipsoid is weakly constrained: over the nine starts eight iterations with damping 1e-3 leave 1.83 mm mean vertex
    distance on average, with 1e-6 0.49 mm.  This is a statement about the mean: one start of the mostly hidden second ellipsoid ends 0.08 mm
    closer with 1e-3 (0.906 against 0.984 mm)."""
    case = IC.ellipsoids()
    strong, _, _ = IC.reference_loop(case, min_pixels=IC.ELLIPSOID_MIN_PIXELS, damping=1e-3)
    weak, _, _ = IC.reference_loop(case, min_pixels=IC.ELLIPSOID_MIN_PIXELS)
    d = lambda poses: np.array([IR.mean_vertex_distance(case["meshes"][int(case["obj"][i])][0], poses[i], case["gt"][i]) for i in range(len(poses))])   # noqa: E731
    print("damping 1e-6:", np.round(d(weak), 3), "1e-3:", np.round(d(strong), 3))
    assert len(weak) == 9 and d(weak).mean() < 0.5 * d(strong).mean() and (d(weak) < d(strong)).sum() >= 8, (d(weak), d(strong))


def test_most_of_the_300_jobs_are_refined():
    """the 300-job case on the reference's loop before the twin and the device run it (3 iterations, as they do)"""
    case = IC.many_jobs()
    poses, status, stats = IC.reference_loop(case, iterations=3)
    assert len(status) == 300 and (status == IR.OK).sum() > 250, np.bincount(status)
    ok = status == IR.OK
    before = np.linalg.norm(case["poses"][:, :, 3] - case["gt"][:, :, 3], axis=1)
    after = np.linalg.norm(poses[:, :, 3] - case["gt"][:, :, 3], axis=1)
    assert np.median(after[ok]) < 0.25 * np.median(before[ok]) and np.array_equal(poses[~ok], case["poses"][~ok])


def test_keep_reject_rule_fires_on_each_unchanged_case():
    case = IC.unchanged()
    poses, status, stats = IC.reference_loop(case)
    assert np.array_equal(status, case["want"]) and len(IC.UNCHANGED) == (status != IR.OK).sum()
    for i in np.flatnonzero(status != IR.OK):
        assert np.array_equal(poses[i], case["poses"][i]), IC.UNCHANGED[i - 1]
        assert stats[i, 0, 0] < 32, IC.UNCHANGED[i - 1]
    assert not np.array_equal(poses[0], case["poses"][0])

