"""tests/kpcov_reference.py on closed-form cases, and the conditions the GPU tests (tests/test_gpu_kpcov.py) need of their inputs, checked on the
reference alone.  No kernel runs here."""
import itertools

import numpy as np
import pytest

import kpcov_reference as KC
import ransac_reference as R

THRESH, MIN_NUM = 0.99, 5
SETTINGS = ((64, 1), (48, 2), (16, 3))   # (hyp, draw seed) of the GPU tests


def test_two_hypotheses_with_weights_one_and_three():
    hp = np.zeros((2, 9, 2), np.float32)
    hp[0, :, :], hp[1, :, :] = (1.0, 2.0), (5.0, -2.0)
    counts = np.tile(np.array([[1], [3]]), (1, 9))
    mean = np.tile(np.array([4.0, -1.0]), (9, 1))       # the weighted mean: (1 + 15) / 4, (2 - 6) / 4
    cov, wsum = KC.covariance(hp, counts, mean)
    # differences (-3, 3) with weight 1 and (1, -1) with weight 3: sxx = (9 + 3) / 4 = 3, sxy = (-9 - 3) / 4 = -3, syy = 3
    assert (wsum == 4).all() and np.array_equal(cov, np.tile([3.0, -3.0, 3.0], (9, 1)))
    cov0, _ = KC.covariance(hp, counts, np.zeros((9, 2)))   # about the origin: the raw second moments
    assert np.array_equal(cov0, np.tile([(1 + 75) / 4, (2 - 30) / 4, (4 + 12) / 4], (9, 1)))


def test_a_permutation_of_the_hypotheses_changes_nothing_beyond_rounding():
    rng = np.random.default_rng(0)
    hp = rng.uniform(-50, 150, (40, 9, 2)).astype(np.float32)
    counts = rng.integers(0, 500, (40, 9))
    mean = rng.uniform(0, 100, (9, 2))
    cov, wsum = KC.covariance(hp, counts, mean)
    perm = rng.permutation(40)
    cov2, wsum2 = KC.covariance(hp[perm], counts[perm], mean)
    assert np.array_equal(wsum, wsum2) and np.abs(cov - cov2).max() <= 64 * np.spacing(np.abs(cov).max())


def test_a_nan_hypothesis_without_inliers_is_skipped():
    hp = np.zeros((3, 9, 2), np.float32)
    hp[0], hp[1], hp[2] = (1.0, 2.0), np.nan, (5.0, -2.0)
    counts = np.tile(np.array([[1], [0], [3]]), (1, 9))
    mean = np.tile(np.array([4.0, -1.0]), (9, 1))
    cov, wsum = KC.covariance(hp, counts, mean)
    assert (wsum == 4).all() and np.array_equal(cov, np.tile([3.0, -3.0, 3.0], (9, 1)))
    mean[4, 1] = np.inf                                       # a non-finite mean: zeros for that keypoint alone
    cov, wsum = KC.covariance(hp, counts, mean)
    assert wsum[4] == 0 and not cov[4].any() and (np.delete(wsum, 4) == 4).all()
    cov, wsum = KC.covariance(hp, np.zeros((3, 9), int), mean)
    assert not cov.any() and not wsum.any()


@pytest.mark.parametrize("hyp,seed", SETTINGS)
def test_the_gpu_inputs_are_usable(hyp, seed):
    """common_input(0) with common_draws(seed, 1, hyp)[0]: hypotheses_f32 does not refuse, and every voted keypoint has definite inliers."""
    labels, field, kps = R.common_input(0)
    draws = R.common_draws(seed, 1, hyp)[0]
    smallest = None
    for bi, o in itertools.product(range(R.B), range(R.OBJECTS)):
        pix = R.pixel_list(labels[bi], o)
        if pix.size < MIN_NUM:
            continue
        direct, coords = R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
        cov, wlo, whi, _ = KC.reference_object(direct, coords, draws[bi, o].astype(np.int64) % pix.size, THRESH, kps[bi, o])
        assert (wlo > 0).all() and (whi >= wlo).all() and np.isfinite(cov).all(), (bi, o, wlo)
        smallest = int(wlo.min()) if smallest is None else min(smallest, int(wlo.min()))
    print("hyp %d seed %d: the smallest definite-inlier sum is %d" % (hyp, seed, smallest))
