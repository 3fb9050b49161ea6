"""The keypoint covariance op (cp_kp_cov_f32 / cp_kp_cov_seeded_f32, csrc/ransac_vote.hip) checked stage by stage on the stage tests' own input
(tests/ransac_reference.py: B = 2, 72 x 100, 4 objects, ragged ballot tails, an interrupted block, a 64-pixel object, an absent object and a
4-pixel object).  Stage A reads the op's pixel list, hypotheses and counts out of the workspace (cp_kp_cov_workspace_layout) and compares them
with the fp64 restatement, as tests/test_gpu_ransac_stages.py does for the voter; stage B compares cov and wsum with
kpcov_reference.covariance of the kernel's OWN stage-A products: wsum exactly, every covariance entry within 8 fp32 ulps of the keypoint's
trace -- one rounding to fp32 of an fp64 sum of at most 64 terms per lane and a 6-level tree, with the project's usual margin (derived, not
measured).  Every condition a check needs of its input is asserted on the reference first (tests/test_kpcov_reference.py)."""
import ctypes as C
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kpcov_reference as KC
import ransac_reference as R

pytestmark = pytest.mark.gpu

THRESH, MIN_NUM = 0.99, 5
SETTINGS = {64: 1, 48: 2, 16: 3}   # hyp -> draw seed (64: vote_kernel<64>; 48 and 16: vote_kernel<16>)
STATE = np.dtype([("tn", "<i4"), ("done", "<i4"), ("rounds", "<i4"), ("hyp_num", "<f4"), ("win_ratio", "<f4", (9,)), ("win_pts", "<f4", (9, 2))])


def kp_cov(lib, device, labels, field, dir_off, objects, hyp, mean, thresh=THRESH, min_num=MIN_NUM, max_num=30000, draws=None, seed=None):
    """One call of cp_kp_cov_f32 (draws given) or cp_kp_cov_seeded_f32 (seed given); everything it left behind, as NumPy arrays."""
    from casapose_amd import _lib

    b, h, w = labels.shape
    offs, state_bytes = (C.c_size_t * 4)(), C.c_size_t()
    _lib.check(lib.cp_kp_cov_workspace_layout(b, h, w, objects, 9, hyp, offs, C.byref(state_bytes)), "cp_kp_cov_workspace_layout")
    assert state_bytes.value == STATE.itemsize
    nbytes = lib.cp_kp_cov_workspace_bytes(b, h, w, objects, 9, hyp)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    assert ws.data_ptr() % 256 == 0
    lab_d, fld_d = torch.from_numpy(labels).to(device), torch.from_numpy(field).to(device)
    mean_d = torch.from_numpy(np.ascontiguousarray(mean, np.float32)).to(device)
    cov = torch.full((b, objects, 9, 3), 7.0, dtype=torch.float32, device=device)
    wsum = torch.full((b, objects, 9), -1, dtype=torch.int32, device=device)
    head = (lab_d.data_ptr(), fld_d.data_ptr(), field.shape[-1], dir_off, b, h, w, objects, 9, mean_d.data_ptr())
    tail = (hyp, float(thresh), int(min_num), int(max_num), ws.data_ptr(), cov.data_ptr(), wsum.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    if draws is not None:
        assert draws.dtype == np.int32 and draws.shape == (b, objects, hyp, 9, 2)
        dr_d = torch.from_numpy(np.ascontiguousarray(draws)).to(device)
        _lib.check(lib.cp_kp_cov_f32(*head, dr_d.data_ptr(), *tail), "cp_kp_cov_f32")
    else:
        _lib.check(lib.cp_kp_cov_seeded_f32(*head, int(seed), *tail), "cp_kp_cov_seeded_f32")
    torch.cuda.synchronize(device)
    raw = ws.cpu().numpy()

    def part(i, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert offs[i] % 256 == 0 and offs[i] + n <= nbytes and all(offs[i] + n <= offs[j] for j in range(4) if offs[j] > offs[i])
        return raw[offs[i]:offs[i] + n].view(dtype).reshape(shape).copy()

    return SimpleNamespace(cov=cov.cpu().numpy(), wsum=wsum.cpu().numpy(), pixlist=part(0, "<i4", (b, objects, h * w)), st=part(1, STATE, (b, objects)),
                           hyp_pts=part(2, "<f4", (b, objects, hyp, 9, 2)), counts=part(3, "<i4", (b, objects, hyp, 9)))


@functools.lru_cache(maxsize=None)
def common():
    labels, field, kps = R.common_input(0)
    objs = {}
    for bi, o in itertools.product(range(R.B), range(R.OBJECTS)):
        pix = R.pixel_list(labels[bi], o)
        if pix.size >= MIN_NUM:
            objs[bi, o] = (pix,) + R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
    assert sorted(objs) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    return labels, field, objs, kps.astype(np.float32)       # the means: the true keypoints, as fp32 values


@functools.lru_cache(maxsize=None)
def draws_of(hyp):
    return R.common_draws(SETTINGS[hyp], 1, hyp)[0]


@functools.lru_cache(maxsize=None)
def reference(hyp):
    """(bi, o) -> (cov [9,3] from the definite inliers, wsum_lo, wsum_hi, hyp_pts fp32, pos_tol) by the reference alone"""
    _, _, objs, mean = common()
    ref = {}
    for (bi, o), (pix, direct, coords) in objs.items():
        idx = draws_of(hyp)[bi, o].astype(np.int64) % pix.size
        ref[bi, o] = KC.reference_object(direct, coords, idx, THRESH, mean[bi, o]) + (R.hypotheses_f32(direct, coords, idx)[1],)
    return ref


@pytest.fixture(scope="module")
def runs(hip_lib, device):
    labels, field, _, mean = common()
    return {hyp: kp_cov(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, hyp, mean, draws=draws_of(hyp)) for hyp in SETTINGS}


# ---- stage A: the op's own compaction, hypotheses and counts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyp", list(SETTINGS))
def test_stage_a_pixels_hypotheses_and_counts(runs, hyp):
    labels, _, objs, _ = common()
    r, ref = runs[hyp], reference(hyp)
    for bi, o in itertools.product(range(R.B), range(R.OBJECTS)):
        st = r.st[bi, o]
        if (bi, o) not in objs:
            assert int((labels[bi] == o + 1).sum()) in (0, 4) and st["tn"] == 0 and st["done"] == 1, (bi, o)
            continue
        pix, direct, coords = objs[bi, o]
        assert st["tn"] == pix.size and st["done"] == 0 and np.array_equal(r.pixlist[bi, o, :pix.size], pix), (bi, o)
        _, _, _, hp, tol = ref[bi, o]
        pts, det = R.hypotheses(direct, coords, draws_of(hyp)[bi, o].astype(np.int64) % pix.size)
        valid = det > 1e-6
        assert not r.hyp_pts[bi, o][~valid].any() and not hp[~valid].any(), (bi, o)      # exactly (0, 0)
        err = np.abs(r.hyp_pts[bi, o].astype(np.float64) - pts).max(-1)
        assert (err[valid] <= tol[valid]).all(), (bi, o, float((err[valid] / tol[valid]).max()))
        lo, hi, _ = R.count_bounds(direct, coords, r.hyp_pts[bi, o], THRESH)       # the kernel's own hypotheses
        got = r.counts[bi, o]
        bad = (got < lo) | (got > hi)
        assert not bad.any(), (bi, o, np.argwhere(bad)[:5], got[bad][:5], lo[bad][:5], hi[bad][:5])


# ---- stage B: the moments of the kernel's own points and counts --------------------------------------------------------------------------------------
def assert_stage_b(r, bi, o, mean, what=""):
    want, wsum = KC.covariance(r.hyp_pts[bi, o], r.counts[bi, o], mean)
    assert np.array_equal(r.wsum[bi, o], wsum), (what, bi, o, r.wsum[bi, o], wsum)
    tol = 8.0 * np.spacing(np.float32(want[:, 0] + want[:, 2])).astype(np.float64)
    err = np.abs(r.cov[bi, o].astype(np.float64) - want)
    assert (err <= tol[:, None]).all(), (what, bi, o, float((err / tol[:, None]).max()))
    return want


@pytest.mark.parametrize("hyp", list(SETTINGS))
def test_stage_b_covariance_of_the_kernels_own_hypotheses(runs, hyp):
    _, _, objs, mean = common()
    for bi, o in objs:
        want = assert_stage_b(runs[hyp], bi, o, mean[bi, o])
        assert (runs[hyp].wsum[bi, o] > 0).all() and (want[:, 0] > 0).all() and (want[:, 2] > 0).all()
        assert (want[:, 1] ** 2 <= want[:, 0] * want[:, 2]).all()


@pytest.mark.parametrize("hyp", list(SETTINGS))
def test_absent_and_small_objects_give_zeros(runs, hyp):
    r = runs[hyp]
    for bi, o in ((0, 3), (1, 3)):       # absent; 4 pixels < min_num
        assert not r.cov[bi, o].any() and not r.wsum[bi, o].any()
    assert np.isfinite(r.cov).all()       # no NaN of the background or of the other channels reached a sum


def test_non_finite_directions_are_skipped_not_multiplied(hip_lib, device):
    """Object 1 of image 0 (64 px): pixel 5 of its list has NaN directions and pixel 9 infinite ones; hypothesis 0 draws pixel 5 and hypothesis 1
    pixel 9 first, for every keypoint.  Whatever those hypotheses are stored as, they have no inliers and the covariance is finite and equals
    the reference without them."""
    labels, field, objs, mean = common()
    hyp, (bi, o) = 16, (0, 1)
    pix = objs[bi, o][0]
    field, draws = field.copy(), draws_of(hyp).copy()
    for t, bad in ((5, np.nan), (9, np.inf)):
        y, x = divmod(int(pix[t]), R.W)
        field[bi, y, x, R.DIR_OFF:R.DIR_OFF + 18:2] = bad
    draws[bi, o, 0, :, 0] = 5 + 3 * pix.size
    draws[bi, o, 1, :, 0] = 9 + 7 * pix.size
    r = kp_cov(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, hyp, mean, draws=draws)
    assert not r.counts[bi, o, :2].any() and (r.counts[bi, o, 2:].sum(0) > 0).all()
    assert np.isfinite(r.cov).all()
    want = assert_stage_b(r, bi, o, mean[bi, o], "non-finite directions")
    without, wsum = KC.covariance(r.hyp_pts[bi, o, 2:], r.counts[bi, o, 2:], mean[bi, o])
    assert np.array_equal(want, without) and np.array_equal(r.wsum[bi, o], wsum)
    direct, coords = R.pixel_records(field[bi], pix, R.W, R.DIR_OFF)
    with np.errstate(invalid="ignore"):
        lo, hi, _ = R.count_bounds(direct, coords, r.hyp_pts[bi, o, 2:], THRESH)
    assert ((lo <= r.counts[bi, o, 2:]) & (r.counts[bi, o, 2:] <= hi)).all()
    for other in objs:
        if other != (bi, o):
            assert_stage_b(r, *other, mean[other], "neighbour of the non-finite object")


def test_a_non_finite_mean_gives_zeros_for_that_keypoint(hip_lib, device, runs):
    labels, field, objs, mean = common()
    mean = mean.copy()
    mean[0, 0, 3, 1], mean[1, 2, 8, 0], mean[1, 1, 0, 0] = np.nan, np.inf, -np.inf
    r = kp_cov(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, 16, mean, draws=draws_of(16))
    for bi, o, v in ((0, 0, 3), (1, 2, 8), (1, 1, 0)):
        assert not r.cov[bi, o, v].any() and r.wsum[bi, o, v] == 0
    keep = np.isfinite(mean).all(-1)
    assert np.array_equal(r.cov[keep], runs[16].cov[keep]) and np.array_equal(r.wsum[keep], runs[16].wsum[keep])


def test_seeded_calls_repeat_bit_for_bit_and_seeds_differ(hip_lib, device):
    labels, field, objs, mean = common()
    run = lambda seed, **kw: kp_cov(hip_lib, device, labels, field, R.DIR_OFF, R.OBJECTS, 64, mean, seed=seed, **kw)   # noqa: E731
    a, a2, c = run(11), run(11), run(12)
    assert np.array_equal(a.cov, a2.cov) and np.array_equal(a.wsum, a2.wsum) and np.array_equal(a.hyp_pts, a2.hyp_pts)
    for bi, o in objs:
        assert not np.array_equal(a.cov[bi, o], c.cov[bi, o]), (bi, o)
        assert_stage_b(a, bi, o, mean[bi, o], "seeded")
        assert a.st[bi, o]["tn"] == objs[bi, o][0].size
    for bi, o in ((0, 3), (1, 3)):
        assert not a.cov[bi, o].any() and not a.wsum[bi, o].any()
    # above max_num the pixels are thinned inside the compaction: fewer pixels vote, the moments are those of the op's own products
    t = run(11, max_num=400)
    for bi, o in ((0, 0), (1, 0)):
        tn = int(t.st[bi, o]["tn"])
        assert abs(tn - 400) <= 5 * np.sqrt(400) and np.isin(t.pixlist[bi, o, :tn], objs[bi, o][0]).all()
        assert_stage_b(t, bi, o, mean[bi, o], "thinned")
    # the min_num gate belongs to the un-thinned count
    g = run(11, min_num=65)
    assert not g.cov[0, 1].any() and not g.wsum[0, 1].any() and g.wsum[0, 0].all()


@pytest.mark.parametrize("hyp", list(SETTINGS))
def test_a_clean_object_has_a_tenth_of_a_noisy_objects_spread(runs, hyp):
    """The feature's point: object 1 (angular noise 0.05, no outliers) against object 2 (noise 0.2, half outliers)."""
    ref = reference(hyp)
    for bi in range(R.B):
        trace = lambda c: np.median(c[:, 0] + c[:, 2])   # noqa: E731
        clean, noisy = trace(ref[bi, 1][0]), trace(ref[bi, 2][0])
        print("hyp %d image %d: reference median trace %.4g against %.4g (ratio 1/%.0f)" % (hyp, bi, clean, noisy, noisy / clean))
        assert clean < noisy / 10.0                      # on the reference first
        got_clean, got_noisy = trace(runs[hyp].cov[bi, 1].astype(np.float64)), trace(runs[hyp].cov[bi, 2].astype(np.float64))
        print("hyp %d image %d: device median trace %.4g against %.4g" % (hyp, bi, got_clean, got_noisy))
        assert got_clean < got_noisy / 10.0


# ---- the Python wrapper --------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_label_and_one_hot_paths_agree(device, runs):
    from casapose_amd.pose_estimation.keypoint_covariance import keypoint_covariance

    labels, field, _, mean = common()
    lab = torch.from_numpy(labels).to(device)
    vert = torch.from_numpy(np.ascontiguousarray(field[..., R.DIR_OFF:R.DIR_OFF + 18])).to(device)
    pts, dr = torch.from_numpy(mean).to(device), torch.from_numpy(draws_of(16)).to(device)
    cov, wsum = keypoint_covariance(lab, vert, pts, hyp=16, draws=dr, return_weight_sum=True)
    assert cov.is_cuda and cov.dtype == torch.float32 and tuple(cov.shape) == (R.B, R.OBJECTS, 9, 3) and wsum.dtype == torch.int32
    assert np.array_equal(cov.cpu().numpy(), runs[16].cov) and np.array_equal(wsum.cpu().numpy(), runs[16].wsum)
    onehot = torch.nn.functional.one_hot(lab.long(), R.OBJECTS + 1)[..., 1:].to(torch.float32)
    cov2 = keypoint_covariance(onehot, vert.reshape(R.B, R.H, R.W, 9, 2), pts, hyp=16, draws=dr)
    assert torch.equal(cov, cov2)
    g = lambda: torch.Generator().manual_seed(5)   # noqa: E731
    assert torch.equal(keypoint_covariance(lab, vert, pts, hyp=16, generator=g()), keypoint_covariance(lab, vert, pts, hyp=16, generator=g()))


def test_return_covariance_is_the_separate_call_on_the_returned_points(device):
    from casapose_amd.pose_estimation.keypoint_covariance import keypoint_covariance
    from casapose_amd.pose_estimation.ransac_voting import ransac_voting_layer_all_masks

    labels, field, objs, _ = common()
    lab = torch.from_numpy(labels).to(device)
    vert = torch.from_numpy(np.nan_to_num(field[..., R.DIR_OFF:R.DIR_OFF + 18])).to(device)
    onehot = torch.nn.functional.one_hot(lab.long(), R.OBJECTS + 1)[..., 1:].to(torch.float32)
    plain = ransac_voting_layer_all_masks(onehot, vert, 64, generator=torch.Generator().manual_seed(3))
    pts, cov = ransac_voting_layer_all_masks(onehot, vert, 64, generator=torch.Generator().manual_seed(3), return_covariance=True)
    assert torch.equal(plain, pts) and tuple(cov.shape) == (R.B, R.OBJECTS, 9, 3)
    g = torch.Generator().manual_seed(3)
    torch.randint(0, 2**62, (1,), dtype=torch.int64, generator=g)        # the voter's own seed
    want = keypoint_covariance(lab, vert, pts, hyp=64, generator=g)
    assert torch.equal(cov, want)
    c = cov.cpu().numpy()
    for bi, o in objs:
        assert (c[bi, o, :, 0] > 0).all() and (c[bi, o, :, 2] > 0).all(), (bi, o)
    assert not c[0, 3].any() and not c[1, 3].any()
    pts2, rounds, cov2 = ransac_voting_layer_all_masks(onehot, vert, 64, generator=torch.Generator().manual_seed(3), return_rounds=True, return_covariance=True)
    assert torch.equal(cov2, cov) and rounds.dtype == torch.int32


def test_host_tensors_and_bad_arguments_are_refused_by_name(hip_lib, device):
    from casapose_amd import _lib
    from casapose_amd.pose_estimation.keypoint_covariance import keypoint_covariance

    labels, field, _, mean = common()
    lab, vert, pts = torch.from_numpy(labels), torch.from_numpy(np.ascontiguousarray(field[..., R.DIR_OFF:R.DIR_OFF + 18])), torch.from_numpy(mean)
    with pytest.raises(_lib.CasaposeHipError, match="keypoint_covariance"):
        keypoint_covariance(lab, vert, pts)
    with pytest.raises(_lib.CasaposeHipError, match="cp_kp_cov_seeded_f32.*multiple of 16"):
        keypoint_covariance(lab.to(device), vert.to(device), pts.to(device), hyp=24)
    # hyp * min(max_num, h*w) >= 2^31 is refused before anything is launched or the workspace is touched: small tensors stand in
    d = [t.to(device) for t in (lab, vert, pts)]
    out = torch.zeros(R.B * R.OBJECTS * 9 * 3, dtype=torch.float32, device=device)
    rc = hip_lib.cp_kp_cov_seeded_f32(d[0].data_ptr(), d[1].data_ptr(), 18, 0, R.B, R.H, R.W, R.OBJECTS, 9, d[2].data_ptr(), 1, 298272, 0.99, 5, 30000,
                                      out.data_ptr(), out.data_ptr(), out.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    assert 298272 % 16 == 0 and 298272 * R.H * R.W >= 2 ** 31 and rc != 0 and b"cp_kp_cov_seeded_f32" in hip_lib.cp_last_error() and b"2^31" in hip_lib.cp_last_error()
    with pytest.raises(ValueError, match="merged field"):
        keypoint_covariance(lab.to(device), vert.to(device)[..., :16], pts.to(device))
    assert hip_lib.cp_kp_cov_workspace_layout(2, 8, 8, 1, 9, 16, None, None) == -1
    assert hip_lib.cp_kp_cov_workspace_layout(2, 8, 8, 1, 8, 16, (C.c_size_t * 4)(), None) == -1 and b"keypoints" in hip_lib.cp_last_error()
