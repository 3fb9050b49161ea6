"""The device BPnP loss's arithmetic on the CPU: `cp_bpnp_loss_host_f64` (the host twin of `cp_bpnp_loss_f64`: the same csrc/bpnp_math.h, serially)
against the host path `training.bpnp_reprojection_loss_host`.  No kernel is launched here.

Gates come from the host path alone, never from the code under test.  RANSAC seeds do not move this loss (the tightening LM ends
in the same optimum), so the gate measures what does: the LM stopping iterate.  The host path runs twice with rng = default_rng(0), as it is and
with its tightening `refine_lm(iters=30, eps=1e-14)` turned into `iters=100, eps=1e-16`; s_g is the largest change of a gradient entry relative to
its pair's max |g|, s_l the relative change of the loss.  Gradient gate per pair: (100 s_g + 8 fp32 ulps of 1) x that pair's max |g|; loss gate:
100 s_l + 8 fp64 ulps, relative.  The factor 100 covers another stopping iterate in the same basin reached from another EPnP start (Jacobi
instead of LAPACK) and the difference between two central-difference Hessians, and stays more than an order of magnitude below the 6e-4 by which a
Gauss-Newton Hessian would change the gradient.  Poses use tests/test_pnp_twin_host.py's R / t gates.

The spreads of the other sets are taken over that set and "hard" together, as tests/test_pnp_twin_host.py does for its noisy nine-point sets: on
the small-residual sets (n = 5, n = 11 without outliers) both host runs stop at the same iterate, bit for bit, and a spread of exactly 0 is a
statement about the sample, not about the host path, whose stop (a relative cost decrease below 1e-14) leaves the iterate uncertain all the same.

Every comparison first asserts, on the host path's own output, that it means something: no |r - p'| or |gt - r| near 0 (the unit vectors), no
keypoint near the smooth-L1 knee or the cap, and both smooth-L1 branches and the cap present in the set.

The batches and references of this module are shared with tests/test_gpu_bpnp.py."""
from collections import namedtuple

import numpy as np
import pytest

import test_pnp_twin_host as T
from casapose_amd import _lib
from casapose_amd import training as TR
from casapose_amd.pose_estimation import pnp as P
from casapose_amd.pose_estimation.device_bpnp import DeviceBPnPLoss
from casapose_amd.pose_estimation.device_pnp import affine_from_offsets

CAP = 12.5
ULP32, ULP64 = float(np.spacing(np.float32(1.0))), float(np.spacing(1.0))
IDENTITY = np.float32([1, 0, 0, 0, 1, 0])
# coords [b,oc,kp,2] (y,x) crop pixels, gt [b,oc,kp,2] (x,y) image pixels, affine [b,6], avail [b,oc], points_3d [b,oc,kp,3]: all float32
Batch = namedtuple("Batch", "coords gt affine avail points_3d")
# the host path on a batch: loss, g [b,oc,kp,2], poses [b,oc,1,3,4], per-keypoint |d1|, |d2|, e, l before the cap (rows of available pairs),
# the stopping-iterate spreads and the gates
Reference = namedtuple("Reference", "loss g poses n1 n2 e l s_g s_l gate_g gate_l")


def _batch(cases, b, oc, gt_sigma, avail=None, affine=None):
    n = cases[0].points_3d.shape[0]
    xy, x3 = T.batch_of(cases, b, oc)   # crop pixels where the cases have them
    image_xy = np.stack([c.points_2d for c in cases]).astype(np.float64).reshape(b, oc, n, 2)
    gt = (image_xy + np.random.default_rng(3).normal(0, np.broadcast_to(gt_sigma, image_xy.shape))).astype(np.float32)
    return Batch(np.ascontiguousarray(xy[..., ::-1]), gt, np.tile(IDENTITY, (b, 1)) if affine is None else affine.astype(np.float32),
                 np.ones((b, oc), np.float32) if avail is None else avail.astype(np.float32), x3)


# For the sets other than "hard" the ground-truth noise cycles over the keypoints (0.4, 2, 30 px), so that a few keypoints lie on the quadratic
# branch and a few above the cap although these sets have few pairs or no planted outliers.
CYCLE = np.float64([0.4, 2.0, 30.0])


def make_batch(name) -> Batch:
    if name == "hard":       # 15 pairs as b = 3, oc = 5: 0.5 px noise, 0..2 planted outliers, gt = points + N(0, 2 px)
        return _batch(T.fixture_set("hard"), 3, 5, 2.0)
    if name == "percam":     # crop pixels under three crop offsets (shift, rotation, scale), one camera, some pairs unavailable
        rng = np.random.default_rng(19)
        cases = [T.make_case(rng, 9, 0.5, outliers, T.K32, T.PERCAM_OFFSETS[i]) for i, outliers in enumerate((0, 1, 2)) for _ in range(5)]
        return _batch(cases, 3, 5, np.resize(CYCLE, 9)[:, None], T.PERCAM_MASK, affine_from_offsets(T.PERCAM_OFFSETS))
    n = {"n5": 5, "n11": 11}[name]
    rng = np.random.default_rng(20 + n)
    return _batch([T.make_case(rng, n, sigma=0.5) for _ in range(2)], 1, 2, np.resize(CYCLE, n)[:, None])


def host_run(batch: Batch, monkeypatch, tighter=False, avail=None):
    """bpnp_reprojection_loss_host with rng = default_rng(0) -> (loss, g float64, poses, [(image points, model points, optimum)] per available
    pair in order).  tighter: its tightening LM runs with iters = 100, eps = 1e-16."""
    seen = []
    lm, backward = P.refine_lm, P.bpnp_backward

    def refine(*a, **k):
        if tighter and k.get("iters") == 30 and k.get("eps") == 1e-14:
            k = dict(k, iters=100, eps=1e-16)
        return lm(*a, **k)

    def record(grad_pose, points_2d, points_3d, K, pose6):
        seen.append((np.array(points_2d, np.float64), np.array(points_3d, np.float64), np.array(pose6, np.float64)))
        return backward(grad_pose, points_2d, points_3d, K, pose6)

    with monkeypatch.context() as m:
        m.setattr(P, "refine_lm", refine)
        m.setattr(P, "bpnp_backward", record)
        loss, g, poses = TR.bpnp_reprojection_loss_host(batch.coords, batch.gt, batch.affine, batch.avail if avail is None else avail, batch.points_3d,
                                                        T.K32, CAP, 1.0, rng=np.random.default_rng(0))
    return loss, g.astype(np.float64), poses, seen


_references = {}


def host_reference(name, monkeypatch) -> Reference:
    if name in _references:
        return _references[name]
    batch = make_batch(name)
    loss, g, poses, seen = host_run(batch, monkeypatch)
    loss2, g2, _, _ = host_run(batch, monkeypatch, tighter=True)
    kp = batch.coords.shape[2]
    on = batch.avail.reshape(-1) != 0
    gt = batch.gt.astype(np.float64).reshape(-1, kp, 2)[on]
    n1, n2 = [], []
    for (xy, X, y), gt_pair in zip(seen, gt):
        res, _ = P._residual_and_jacobian(X, xy, T.K32.astype(np.float64), y[:3], y[3:])
        r = res.reshape(kp, 2) + xy
        n1.append(np.linalg.norm(r - xy, axis=1))
        n2.append(np.linalg.norm(gt_pair - r, axis=1))
    n1, n2 = np.array(n1), np.array(n2)
    e = 0.5 * (n1 + n2)
    l = np.where(e < 1.0, 0.5 * e * e, e - 0.5)
    pair_max = np.abs(g).reshape(len(on), -1).max(axis=1)
    assert (pair_max[on] > 0).all() and not g.reshape(len(on), -1)[~on].any()
    s_g = float((np.abs(g2 - g).reshape(len(on), -1).max(axis=1)[on] / pair_max[on]).max())
    s_l = float(abs(loss2 - loss) / abs(loss))
    if name != "hard":   # the spread of the noisy family: see the module docstring
        s_g, s_l = max(s_g, host_reference("hard", monkeypatch).s_g), max(s_l, host_reference("hard", monkeypatch).s_l)
    ref = Reference(loss, g, poses, n1, n2, e, l, s_g, s_l, 100.0 * s_g + 8.0 * ULP32, 100.0 * s_l + 8.0 * ULP64)
    print("%s: host path s_g %.3g, s_l %.3g -> gradient gate %.3g x max|g| of the pair, loss gate %.3g" % (name, s_g, s_l, ref.gate_g, ref.gate_l))
    _references[name] = ref
    return ref


def assert_preconditions(ref: Reference, what):
    """on the host path's output: the unit vectors are defined, no keypoint sits at the smooth-L1 knee or at the cap, and every branch occurs"""
    print("%s: min |d1| %.3g, min |d2| %.3g, min |e - 1| %.3g, min |l - cap| %.3g; %d quadratic, %d linear, %d capped keypoints"
          % (what, ref.n1.min(), ref.n2.min(), np.abs(ref.e - 1.0).min(), np.abs(ref.l - CAP).min(), (ref.e < 1.0).sum(),
             ((ref.e >= 1.0) & (ref.l <= CAP)).sum(), (ref.l > CAP).sum()))
    assert ref.n1.min() > 1e-2 and ref.n2.min() > 1e-2, what
    assert np.abs(ref.e - 1.0).min() > 1e-4 and np.abs(ref.l - CAP).min() > 1e-4, what
    assert (ref.e < 1.0).any() and ((ref.e >= 1.0) & (ref.l <= CAP)).any() and (ref.l > CAP).any(), what


def assert_loss_and_gradient(loss, g, ref: Reference, what, want_loss=None, want_g=None):
    """every pair, none dropped: |g - host g| <= gate_g x that pair's max |host g|; the loss relative"""
    want_loss = ref.loss if want_loss is None else want_loss
    want_g = ref.g if want_g is None else want_g
    pairs = want_g.shape[0] * want_g.shape[1]
    pair_max = np.abs(want_g).reshape(pairs, -1).max(axis=1)
    diff = np.abs(np.asarray(g, np.float64) - want_g).reshape(pairs, -1).max(axis=1)
    live = pair_max > 0
    rel_g = float((diff[live] / pair_max[live]).max()) if live.any() else 0.0
    rel_l = abs(float(loss) - want_loss) / abs(want_loss) if want_loss != 0 else abs(float(loss))
    print("%s: max |dg| / max|g| of the pair %.3g (gate %.3g), relative loss difference %.3g (gate %.3g)" % (what, rel_g, ref.gate_g, rel_l, ref.gate_l))
    assert (diff <= ref.gate_g * pair_max).all(), "%s: gradient differs by %.3g of the pair's max |g| (gate %.3g)" % (what, rel_g, ref.gate_g)
    assert rel_l <= ref.gate_l, "%s: loss differs by %.3g relative (gate %.3g)" % (what, rel_l, ref.gate_l)


def assert_poses(poses, ref: Reference, on, what):
    pose_ref = T.host_reference("hard")   # the R / t gates of the nine-point noisy sets
    got, want = np.asarray(poses).reshape(-1, 3, 4), ref.poses.reshape(-1, 3, 4)
    T.assert_within_gates(got[on], want[on], pose_ref, what)
    assert not got[~on].any(), what


def twin_call(batch: Batch, weight=1.0, avail=None, cap=CAP):
    twin = DeviceBPnPLoss(None, batch.coords.shape[2])
    loss, g, poses = twin.loss_and_grad_host(batch.coords, batch.gt, batch.affine, batch.avail if avail is None else avail, batch.points_3d, T.K32, cap, weight)
    return loss, g, poses, twin


def collapsed(batch: Batch, pair=(1, 2)) -> Batch:
    coords = batch.coords.copy()
    coords[pair] = np.float32([207.25, 311.5])   # every vote of the pair at one pixel
    return batch._replace(coords=coords)


def test_hard_set_against_the_host_path(monkeypatch):
    batch, ref = make_batch("hard"), host_reference("hard", monkeypatch)
    assert_preconditions(ref, "hard")
    loss, g, poses, twin = twin_call(batch)
    assert g.dtype == np.float32 and g.shape == (3, 5, 9, 2) and poses.shape == (3, 5, 1, 3, 4) and poses.dtype == np.float32
    assert twin.last_counts.tolist() == [15, 0] and (twin.last_info[..., 0] == 0).all()
    for i, c in enumerate(T.fixture_set("hard")):
        assert twin.last_info.reshape(15, 4)[i, 2] >= 9 - c.outliers and 1 <= twin.last_info.reshape(15, 4)[i, 3] <= 20
    assert_loss_and_gradient(loss, g, ref, "twin against the host path, hard")
    assert_poses(poses, ref, np.ones(15, bool), "twin against the host path, hard")


def test_crop_affines_and_unavailable_pairs(monkeypatch):
    batch, ref = make_batch("percam"), host_reference("percam", monkeypatch)
    assert_preconditions(ref, "percam")
    loss, g, poses, twin = twin_call(batch)
    on = T.PERCAM_MASK.reshape(15) != 0
    assert twin.last_counts.tolist() == [int(on.sum()), 0]
    assert np.array_equal(twin.last_info.reshape(15, 4)[:, 0], np.where(on, 0, 1))
    assert not g.reshape(15, -1)[~on].any(), "an unavailable pair has exactly zero gradient"
    assert_loss_and_gradient(loss, g, ref, "twin against the host path, crop affines")
    assert_poses(poses, ref, on, "twin against the host path, crop affines")


@pytest.mark.parametrize("name", ["n5", "n11"])
def test_other_point_counts(monkeypatch, name):
    batch, ref = make_batch(name), host_reference(name, monkeypatch)
    assert_preconditions(ref, name)
    loss, g, poses, twin = twin_call(batch)
    assert twin.last_counts.tolist() == [2, 0] and twin.hypotheses == (1 if name == "n5" else 256)
    assert_loss_and_gradient(loss, g, ref, "twin against the host path, %s" % name)
    assert_poses(poses, ref, np.ones(2, bool), "twin against the host path, %s" % name)


def test_gradient_by_central_differences_of_the_twins_own_loss():
    """step 2^-10 px on the fp32 coordinates (exact below 2^13 px), every second keypoint of two pairs: one with a planted outlier, one without;
    the PnP is re-solved at every perturbed point set.  Tolerance: tests/test_pose_host.py's for the same check of the host path."""
    hard = make_batch("hard")
    batch = Batch(*(a.reshape((15,) + a.shape[2:])[[1, 7]][None] for a in (hard.coords, hard.gt)), hard.affine[:1], hard.avail[:1, :2],
                  hard.points_3d.reshape(15, 9, 3)[[1, 7]][None])
    h = 2.0 ** -10
    loss, g, _, twin = twin_call(batch)
    assert twin.last_counts.tolist() == [2, 0] and np.isfinite(loss)
    num = np.zeros(batch.coords.shape)
    for o in range(2):
        for j in range(0, 9, 2):
            for a in range(2):
                up, down = batch.coords.copy(), batch.coords.copy()
                up[0, o, j, a] += np.float32(h)
                down[0, o, j, a] -= np.float32(h)
                assert up[0, o, j, a] - down[0, o, j, a] == 2 * h
                num[0, o, j, a] = (twin_call(batch._replace(coords=up))[0] - twin_call(batch._replace(coords=down))[0]) / (2 * h)
    m = num != 0
    assert m.sum() == 20
    print("central differences: max |g - num| %.3g of max |num| %.3g" % (np.abs(g[m] - num[m]).max(), np.abs(num[m]).max()))
    assert np.abs(g[m] - num[m]).max() < 2e-2 * np.abs(num[m]).max()


def test_collapsed_vote_is_unsolved_and_all_unavailable_is_zero(monkeypatch):
    hard, ref = make_batch("hard"), host_reference("hard", monkeypatch)
    batch = collapsed(hard)
    loss, g, poses, twin = twin_call(batch)
    assert twin.last_counts.tolist() == [14, 1] and twin.last_info[1, 2].tolist() == [3, -1, 0, 0]
    assert not g[1, 2].any() and not poses[1, 2].any()
    cleared = hard.avail.copy()
    cleared[1, 2] = 0
    want_loss, want_g, _, _ = host_run(hard, monkeypatch, avail=cleared)
    assert_loss_and_gradient(loss, g, ref, "collapsed vote against the host path without that pair", want_loss, want_g)
    loss, g, poses, twin = twin_call(hard, avail=np.zeros((3, 5), np.float32))
    assert loss == 0.0 and not g.any() and not poses.any() and twin.last_counts.tolist() == [0, 0] and (twin.last_info[..., 0] == 1).all()
    nan = hard.coords.copy()
    nan[0, 0, 4, 1] = np.nan
    loss, g, _, twin = twin_call(hard._replace(coords=nan))
    assert twin.last_counts.tolist() == [14, 1] and twin.last_info[0, 0, 0] == 2 and np.isfinite(loss) and np.isfinite(g).all() and not g[0, 0].any()


def test_weight_scales_exactly_and_calls_repeat_bit_for_bit():
    batch = make_batch("hard")
    loss, g, poses, _ = twin_call(batch)
    loss2, g2, poses2, _ = twin_call(batch)
    assert loss == loss2 and np.array_equal(g, g2) and np.array_equal(poses, poses2)
    for w in (0.5, 0.0078125):
        lw, gw, _, _ = twin_call(batch, weight=w)
        assert lw == loss and np.array_equal(gw, np.float32(w) * g)
    assert not twin_call(batch, weight=0.0)[1].any()


def test_argument_validation():
    batch = make_batch("hard")
    for n in (4, 17):
        with pytest.raises(ValueError, match="host path"):
            DeviceBPnPLoss(None, n)
    twin = DeviceBPnPLoss(None, 9)
    args = (batch.coords, batch.gt, batch.affine, batch.avail, batch.points_3d, T.K32)
    with pytest.raises(ValueError, match="coords_yx"):
        twin.loss_and_grad_host(batch.coords[:, :, :8], *args[1:])
    with pytest.raises(ValueError, match="gt_xy"):
        twin.loss_and_grad_host(batch.coords, batch.gt[:, :4], *args[2:])
    with pytest.raises(_lib.CasaposeHipError, match="max_pixel_error must be positive"):
        twin.loss_and_grad_host(*args, 0.0)
    with pytest.raises(_lib.CasaposeHipError, match="weight must be finite"):
        twin.loss_and_grad_host(*args, CAP, float("nan"))
    with pytest.raises(_lib.CasaposeHipError, match="reprojection_error must be positive"):
        DeviceBPnPLoss(None, 9, reprojection_error=0.0).loss_and_grad_host(*args, CAP)
    with pytest.raises(_lib.CasaposeHipError, match="loss_and_grad_host"):
        twin.loss_and_grad(*args, CAP)
    bad = DeviceBPnPLoss(None, 9)
    bad.table_host = bad.table_host.copy()
    bad.table_host[3, 4] = 9
    with pytest.raises(_lib.CasaposeHipError, match="hypothesis 3 names point 9 of 9"):
        bad.loss_and_grad_host(*args, CAP)
    lib = _lib.load()
    assert lib.cp_bpnp_loss_workspace_bytes(3, 5, 9) == (3 * 5 * 18 + 15) * 8 and lib.cp_bpnp_loss_workspace_bytes(0, 5, 9) == 0
    p = [16] * 7
    out = [16] * 6
    assert lib.cp_bpnp_loss_host_f64(None, *p[1:], 3, 5, 9, 126, 12.0, CAP, 1.0, *out) == -1 and b"null pointer" in lib.cp_last_error()
    assert lib.cp_bpnp_loss_f64(*p, 3, 5, 9, 126, 12.0, CAP, 1.0, *out[:5], None, None) == -1 and b"null pointer" in lib.cp_last_error()
    for kp in (4, 17):
        assert lib.cp_bpnp_loss_f64(*p, 3, 5, kp, 126, 12.0, CAP, 1.0, *out, None) == -1 and b"kp must lie in [5, 16]" in lib.cp_last_error()
    assert lib.cp_bpnp_loss_f64(*p, 3, 5, 9, 257, 12.0, CAP, 1.0, *out, None) == -1 and b"H must lie in [1, 256]" in lib.cp_last_error()
    assert lib.cp_bpnp_loss_f64(*p, 256, 256, 9, 126, 12.0, CAP, 1.0, *out, None) == -1 and b"65535" in lib.cp_last_error()
    assert lib.cp_bpnp_loss_f64(*p, 0, 5, 9, 126, 12.0, CAP, 1.0, *out, None) == -1 and b"positive" in lib.cp_last_error()
