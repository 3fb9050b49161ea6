"""cp_pose_match_f32 (csrc/pose_match.hip) and DeviceInstanceEvaluator on the GPU against match_instances_host in fp64, fed the same
fp32-rounded inputs, and bit for bit against cp_pose_eval_f32 on the same (estimate, instance) pairs.

Gates: those of tests/test_gpu_pose_eval.py, whose header derives them.  S = the largest |camera-frame coordinate| of the scene, every point
keeps z >= S / 2 (asserted): 3-D |dev - ref| <= 4e-6 * S, 2-D |dev - ref| <= 2e-6 * (f + max(W, H)).  Matches, flags and tallies must be equal;
the scene is built (its seed picked on the CPU, the property asserted on the fp64 reference) so that within a group all finite costs differ by
more than 10 gates and no error lies within 10 gates of its threshold: no rounding can change a match or a flag.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K32 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
GATE_2D = 2e-6 * (float(K32[1, 1]) + 640.0)
ALLOWED_2D = 5.0


def gate_3d(s):
    return 4e-6 * s


def rodrigues(rv):
    from casapose_amd.pose_estimation import pnp as P

    return P.rodrigues(np.asarray(rv, np.float64))


def pose32(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32)


def spread_translations(rng, n, apart=150.0, half=(150.0, 100.0), depth=(700.0, 1100.0)):
    """n camera-frame positions at least `apart` mm from each other"""
    out = []
    while len(out) < n:
        t = np.array([rng.uniform(-half[0], half[0]), rng.uniform(-half[1], half[1]), rng.uniform(*depth)])
        if all(np.linalg.norm(t - u) >= apart for u in out):
            out.append(t)
    return out


def perturbed(rng, gt, shift, degrees):
    """the pose moved by `shift` mm in a random direction and turned by `degrees` about a random axis through the object's origin"""
    d, a = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
    R = rodrigues(a / np.linalg.norm(a) * np.deg2rad(degrees)) @ gt[:, :3].astype(np.float64)
    return pose32(R, gt[:, 3].astype(np.float64) + d / np.linalg.norm(d) * shift)


COUNTS, FLAGS, VMAX = [300, 1030, 7], [0, 1, 1], 1030     # a partial chunk; five chunks and a second LDS tile of 6 points; fewer than TILE_UNROLL
GT_COUNTS = np.array([[3, 2, 1], [0, 3, 2]], np.int32)
# per group the ground-truth instance each slot estimates (None: an empty slot; "x": one more estimate, of instance 0, pushed far off)
SLOTS = [[(2, 0, 1), (1, "x", 0), (None, 0, None)],
         [("x", "x", None), (2, None, 0), (None, None, None)]]   # estimates without ground truth; one instance missed; ground truth without estimates


def build_scene(seed):
    rng = np.random.default_rng(seed)
    b, oc, R, I = 2, 3, 3, 3
    mesh = np.full((oc, VMAX, 3), np.nan, np.float32)          # rows counts[o] .. vmax-1 must never be read
    for o, c in enumerate(COUNTS):
        mesh[o, :c] = rng.uniform(-50, 50, (c, 3))
    diam = np.array([140.0, 150.0, 120.0], np.float32)
    gt = np.full((b, oc, I, 3, 4), np.nan, np.float32)         # rows at and beyond the group's count must never be read
    est = np.zeros((b, oc, R, 3, 4), np.float32)
    for n in range(b):
        for o in range(oc):
            where = spread_translations(rng, I)
            for g in range(I):
                gt[n, o, g] = pose32(rodrigues(rng.normal(0, 1, 3)), where[g])
            truth = gt[n, o].copy()                          # all I poses are drawn; those at and beyond the count become NaN below
            for e, g in enumerate(SLOTS[n][o]):
                if g is None:
                    continue
                if g == "x":
                    est[n, o, e] = perturbed(rng, truth[0], rng.uniform(60.0, 90.0), rng.uniform(0.0, 20.0))
                else:
                    est[n, o, e] = perturbed(rng, truth[g], float(np.exp(rng.uniform(np.log(0.5), np.log(40.0)))), rng.uniform(0.0, 20.0))
            gt[n, o, GT_COUNTS[n, o]:] = np.nan
    cams = np.tile(K32[None], (b, 1, 1))
    return dict(mesh=mesh, counts=np.array(COUNTS, np.int32), flags=FLAGS, diam=diam, gt=gt, est=est, gt_counts=GT_COUNTS, cams=cams)


def extent(sc):
    """(S, smallest z) over every transformed point of the scene, fp64"""
    big, zmin = 0.0, np.inf
    for o, c in enumerate(sc["counts"]):
        X = sc["mesh"][o, :c].astype(np.float64)
        for P in list(sc["est"][:, o].reshape(-1, 3, 4)) + list(sc["gt"][:, o].reshape(-1, 3, 4)):
            if np.isnan(P).any() or not P.any():
                continue
            cam = X @ P[:, :3].T.astype(np.float64) + P[:, 3].astype(np.float64)
            big, zmin = max(big, np.abs(cam).max()), min(zmin, cam[:, 2].min())
    return big, zmin


def reference(sc):
    from casapose_amd.pose_estimation.instance_evaluation import match_instances_host

    return match_instances_host(sc["est"], sc["gt"], sc["gt_counts"], sc["mesh"], sc["counts"], sc["cams"], sc["diam"], symmetric=sc["flags"],
                                allowed_error_2d=ALLOWED_2D)


def margins(sc, ref):
    """(the smallest difference of two finite costs of one group, the smallest |err_3d - 0.1 diameter|, the smallest |err_2d - allowed|)"""
    err = ref[0]
    cost_gap, gap3, gap2 = np.inf, np.inf, np.inf
    for n in range(err.shape[0]):
        for o in range(err.shape[1]):
            c = err[n, o, :, :, 1]
            c = np.sort(c[np.isfinite(c)])
            if len(c) > 1:
                cost_gap = min(cost_gap, np.diff(c).min())
            if len(c):
                gap3 = min(gap3, np.abs(c - 0.1 * float(sc["diam"][o])).min())
                e2 = err[n, o, :, :, 0]
                gap2 = min(gap2, np.abs(e2[np.isfinite(e2)] - ALLOWED_2D).min())
    return cost_gap, gap3, gap2


def well_separated(sc, ref):
    s, zmin = extent(sc)
    cost_gap, gap3, gap2 = margins(sc, ref)
    return zmin >= s / 2 and cost_gap > 10 * gate_3d(s) and gap3 > 10 * gate_3d(s) and gap2 > 10 * GATE_2D


def as_meant(ref):
    """every estimate goes to the instance it was made for; the far ones ("x") stay without"""
    em = ref[2]
    return (em[0, 0].tolist() == [2, 0, 1] and em[0, 1].tolist() == [1, -1, 0] and em[0, 2].tolist() == [-2, 0, -2] and em[1, 0].tolist() == [-1, -1, -2]
            and em[1, 1].tolist() == [2, -2, 0] and em[1, 2].tolist() == [-2, -2, -2])


@functools.lru_cache(maxsize=None)
def main_scene():
    """the first seed whose scene is well separated and holds matches on both sides of 0.1 diameters (decided on the CPU, in fp64)"""
    for seed in range(64):
        sc = build_scene(seed)
        ref = reference(sc)
        valid = ref[1][..., 3][ref[1][..., 0] >= 0]
        if well_separated(sc, ref) and as_meant(ref) and valid.min() == 0 and valid.max() == 1:
            for a in list(sc.values()) + list(ref):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            return sc, ref
    raise AssertionError("no seed below 64 gives a well separated scene")


def evaluator_of(sc, device):
    from casapose_amd.pose_estimation.instance_evaluation import DeviceInstanceEvaluator

    return DeviceInstanceEvaluator(sc["mesh"], sc["counts"], device, symmetric=sc["flags"])


def run(sc, device):
    return evaluator_of(sc, device).match(sc["est"], sc["gt"], sc["gt_counts"], sc["cams"], sc["diam"], ALLOWED_2D)


def assert_against_reference(got, ref, s, where=""):
    err, rec, em, tally = got
    rerr, rrec, rem, rtally = ref
    finite = np.isfinite(rerr)
    assert np.array_equal(np.isposinf(err), ~finite), where
    d2 = np.abs(err[..., 0][finite[..., 0]] - rerr[..., 0][finite[..., 0]]).max() if finite.any() else 0.0
    d3 = np.abs(err[..., 1][finite[..., 1]] - rerr[..., 1][finite[..., 1]]).max() if finite.any() else 0.0
    print("%s max |err_2d - ref| = %.3g (gate %.3g), max |err_3d - ref| = %.3g (gate %.3g)" % (where, d2, GATE_2D, d3, gate_3d(s)))
    assert d2 <= GATE_2D and d3 <= gate_3d(s), where
    assert np.array_equal(rec[..., 0], rrec[..., 0]) and np.array_equal(em, rem) and np.array_equal(tally, rtally), where
    assert np.array_equal(rec[..., 3:], rrec[..., 3:]), where
    assert np.abs(rec[..., 1] - rrec[..., 1]).max() <= GATE_2D and np.abs(rec[..., 2] - rrec[..., 2]).max() <= gate_3d(s), where


def test_main_scene_against_the_host_reference(device):
    sc, ref = main_scene()
    s, zmin = extent(sc)
    cost_gap, gap3, gap2 = margins(sc, ref)
    print("S = %.1f, z >= %.1f; cost gap %.3g, threshold gaps %.3g (3-D), %.3g (2-D); gates %.3g, %.3g" % (s, zmin, cost_gap, gap3, gap2, gate_3d(s), GATE_2D))
    # the precondition, on the fp64 reference: asserted, never skipped
    assert zmin >= s / 2 and cost_gap > 10 * gate_3d(s) and gap3 > 10 * gate_3d(s) and gap2 > 10 * GATE_2D
    rerr, rrec, rem, rtally = ref
    # what the scene is meant to hold
    assert sorted(set(sc["gt_counts"].reshape(-1).tolist())) == [0, 1, 2, 3]
    assert rtally[1, 0].tolist() == [0, 2, 0, 0, 0] and rem[1, 0].tolist() == [-1, -1, -2]          # estimates without ground truth
    assert rtally[1, 2].tolist() == [2, 0, 0, 0, 0] and rem[1, 2].tolist() == [-2, -2, -2]          # ground truth without estimates
    assert as_meant(ref)
    assert rrec[1, 1, :, 0].tolist() == [2, -1, 0]
    got = run(sc, device)
    assert got[0].dtype == np.float32 and got[0].shape == (2, 3, 3, 3, 2) and got[1].shape == (2, 3, 3, 5)
    assert got[2].dtype == np.int32 and got[2].shape == (2, 3, 3) and got[3].dtype == np.int32 and got[3].shape == (2, 3, 5)
    assert_against_reference(got, ref, s, "main scene:")


def test_errors_equal_cp_pose_eval_bit_for_bit(device):
    """every finite err[b, o, e, g] is records 0 and 1 of cp_pose_eval_f32 on the pair (estimate e, instance g, valid 1): one copy of the
    arithmetic, one order of summation"""
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    sc, _ = main_scene()
    err = run(sc, device)[0]
    ev = DevicePoseEvaluator(sc["mesh"], sc["counts"], device, symmetric=sc["flags"])
    b, oc, R, I = err.shape[:4]
    diam = np.tile(sc["diam"][None, :, None], (b, 1, 1))
    compared = 0
    for e in range(R):
        for g in range(I):
            ev.evaluate(sc["est"][:, :, e], sc["gt"][:, :, g][:, :, None], sc["cams"], diam, np.ones((b, oc), np.float32), ALLOWED_2D)
            on = np.isfinite(err[:, :, e, g, 1])
            assert np.array_equal(err[:, :, e, g][on].view(np.uint32), ev.last_records[..., :2][on].view(np.uint32)), (e, g)
            compared += int(on.sum())
    assert compared == 3 * 3 + 3 * 2 + 1 + 2 * 3


def test_one_estimate_one_instance_gives_the_records_of_cp_pose_eval(device):
    from casapose_amd.pose_estimation.device_evaluation import DevicePoseEvaluator

    sc, _ = main_scene()
    est, gt, counts = sc["est"][:, :, 1:2], sc["gt"][:, :, :1], np.minimum(sc["gt_counts"], 1)
    err, rec, em, tally = evaluator_of(sc, device).match(est, gt, counts, sc["cams"], sc["diam"], ALLOWED_2D)
    ev = DevicePoseEvaluator(sc["mesh"], sc["counts"], device, symmetric=sc["flags"])
    ev.evaluate(est[:, :, 0], gt, sc["cams"], np.tile(sc["diam"][None, :, None], (2, 1, 1)), np.ones((2, 3), np.float32), ALLOWED_2D)
    on = tally[..., 2] == 1
    assert on.sum() >= 2 and np.array_equal(on, em[..., 0] == 0)
    assert np.array_equal(rec[:, :, 0, 1:5][on].view(np.uint32), ev.last_records[..., 0:4][on].view(np.uint32))
    assert np.all(rec[:, :, 0][~on] == [-1, 0, 0, 0, 0])


def test_two_calls_give_identical_bytes(device):
    sc, _ = main_scene()
    ev = evaluator_of(sc, device)
    first = ev.match(sc["est"], sc["gt"], sc["gt_counts"], sc["cams"], sc["diam"], ALLOWED_2D)
    second = ev.match(sc["est"], sc["gt"], sc["gt_counts"], sc["cams"], sc["diam"], ALLOWED_2D)
    for a, c in zip(first, second):
        assert a.tobytes() == c.tobytes()
    assert all(a is c for a, c in zip(second, (ev.last_err, ev.last_gt_rec, ev.last_est_match, ev.last_tally)))


def test_identical_estimates_slot_0_matches_slot_1_is_the_false_positive(device):
    sc, _ = main_scene()
    gt = sc["gt"][:1, :, :1]
    one = perturbed(np.random.default_rng(5), gt[0, 1, 0], 2.0, 1.0)
    est = np.zeros((1, 3, 2, 3, 4), np.float32)
    est[0, 1, 0] = est[0, 1, 1] = one
    err, rec, em, tally = evaluator_of(sc, device).match(est, gt, np.array([[1, 1, 1]], np.int32), sc["cams"][:1], sc["diam"], ALLOWED_2D)
    assert err[0, 1, 0, 0].tobytes() == err[0, 1, 1, 0].tobytes() and np.isfinite(err[0, 1]).all()
    assert em[0].tolist() == [[-2, -2], [0, -1], [-2, -2]] and rec[0, 1, 0, 0] == 0 and tally[0].tolist() == [[1, 0, 0, 0, 0], [1, 2, 1, 1, 1], [1, 0, 0, 0, 0]]


def test_sixteen_by_sixteen_recovers_the_permutation(device):
    """R = I = 16, two objects of 64 points (one symmetric): the estimates are a permutation of the ground truth moved by 0.2 mm"""
    rng = np.random.default_rng(16)
    mesh = rng.uniform(-40, 40, (2, 64, 3)).astype(np.float32)
    gt, est, perm = np.zeros((1, 2, 16, 3, 4), np.float32), np.zeros((1, 2, 16, 3, 4), np.float32), np.zeros((2, 16), np.int64)
    for o in range(2):
        where = spread_translations(rng, 16, half=(450.0, 350.0))
        perm[o] = rng.permutation(16)
        for g in range(16):
            gt[0, o, g] = pose32(rodrigues(rng.normal(0, 1, 3)), where[g])
        for e in range(16):
            est[0, o, e] = perturbed(rng, gt[0, o, perm[o, e]], 0.2, 0.0)
    sc = dict(mesh=mesh, counts=np.array([64, 64], np.int32), flags=[0, 1], diam=np.array([120.0, 120.0], np.float32), gt=gt, est=est,
              gt_counts=np.full((1, 2), 16, np.int32), cams=K32[None])
    ref = reference(sc)
    assert np.array_equal(ref[2][0], perm) and ref[3].tolist() == [[[16, 16, 16, 16, 16]] * 2]
    s, _ = extent(sc)
    # every estimate has one instance within 0.25 mm and every other one beyond 50 mm: no rounding, and no order among the sixteen nearly equal
    # smallest costs, can change the assignment
    own = np.take_along_axis(ref[0][0, ..., 1], perm[:, :, None], axis=2)[..., 0]
    others = np.sort(ref[0][0, ..., 1], axis=2)[..., 1]
    assert own.max() < 0.25 and others.min() > 50.0
    err, rec, em, tally = run(sc, device)
    assert np.array_equal(em[0], perm) and tally.tolist() == [[[16, 16, 16, 16, 16]] * 2]
    assert np.array_equal(rec[..., 0], ref[1][..., 0]) and np.all(rec[..., 3:] == 1) and rec[..., 2].max() < 0.25
    assert np.isfinite(err).all() and np.abs(err[..., 1] - ref[0][..., 1]).max() <= gate_3d(s)


def oracle_output(batch, i):
    """the network output a perfect network would give for image i: 10 x one-hot segmentation, unit directions (dy, dx) from every pixel centre to
    the keypoints of its own instance (by instance_seg), zero confidence -> float32 [1, h, w, K + 2 kp + kp]"""
    seg = batch["target_seg"][i].numpy()
    lab, iseg = batch["filtered_seg"][i, ..., 0].numpy(), batch["instance_seg"][i].numpy()
    kp2 = batch["target_vert"][i].numpy().astype(np.float64)              # [oc, I, kp, 2] (y, x)
    h, w = lab.shape
    kp = kp2.shape[2]
    yy, xx = np.mgrid[0:h, 0:w] + 0.5
    dirs = np.zeros((h, w, kp, 2))
    for o in range(kp2.shape[0]):
        for r in range(kp2.shape[1]):
            on = (lab == o + 1) & (iseg == r)
            if not on.any():
                continue
            d = kp2[o, r][None, :, :] - np.stack([yy[on], xx[on]], axis=-1)[:, None, :]
            dirs[on] = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-12)
    return np.concatenate([10.0 * seg, dirs.reshape(h, w, 2 * kp), np.zeros((h, w, kp))], axis=-1).astype(np.float32)[None]


def grown(mask):
    out = np.zeros_like(mask)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out[max(dy, 0):mask.shape[0] + min(dy, 0), max(dx, 0):mask.shape[1] + min(dx, 0)] |= \
                mask[max(-dy, 0):mask.shape[0] + min(-dy, 0), max(-dx, 0):mask.shape[1] + min(-dx, 0)]
    return out


def one_piece(mask):
    """the mask is one 8-connected component (an occluder has not cut the instance in two)"""
    seed = np.zeros_like(mask)
    seed[tuple(np.argwhere(mask)[0])] = True
    while True:
        more = grown(seed) & mask
        if more.sum() == seed.sum():
            return bool(more.sum() == mask.sum())
        seed = more


def clean_image(batch, i, min_pixels=300):
    """every instance of image i has at least min_pixels pixels in one piece, and no two instances of one object touch (8-neighbourhood)"""
    lab, iseg = batch["filtered_seg"][i, ..., 0].numpy(), batch["instance_seg"][i].numpy()
    for o in range(batch["instance_count"].shape[1]):
        masks = [(lab == o + 1) & (iseg == r) for r in range(int(batch["instance_count"][i, o]))]
        if any(m.sum() < min_pixels or not one_piece(m) for m in masks):
            return False
        for a in range(len(masks)):
            if any((grown(masks[a]) & masks[c]).any() for c in range(len(masks)) if c != a):
                return False
    return True


def test_evaluate_instance_batch_on_an_oracle_field(device):
    import torch

    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_estimation.instance_evaluation import DeviceInstanceEvaluator, crop_cameras, evaluate_instance_batch, summarise
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    ds = SyntheticSceneDataset(2, (128, 160), instances=2)
    batch = ds.batch(0, 6)
    clean = [i for i in range(6) if clean_image(batch, i)]
    assert len(clean) >= 2, "the stream's first images have to hold clean ones"
    mesh, counts = ds.generate_object_vertex_array()
    evaluator = DeviceInstanceEvaluator(mesh, counts, device, symmetric=[0, 1])
    voter = InstanceLSVoting(name="coords_ls_voting", num_classes=3, num_points=9, max_instances=2)
    cams = crop_cameras(batch["cam_mat"], batch["offsets"])
    tallies, records = [], []
    for i in clean:
        one = {k: v[i:i + 1] for k, v in batch.items()}
        err, rec, em, tally = evaluate_instance_batch(one, torch.from_numpy(oracle_output(batch, i)).to(device), voter, evaluator, ds.keypoints3d, cams[i],
                                                      min_num=20, rng=np.random.default_rng(0))
        assert evaluator.last_poses.shape == (1, 2, 2, 3, 4)
        assert np.array_equal(tally[0, :, 0], batch["instance_count"][i].numpy())
        tallies.append(tally)
        records.append(rec)
    s = summarise(np.concatenate(tallies), np.concatenate(records))
    print("oracle field, images %s: %s" % (clean, s["all"]))
    for row in s["objects"] + [s["all"]]:
        assert row["recall_add"] == 1.0 and row["precision_add"] == 1.0 and row["recall_2d"] == 1.0 and row["precision_2d"] == 1.0
    rec = np.concatenate(records)
    matched = rec[..., 0] >= 0
    assert (rec[..., 2] / ds.diameters[None, :, None].astype(np.float32))[matched].max() < 0.01      # far below 0.1 diameters


def raw_call(hip_lib, device, b=1, oc=1, vmax=8, R=2, I=2, null=None):
    """cp_pose_match_f32 on small buffers, the outputs pre-filled with a sentinel -> (status, the outputs afterwards)"""
    import torch

    t = lambda n, dt, v=0: torch.full((max(n, 1),), v, dtype=dt, device=device)  # noqa: E731
    rr, ii = min(max(R, 1), 16), min(max(I, 1), 16)
    bufs = dict(points=t(oc * vmax * 3, torch.float32, 1.0), counts=t(oc, torch.int32, vmax), symmetric=t(oc, torch.int32), est=t(min(b, 4) * oc * rr * 12, torch.float32, 1.0),
                gt=t(min(b, 4) * oc * ii * 12, torch.float32, 1.0), gt_counts=t(min(b, 4) * oc, torch.int32, 1), cams=t(min(b, 4) * 9, torch.float32, 1.0),
                diameters=t(oc, torch.float32, 1.0), workspace=t(1024, torch.float64))
    outs = dict(err=t(min(b, 4) * oc * rr * ii * 2, torch.float32, -7.0), gt_rec=t(min(b, 4) * oc * ii * 5, torch.float32, -7.0),
                est_match=t(min(b, 4) * oc * rr, torch.int32, -7), tally=t(min(b, 4) * oc * 5, torch.int32, -7))
    p = {k: (None if k == null else v.data_ptr()) for k, v in {**bufs, **outs}.items()}
    status = hip_lib.cp_pose_match_f32(p["points"], p["counts"], p["symmetric"], oc, vmax, p["est"], R, p["gt"], I, p["gt_counts"], p["cams"], p["diameters"], b,
                                       5.0, p["workspace"], p["err"], p["gt_rec"], p["est_match"], p["tally"], torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    return status, outs


@pytest.mark.parametrize("kw, words", [
    (dict(R=0), "slots and instances must lie in 1..16"), (dict(R=17), "slots and instances must lie in 1..16"),
    (dict(I=0), "slots and instances must lie in 1..16"), (dict(I=17), "slots and instances must lie in 1..16"),
    (dict(b=4096, R=16, I=1), "more than 65535 (image, object, slot) rows"), (dict(null="gt_counts"), "null pointer"), (dict(null="tally"), "null pointer"),
    (dict(vmax=0), "must be positive"), (dict(b=0), "must be positive"),
])
def test_bad_arguments_are_refused_by_name_and_launch_nothing(device, hip_lib, kw, words):
    from casapose_amd import _lib

    status, outs = raw_call(hip_lib, device, **kw)
    assert status != 0
    message = hip_lib.cp_last_error().decode()
    assert message.startswith("cp_pose_match_f32:") and words in message, message
    assert all(bool((v == -7).all()) for v in outs.values())                    # nothing was written
    with pytest.raises(_lib.CasaposeHipError, match="cp_pose_match_f32"):
        _lib.check(status, "cp_pose_match_f32")


def test_workspace_bytes_and_the_wrapper_raises(device, hip_lib):
    from casapose_amd import _lib

    assert hip_lib.cp_pose_match_workspace_bytes(2, 3, 1030, 3, 3) == 2 * 3 * 3 * 5 * 3 * 2 * 8
    assert hip_lib.cp_pose_match_workspace_bytes(2, 3, 1030, 17, 3) == 0 and hip_lib.cp_pose_match_workspace_bytes(2, 3, 1030, 3, 0) == 0
    sc, _ = main_scene()
    too_many = np.zeros((2, 3, 17, 3, 4), np.float32)
    with pytest.raises(_lib.CasaposeHipError, match="slots and instances"):
        evaluator_of(sc, device).match(too_many, sc["gt"], sc["gt_counts"], sc["cams"], sc["diam"])
    status, outs = raw_call(hip_lib, device)                                        # the same buffers with good sizes do run
    assert status == 0 and outs["tally"][:5].tolist() == [1, 2, 1, 1, 1]
