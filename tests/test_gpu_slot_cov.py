"""cp_ls_slot_covariance_f32 (csrc/ls_vote.hip, csrc/ls_cov_math.h) stage by stage against tests/slot_cov_reference.py, at the smallest shapes
at which the walk of the two kernels can go wrong:
    48 x 64   whole strips of 64 x 16, label words          37 x 50   a partial strip, W % 4 != 0: byte labels
    33 x 130  three strips across, a 17th and a 33rd row    batch 2 everywhere, the second image the first one's map mirrored
    rec36     the production record: ls_accumulate36_slots_kernel<LS_MOMENTS>
    rec40s    ld = 40, every offset shifted, sigmoid weights: ls_accumulate_kernel<9, LS_MOMENTS>
    rec64     ld = 64 beside 254 slots: the LDS ceiling of the generic kernel
    4 slots (labels 1..4 and a label 7, above `slots`) and 254 slots (labels 1, 130, 253, 254 and a label 255); cut-off none and 4 px.
The fields are noisy (directions turned by N(0, 0.05 rad), estimates N(0, 0.3 px) off the planted keypoints) so that Q is not rounding; 2 % of
the directions are (0, 0); the third blob's directions are all (1, 0) (rank one); one estimate is NaN.  Every float no kernel may use is NaN.

THE FIVE SUMS are compared with the reference's fp64 sums on the measure |sum - ref| / sum |term|, gated as tests/test_gpu_ls_robust.py gates
the reweighted sums: four times the distance, on that measure and on the same run, between the reference's two restatements (fp32 in the
header's order against fp64 throughout), measured on the CPU -- but not less than FWD_GATE of the layout (tests/test_gpu_ls_stages.py).

THE FINISH is compared with the fp64 finish (slot_cov_reference.finish) of the device's own sums: 3 * 2^-24 |ref| for the rounding of the
output to fp32 plus 1e-10 * cond * the largest entry for the determinant's cancellation, as solve_tolerance of test_gpu_ls_stages has it."""
import functools

import numpy as np
import pytest
import torch

import slot_cov_reference as SC
from test_gpu_ls_stages import FWD_GATE, _labels_on_device

KP = 9
CUTOFFS = (None, 4.0)
SHAPES = {"48x64": (48, 64), "37x50": (37, 50), "33x130": (33, 130)}
LAYOUTS = {"rec36": (dict(ld=36, dir_off=9, conf_off=27), 0, "rec36-labels"),
           "rec40s": (dict(ld=40, dir_off=13, conf_off=31), 1, "rec40-labels"),
           "rec64": (dict(ld=64, dir_off=21, conf_off=50), 0, "rec40-labels")}
LABELS = {4: ((1, 2, 3, 4), 7), 254: ((1, 130, 253, 254), 255)}
RUNS = [("48x64", "rec36", 4), ("37x50", "rec36", 4), ("33x130", "rec36", 4), ("33x130", "rec36", 254),
        ("48x64", "rec40s", 4), ("37x50", "rec40s", 4), ("33x130", "rec40s", 4), ("37x50", "rec64", 254), ("33x130", "rec64", 254)]
NAN_AT = (0, 0, 4)        # (image, blob, keypoint) of the NaN estimate


@functools.lru_cache(maxsize=None)
def scene(shape, layout, slots, seed=0):
    """-> (field [2,h,w,ld], slot map [2,h,w], estimates fp32 [2,slots,KP,2], the four labels)"""
    h, w = SHAPES[shape]
    lay = LAYOUTS[layout][0]
    labels, above = LABELS[slots]
    rng = np.random.default_rng([seed, h, w, lay["ld"], slots])
    one = np.zeros((h, w), np.uint8)
    one[1:h // 2, 2:w // 3] = labels[0]
    one[h // 2:h, w // 4:w] = labels[1]                         # down to the last row, out to the last column, across every strip boundary
    one[0:h // 3, w // 2:w - 1] = labels[2]                     # rank one
    one[h // 3 + 1:h // 2 - 1, w // 2:w - 3] = above            # no row of the table: background
    one[0:5, w // 3 + 1:w // 2 - 1] = labels[3]
    sm = np.stack([one, one[:, ::-1]])
    yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    field = np.full((2, h, w, lay["ld"]), np.nan, np.float32)
    est = np.zeros((2, slots, KP, 2), np.float32)
    do, co = lay["dir_off"], lay["conf_off"]
    for bi in range(2):
        for k, lab in enumerate(labels):
            m = sm[bi] == lab
            ys, xs = yy[m], xx[m]
            ext = np.array([np.ptp(ys), np.ptp(xs)]) / 2 + 3.0
            kpt = np.array([ys.mean(), xs.mean()]) + rng.uniform(-1, 1, (KP, 2)) * ext * (0.3 + 0.4 * np.arange(KP)[:, None])
            v = kpt[None] - np.stack([ys, xs], -1)[:, None]
            ang = np.arctan2(v[..., 0], v[..., 1]) + rng.normal(0, 0.05, v.shape[:2])
            d = np.stack([np.sin(ang), np.cos(ang)], -1) * rng.uniform(0.5, 2.0, v.shape[:2])[..., None]
            d[rng.random(v.shape[:2]) < 0.02] = 0.0
            if k == 2:
                d[:] = (1.0, 0.0)
            field[bi][m, do:do + 2 * KP] = d.reshape(-1, 2 * KP)
            field[bi][m, co:co + KP] = rng.normal(0, 1.5, (int(m.sum()), KP))
            est[bi, lab - 1] = kpt + rng.normal(0, 0.3, (KP, 2))
    est[NAN_AT[0], labels[NAN_AT[1]] - 1, NAN_AT[2], 1] = np.nan
    return field, sm, est, labels


@functools.lru_cache(maxsize=None)
def reference(shape, layout, slots, cutoff):
    """((S32, A32), (S64, A64)) of slot_cov_reference.moments"""
    field, sm, est, _ = scene(shape, layout, slots)
    lay, sigmoid, _ = LAYOUTS[layout]
    return SC.moments(field, lay["dir_off"], lay["conf_off"], sigmoid, sm, slots, est, cutoff)


def usable(shape, layout, slots):
    """bool [2,slots,KP]: the entries whose sums are numbers (every entry but the NaN estimate's)"""
    _, _, est, _ = scene(shape, layout, slots)
    return np.isfinite(est).all(-1)


def covariance(lib, device, field, sm, est, lay, slots, sigmoid, cutoff):
    """One call of cp_ls_slot_covariance_f32 -> (sums, cov, stat, keypoints after the call) as NumPy arrays (outputs prefilled with 7)"""
    from casapose_amd import _lib

    b, h, w, ld = field.shape
    f = torch.from_numpy(field).to(device)
    keep, ptr = _labels_on_device(sm, device, False)
    kp = torch.from_numpy(est).to(device)
    ws = torch.full((b, slots, KP, 5), 7.0, dtype=torch.float64, device=device)
    cov = torch.full((b, slots, KP, 3), 7.0, dtype=torch.float32, device=device)
    stat = torch.full((b, slots, KP, 2), 7.0, dtype=torch.float32, device=device)
    assert lib.cp_ls_vote_workspace_bytes(b, slots, KP) == ws.numel() * 8
    _lib.check(lib.cp_ls_slot_covariance_f32(f.data_ptr(), ld, lay["dir_off"], lay["conf_off"], ptr, b, h, w, slots, KP, sigmoid, 0.0 if cutoff is None else cutoff,
                                             kp.data_ptr(), ws.data_ptr(), cov.data_ptr(), stat.data_ptr(), torch.cuda.current_stream(device).cuda_stream),
               "cp_ls_slot_covariance_f32")
    torch.cuda.synchronize(device)
    del keep
    return ws.cpu().numpy(), cov.cpu().numpy(), stat.cpu().numpy(), kp.cpu().numpy()


@pytest.fixture(scope="module")
def device_run(hip_lib, device):
    done = {}

    def run(shape, layout, slots, cutoff):
        key = (shape, layout, slots, cutoff)
        if key not in done:
            field, sm, est, _ = scene(shape, layout, slots)
            lay, sigmoid, _ = LAYOUTS[layout]
            done[key] = covariance(hip_lib, device, field, sm, est, lay, slots, sigmoid, cutoff)
        return done[key]
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("shape,layout,slots", RUNS)
def test_the_five_sums_match_the_fp64_reference(device_run, shape, layout, slots, cutoff):
    (s32, _), (ref, mag) = reference(shape, layout, slots, cutoff)
    ok = usable(shape, layout, slots)
    labels = scene(shape, layout, slots)[3]
    ws = device_run(shape, layout, slots, cutoff)[0]
    used = np.zeros(slots, bool)
    used[np.array(labels) - 1] = True
    assert not ws[:, ~used].any()                                        # a slot without pixels, and the label above `slots`: exactly 0
    assert np.isfinite(ws[ok]).all()                                     # no NaN of the background came through
    assert (mag[:, used][..., 4] > 0).all() and (cutoff is not None or (mag[:, used][..., 3] > 0)[ok[:, used]].all())    # Wall and Q are sums of something
    near = [labels[i] - 1 for i in (0, 1, 3)]                                                       # (a far keypoint can lose every pixel to the cut-off)
    assert (mag[:, near, :4, 3] > 0).all()
    den = np.where(mag > 0, mag, 1.0)
    gap = float((np.abs(s32 - ref) / den)[ok].max())
    gate = max(4 * gap, FWD_GATE[LAYOUTS[layout][2]])
    ratio = np.where(ok[..., None], np.abs(ws - ref) / den, 0.0)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s %s slots=%d cutoff=%s: |err| / sum|term| per entry (A00 A01 A11 Q Wall) %s; worst at (image, slot, keypoint, entry) %s; CPU gap %.3g, gate %.3g"
          % (shape, layout, slots, cutoff, " ".join("%.2e" % v for v in ratio.max((0, 1, 2))), at, gap, gate))
    assert ratio.max() <= gate, (shape, layout, slots, cutoff, float(ratio.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("shape,layout,slots", RUNS)
def test_the_finish_is_the_fp64_finish_of_the_device_sums_and_refuses_what_it_must(device_run, shape, layout, slots, cutoff):
    field, sm, est, labels = scene(shape, layout, slots)
    h = field.shape[1]
    ws, cov, stat, kp_after = device_run(shape, layout, slots, cutoff)
    assert np.array_equal(kp_after.view(np.uint32), est.view(np.uint32))                      # the keypoints are only read
    ref_cov, ref_stat, ok = SC.finish(ws, est, h)
    assert np.array_equal(np.isnan(cov).all(-1), ~ok) and np.isfinite(cov[ok]).all()         # three NaNs exactly where there is no covariance
    cond = np.where(ok, SC.condition(ws), 0.0)
    tol = 3 * 2.0 ** -24 * np.abs(ref_cov[ok]) + 1e-10 * cond[ok][:, None] * np.abs(ref_cov[ok]).max(-1, keepdims=True)
    err = np.abs(cov[ok] - ref_cov[ok])
    assert (err <= tol).all(), float((err / tol).max())
    assert np.abs(stat - ref_stat).max() <= 3 * 2.0 ** -24 * max(1.0, float(np.abs(ref_stat).max()))
    # the refusals of this scene: the rank-one blob, every slot without pixels, the NaN estimate
    used = np.zeros(slots, bool)
    used[np.array(labels) - 1] = True
    assert not ok[:, ~used].any() and not stat[:, ~used].any()
    assert not ok[:, labels[2] - 1].any() and (cutoff is not None or (stat[:, labels[2] - 1, :, 1] == 1.0).all())       # weight enough, and no covariance
    bi, k, j = NAN_AT
    assert not ok[bi, labels[k] - 1, j] and not stat[bi, labels[k] - 1, j].any()
    good = [labels[i] - 1 for i in (0, 1, 3)]
    n_ok = int(ok[:, good].sum())
    print("%s %s slots=%d cutoff=%s: %d of %d keypoints of the regular blobs have a covariance; sigma2 %.3g .. %.3g px^2, kept %.3g .. 1"
          % (shape, layout, slots, cutoff, n_ok, 2 * 3 * KP, stat[:, good][..., 0][ok[:, good]].min(), stat[:, good][..., 0].max(), stat[:, good][..., 1][ok[:, good]].min()))
    assert n_ok >= 2 * 3 * KP - 1 - 6                                   # all but the NaN one and at most a few ill-conditioned far keypoints
    assert (cov[ok][:, 0] > 0).all() and (cov[ok][:, 2] > 0).all() and (cov[ok][:, 0] * cov[ok][:, 2] > cov[ok][:, 1] ** 2).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rec36", "rec40s"])
def test_a_slot_that_keeps_too_little_weight_has_no_covariance(hip_lib, device, layout):
    """estimates 2.5 px off at a cut-off of 2 px: the slots keep less than 1/8 of their weight; without a cut-off they have a (large) covariance"""
    field, sm, est, labels = scene("48x64", layout, 4)
    lay, sigmoid, _ = LAYOUTS[layout]
    off = est.copy()
    off[..., 0] += 2.5
    off[..., 1] -= 2.5
    ws, cov, stat, _ = covariance(hip_lib, device, field, sm, off, lay, 4, sigmoid, 2.0)
    _, _, ok = SC.finish(ws, off, field.shape[1])
    regular = np.zeros(4, bool)
    regular[[labels[i] - 1 for i in (0, 1, 3)]] = True
    low = (stat[..., 1] < SC.MIN_KEPT) & (ws[..., 0] + ws[..., 2] > 0) & regular[None, :, None] & np.isfinite(off).all(-1)
    print("%s: %d keypoints kept less than 1/8 of their weight (smallest share %.3g)" % (layout, low.sum(), stat[..., 1][low].min()))
    assert low.sum() >= 5 and np.isnan(cov[low]).all() and np.array_equal(np.isnan(cov).all(-1), ~ok)
    _, cov0, stat0, _ = covariance(hip_lib, device, field, sm, off, lay, 4, sigmoid, None)
    assert np.isfinite(cov0[low]).all() and np.abs(stat0[..., 1][low] - 1.0).max() <= 1e-5          # |n| = 1 to fp32 rounding: W = Wall to that


@pytest.mark.gpu
def test_refusals(hip_lib, device):
    from casapose_amd import _lib

    f = torch.zeros(1, 16, 64, 36, device=device)
    sm = torch.zeros(1, 16, 64, dtype=torch.uint8, device=device)
    ws = torch.full((254 * 45,), 7.0, dtype=torch.float64, device=device)
    kp = torch.full((254 * 18 + 2,), 7.0, device=device)
    cov = torch.full((254 * 27,), 7.0, device=device)
    stat = torch.full((254 * 18,), 7.0, device=device)
    st = torch.cuda.current_stream(device).cuda_stream

    def call(ld=36, do=9, co=27, ptr=sm.data_ptr(), slots=8, k=9, cutoff=4.0, w=ws.data_ptr(), kps=kp.data_ptr(), c=cov.data_ptr(), s=stat.data_ptr()):
        return hip_lib.cp_ls_slot_covariance_f32(f.data_ptr(), ld, do, co, ptr, 1, 16, 64, slots, k, 0, cutoff, kps, w, c, s, st)

    for kw, words in ((dict(ptr=None), "slot map is required"), (dict(slots=0), "slots must be in 1..254"), (dict(slots=255), "slots must be in 1..254"),
                      (dict(k=8), "built for 9 keypoints"), (dict(do=19), "offsets outside"), (dict(co=28), "offsets outside"), (dict(ld=34), "multiple of 4"),
                      (dict(cutoff=-4.0), "cutoff_px must be finite and >= 0"), (dict(cutoff=float("nan")), "cutoff_px"), (dict(cutoff=float("inf")), "cutoff_px"),
                      (dict(w=None), "null pointer"), (dict(kps=None), "null pointer"), (dict(c=None), "cov and stat are required"),
                      (dict(s=None), "cov and stat are required"), (dict(kps=kp.data_ptr() + 4), "8-byte aligned")):
        with pytest.raises(_lib.CasaposeHipError, match="cp_ls_slot_covariance_f32: .*" + words):
            _lib.check(call(**kw), "cp_ls_slot_covariance_f32")
    torch.cuda.synchronize(device)
    assert bool((ws == 7.0).all()) and bool((cov == 7.0).all()) and bool((stat == 7.0).all())      # nothing was launched
    for cutoff in (0.0, 4.0):                                                                      # an all-background map: no sums, no covariance
        _lib.check(call(cutoff=cutoff), "cp_ls_slot_covariance_f32")
        torch.cuda.synchronize(device)
        assert not ws[:8 * 45].any() and bool(torch.isnan(cov[:8 * 27]).all()) and not stat[:8 * 18].any()
        assert bool((ws[8 * 45:] == 7.0).all()) and bool((cov[8 * 27:] == 7.0).all()) and bool((stat[8 * 18:] == 7.0).all()) and bool((kp == 7.0).all())


@pytest.mark.gpu
def test_the_op_is_the_entry_point(hip_lib, device):
    from casapose_amd import ops

    field, sm, est, _ = scene("37x50", "rec36", 4)
    lay, sigmoid, _ = LAYOUTS["rec36"]
    rec, m, kp = torch.from_numpy(field).to(device), torch.from_numpy(sm).to(device), torch.from_numpy(est).to(device)
    for cutoff in CUTOFFS:
        ws, cov, stat, _ = covariance(hip_lib, device, field, sm, est, lay, 4, sigmoid, cutoff)
        c, s, sums = ops.ls_slot_covariance(rec, 9, 27, 4, KP, m, kp, cutoff=cutoff, return_sums=True)
        assert c.dtype == torch.float32 and tuple(c.shape) == (2, 4, KP, 3) and tuple(s.shape) == (2, 4, KP, 2) and sums.dtype == torch.float64
        # the order of the atomics is free: the sums agree to the gate, cov and stat to the finish's tolerance
        fin = np.isfinite(cov)
        assert np.array_equal(np.isfinite(c.cpu().numpy()), fin)
        assert np.abs(c.cpu().numpy()[fin] - cov[fin]).max() <= 1e-5 * np.abs(cov[fin]).max()
        assert len(ops.ls_slot_covariance(rec, 9, 27, 4, KP, m, kp, cutoff=cutoff)) == 2
    with pytest.raises(ValueError, match="keypoints must be"):
        ops.ls_slot_covariance(rec, 9, 27, 4, KP, m, kp[:, :3])
