"""cp_ls_vote_slots_robust_f32 (csrc/ls_vote.hip, csrc/ls_robust_math.h) stage by stage against tests/robust_ls_reference.py, on the scenes of
tests/ls_reference.py cut into slots as tests/test_gpu_ls_slots.py cuts them (8, 32 and 254 slots; the five layouts of that file), and on the two
touching scenes of tests/test_gpu_vote_split_e2e.py (48 x 64 and 60 x 80, the slot map of the reference split, 32 slots).  Cut-off 4 px.

ONE PASS IN ISOLATION.  After a call with passes = 1 block 0 of the workspace holds the plain sums and block 1 the reweighted ones.  The estimate
the pass ran against is the plain solve of block 0, stored as ls_solve_kernel stores it (p rounded to fp32, times H in fp32): the test restates it
from the device's own block 0, and the passes = 0 test pins the device's plain keypoints to cp_ls_vote_slots_f32's.  The reference is given that
estimate and block 1 is compared with its fp64 sums on the measure |sum - ref| / sum |rho * term|.  The gate of a case is four times the largest
distance, on that measure and on the same (width, slots) runs, between the reference's two restatements (fp32 in the header's order against fp64
throughout), measured on the CPU -- but not less than FWD_GATE of the layout.  Four is that file's factor for another summation order and seed.
CPU_GAP holds the measured values, test_the_gaps_are_what_the_cpu_measures pins them, and the largest value seen on the MI355X stands beside.

KEYPOINTS are the solve of the device's own block 1 under the rule (solve_tolerance of tests/test_gpu_ls_stages.py) where
robust_ls_reference.accepted takes the system, and exactly the value of the pass before where it does not.

END TO END, InstanceLSVoting(split="votes", voter="robust") on touch2 / touch3.  Measured on the CPU (the fp64 chain of
robust_ls_reference.run after 2 passes against the planted values, worst instance; the plain voter's figures stand in test_gpu_vote_split_e2e.py):
    touch2: keypoints 0.0334 px (plain 1.16), rotation |dR| 0.00115 (0.0266), translation 0.215 mm (40.2)
    touch3: keypoints 0.0465 px (plain 1.84), rotation |dR| 0.00162 (0.0581), translation 0.218 mm (98.2)
The device stays within twice these, and its keypoints also below a quarter of the bound that file grants the plain voter."""
import functools

import numpy as np
import pytest
import torch

import ls_reference as L
import robust_ls_reference as RL
import test_gpu_vote_split_e2e as E
from test_gpu_ls_slots import CASES, RUNS, SLOTS, reference, slot_map_of, vote_slots
from test_gpu_ls_stages import FWD_GATE, _labels_on_device, solve_tolerance

KP = 9
CUTOFF = 4.0
TOUCH = {"touch2": 32, "touch3": 32}           # the touching scenes as runs of the stage tests: (case, width 0, slots)
ALL_RUNS = RUNS + [(name, 0, slots) for name, slots in TOUCH.items()]
# case: the largest |S(fp32 order) - S(fp64)| / sum |rho * term| on the CPU over the case's runs            largest device value seen on the MI355X
CPU_GAP = {
    "rec36": 7.85e-6,              # W = 136 at 32 and 254 slots (2.71e-6 at 8); gate 3.14e-5                       3.21e-6 (S00, W = 139, 8 slots)
    "rec36-misaligned": 7.85e-6,   # the same runs at W = 136; gate 3.14e-5                                         2.86e-6 (S11 at 8 slots)
    "rec40": 5.71e-6,              # W = 139 at 32 and 254 slots (1.16e-6 at 8); gate 2.28e-5                       5.71e-6 (S00, W = 139, 32 and 254 slots)
    "rec32": 3.89e-6,              # W = 136 at 32 and 254 slots (2.34e-6 at 8); gate 1.56e-5                       3.74e-6 (S00, W = 136, 32 and 254 slots)
    "rec36-sigmoid": 2.27e-6,      # W = 136 at 32 and 254 slots (1.07e-6 at 8); gate 9.08e-6                       2.25e-6 (S11, W = 136, 32 and 254 slots)
    "touch2": 3.42e-7,             # gate 4.16e-6, FWD_GATE of the production record                                3.16e-7 (T1)
    "touch3": 4.60e-7,             # gate 4.16e-6                                                                   4.52e-7 (T1)
}
# twice the reference chain's own error against the planted values (the docstring has them): keypoints px, |dR|, |dt| mm
BOUNDS = {"touch2": (2 * 0.0334, 2 * 0.00115, 2 * 0.215), "touch3": (2 * 0.0465, 2 * 0.00162, 2 * 0.218)}


def layout_of(case):
    """(layout dict, FWD_GATE key, sigmoid, misaligned slot map)"""
    if case in TOUCH:
        return L.LAYOUTS["rec36"], "rec36-labels", 0, False
    layout, gate, sigmoid, misalign = CASES[case]
    return L.LAYOUTS[layout], gate, sigmoid, misalign


def gate_of(case):
    return max(4 * CPU_GAP[case], FWD_GATE[layout_of(case)[1]])


@functools.lru_cache(maxsize=None)
def inputs(case, w, slots):
    """(field, slot map, sum |term| of the plain pass per entry)"""
    if case in TOUCH:
        rec = E.scene(case)[0]
        sm, _, _, mag, _, _ = E.reference_chain(case)
        return rec, sm, mag
    s, sm, _, mag = reference(case, w, slots)
    return s.field, sm, mag


def plain_estimate(block0, h):
    """the keypoints ls_solve_kernel makes of these sums"""
    return RL.device_rounding(L.solve(block0, h), h)


def one_pass_reference(case, w, slots, est):
    field, sm, _ = inputs(case, w, slots)
    lay, _, sigmoid, _ = layout_of(case)
    return RL.one_pass(field, lay["ld"], lay["dir_off"], lay["conf_off"], sigmoid, sm, slots, est, CUTOFF)


@functools.lru_cache(maxsize=None)
def cpu_gap(case, w, slots):
    """the two restatements against each other, given the fp32-order plain estimate"""
    field, sm, _ = inputs(case, w, slots)
    lay, _, sigmoid, _ = layout_of(case)
    plain = L.sums(L.terms(field, lay["ld"], lay["dir_off"], lay["conf_off"], sigmoid, field.shape[1])[0], sm, slots)[0]
    (s32, _), (s64, a64) = one_pass_reference(case, w, slots, plain_estimate(plain, field.shape[1]))
    return float((np.abs(s32 - s64) / np.where(a64 > 0, a64, 1.0)).max())


def test_the_gaps_are_what_the_cpu_measures():
    for case in CPU_GAP:
        got = max(cpu_gap(c, w, s) for c, w, s in ALL_RUNS if c == case)
        print("%s: fp32 order against fp64, |difference| / sum|rho * term| %.3g (CPU_GAP %.3g, gate %.3g)" % (case, got, CPU_GAP[case], gate_of(case)))
        assert 0.98 * CPU_GAP[case] <= got <= 1.02 * CPU_GAP[case]       # the figures as written: three digits


def vote_robust(lib, device, field, slot_map, lay, slots, sigmoid, misalign, passes, cutoff=CUTOFF):
    """One call of cp_ls_vote_slots_robust_f32; (workspace [2,b,slots,KP,5], keypoints) as NumPy arrays (prefilled with 7: the call owns both)."""
    from casapose_amd import _lib

    b, h, w, ld = field.shape
    f = torch.from_numpy(field).to(device)
    keep, ptr = _labels_on_device(slot_map, device, misalign)
    ws = torch.full((2, b, slots, KP, 5), 7.0, dtype=torch.float64, device=device)
    kp = torch.full((b, slots, KP, 2), 7.0, dtype=torch.float32, device=device)
    assert lib.cp_ls_vote_robust_workspace_bytes(b, slots, KP) == ws.numel() * 8
    _lib.check(lib.cp_ls_vote_slots_robust_f32(f.data_ptr(), ld, lay["dir_off"], lay["conf_off"], ptr, b, h, w, slots, KP, sigmoid, cutoff, passes,
                                               ws.data_ptr(), kp.data_ptr(), torch.cuda.current_stream(device).cuda_stream), "cp_ls_vote_slots_robust_f32")
    torch.cuda.synchronize(device)
    del keep
    return ws.cpu().numpy(), kp.cpu().numpy()


@pytest.fixture(scope="module")
def robust_run(hip_lib, device):
    done = {}

    def run(case, w, slots, passes):
        if (case, w, slots, passes) not in done:
            field, sm, _ = inputs(case, w, slots)
            lay, _, sigmoid, misalign = layout_of(case)
            done[case, w, slots, passes] = vote_robust(hip_lib, device, field, sm, lay, slots, sigmoid, misalign, passes)
        return done[case, w, slots, passes]
    return run


@pytest.fixture(scope="module")
def plain_run(hip_lib, device):
    done = {}

    def run(case, w, slots):
        if (case, w, slots) not in done:
            field, sm, _ = inputs(case, w, slots)
            lay, _, sigmoid, misalign = layout_of(case)
            done[case, w, slots] = vote_slots(hip_lib, device, field, sm, lay, slots, sigmoid, misalign)
        return done[case, w, slots]
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("case,w,slots", ALL_RUNS)
def test_one_pass_matches_the_fp64_sums(robust_run, case, w, slots):
    field, sm, mag = inputs(case, w, slots)
    h = field.shape[1]
    ws, kp = robust_run(case, w, slots, 1)
    present = mag > 0
    empty = ~present.any((0, 2, 3))
    if case not in TOUCH:
        assert present[:, slots - 1].all() and empty.sum() >= slots - 5 * SLOTS[slots]      # the last row is used, and there are empty slots
    assert not ws[:, :, empty].any() and not kp[:, empty].any()                            # a slot without pixels: exactly 0 in both blocks
    assert np.isfinite(ws).all() and np.isfinite(kp).all()                                 # no NaN of the logits or the background came through
    _, (ref, rmag) = one_pass_reference(case, w, slots, plain_estimate(ws[0], h))
    assert (rmag > 0).any((2, 3))[:, ~empty].all()                                          # every slot with pixels keeps some weight here
    ratio = np.abs(ws[1] - ref) / np.where(rmag > 0, rmag, 1.0)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s w=%d slots=%d: block 1, |err| / sum|rho * term| per entry (S00 S01 S11 T0 T1) %s; worst at (image, slot, keypoint, entry) %s; CPU gap %.3g, gate %.3g"
          % (case, w, slots, " ".join("%.2e" % v for v in ratio.max((0, 1, 2))), at, cpu_gap(case, w, slots), gate_of(case)))
    assert ratio.max() <= gate_of(case), (case, w, slots, float(ratio.max()))


def check_the_rule(what, ws, kp, before, present, h):
    """kp are the solve of block 1 where the rule takes it and `before` exactly where it does not -> (taken, refused with pixels, of those for weight)"""
    took = RL.accepted(ws[1], ws[0])
    assert not took[~present].any()
    ref, cond = L.solve(np.where(took[..., None], ws[1], 0.0), h), np.where(took, L.condition(ws[1]), 0.0)
    err, tol = np.abs(kp - ref), solve_tolerance(ref, cond, h)
    assert (err <= tol)[took].all(), (what, float((err / np.where(tol > 0, tol, 1.0))[took].max()))
    assert np.array_equal(kp[~took], before[~took]), what
    refused = present[..., None] & ~took
    low = refused & (RL.kept(ws[1], ws[0]) < RL.MIN_KEPT)
    print("%s: %d of %d systems taken, %d refused (%d of them for a weight below 1/8), largest move %.3g px"
          % (what, took.sum(), present.sum() * KP, refused.sum(), low.sum(), np.abs(kp - before).max()))
    return int(took.sum()), int(refused.sum()), int(low.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("case,w,slots", ALL_RUNS)
def test_keypoints_follow_the_solve_rule(robust_run, case, w, slots, passes):
    """the keypoints of pass k are the solve of the device's own block 1 where the rule takes it, the keypoints of pass k - 1 (the call with one
    pass less: the same kernels on the same input) where it does not.  At 4 px every system with pixels is taken on these scenes (the smallest
    share of the plain weight a pass keeps is 0.175); test_the_rule_falls_back_on_the_device has the other branch."""
    field, _, mag = inputs(case, w, slots)
    ws, kp = robust_run(case, w, slots, passes)
    _, before = robust_run(case, w, slots, passes - 1)
    taken, _, _ = check_the_rule("%s w=%d slots=%d passes=%d" % (case, w, slots, passes), ws, kp, before, mag.any((2, 3)), field.shape[1])
    assert taken > 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rec36", "rec40"])
def test_the_rule_falls_back_on_the_device(hip_lib, device, layout):
    """the two refusals on both kernels: a slot whose directions are all (1, 0) (rank one) keeps its plain value at 4 px, and at a cut-off of
    0.3 px the systems that keep less than 1/8 of their weight keep the value of the pass before, in pass 1 and again in pass 2"""
    lay = L.LAYOUTS[layout]
    s = L.scene(136, rank_one=True, **lay)
    sm = slot_map_of(s.labels, 8)
    present = np.stack([(sm[b][..., None] == np.arange(1, 9)).any((0, 1)) for b in range(s.b)])
    runs = [vote_robust(hip_lib, device, s.field, sm, lay, 8, 0, False, passes) for passes in (0, 1, 2)]
    (o,) = np.unique(sm[s.labels == L.RANK_ONE]) - 1
    for passes in (1, 2):
        _, refused, low = check_the_rule("%s rank one, passes=%d" % (layout, passes), runs[passes][0], runs[passes][1], runs[passes - 1][1], present, s.h)
        assert refused >= s.b * KP                  # the rank-one slot's keypoints in every image (some of them have also lost their weight)
        assert np.array_equal(runs[passes][1][:, o], runs[0][1][:, o]) and np.abs(runs[0][1][:, o]).max() > 0
    s = L.scene(139, **lay)
    sm = slot_map_of(s.labels, 32)
    present = np.stack([(sm[b][..., None] == np.arange(1, 33)).any((0, 1)) for b in range(s.b)])
    runs = [vote_robust(hip_lib, device, s.field, sm, lay, 32, 0, False, passes, cutoff=0.3) for passes in (0, 1, 2)]
    for passes in (1, 2):
        taken, _, low = check_the_rule("%s cut-off 0.3 px, passes=%d" % (layout, passes), runs[passes][0], runs[passes][1], runs[passes - 1][1], present, s.h)
        assert taken >= 10 and low >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("case,w,slots", ALL_RUNS)
def test_no_pass_is_the_plain_voter_and_block_0_stays_its_sums(robust_run, plain_run, case, w, slots):
    _, _, mag = inputs(case, w, slots)
    old_sums, old_kp = plain_run(case, w, slots)
    ws, kp = robust_run(case, w, slots, 0)
    assert torch.equal(torch.from_numpy(kp), torch.from_numpy(old_kp))
    assert (ws[1] == 7.0).all()                                          # no reweighted pass: block 1 is not written
    gate = 2 * FWD_GATE[layout_of(case)[1]]                               # the order of the atomics is free
    for passes in (0, 1, 2):
        block0 = robust_run(case, w, slots, passes)[0][0]
        ratio = np.abs(block0 - old_sums) / np.where(mag > 0, mag, 1.0)
        assert ratio.max() <= gate, (case, w, slots, passes, float(ratio.max()))
        assert not block0[mag == 0].any()


@pytest.mark.gpu
def test_refusals(hip_lib, device):
    from casapose_amd import _lib

    f = torch.zeros(1, 16, 64, 36, device=device)
    sm = torch.zeros(1, 16, 64, dtype=torch.uint8, device=device)
    ws = torch.full((2 * 254 * 45,), 7.0, dtype=torch.float64, device=device)
    kp = torch.full((254 * 18,), 7.0, device=device)
    st = torch.cuda.current_stream(device).cuda_stream

    def call(ld=36, do=9, co=27, ptr=sm.data_ptr(), slots=8, k=9, cutoff=4.0, passes=2, w=ws.data_ptr()):
        return hip_lib.cp_ls_vote_slots_robust_f32(f.data_ptr(), ld, do, co, ptr, 1, 16, 64, slots, k, 0, cutoff, passes, w, kp.data_ptr(), st)

    for kw, words in ((dict(ptr=None), "slot map is required"), (dict(slots=0), "slots must be in 1..254"), (dict(slots=255), "slots must be in 1..254"),
                      (dict(k=8), "built for 9 keypoints"), (dict(do=19), "offsets outside"), (dict(co=28), "offsets outside"), (dict(ld=34), "multiple of 4"),
                      (dict(cutoff=0.0), "cutoff_px must be finite and > 0"), (dict(cutoff=-4.0), "cutoff_px"), (dict(cutoff=float("nan")), "cutoff_px"),
                      (dict(cutoff=float("inf")), "cutoff_px"), (dict(passes=-1), r"passes must be in 0\.\.8"), (dict(passes=9), r"passes must be in 0\.\.8"),
                      (dict(w=None), "null pointer")):
        with pytest.raises(_lib.CasaposeHipError, match="cp_ls_vote_slots_robust_f32: .*" + words):
            _lib.check(call(**kw), "cp_ls_vote_slots_robust_f32")
    torch.cuda.synchronize(device)
    assert bool((ws == 7.0).all()) and bool((kp == 7.0).all())         # nothing was launched
    _lib.check(call(passes=8), "cp_ls_vote_slots_robust_f32")          # an all-background map: every sum and keypoint 0
    torch.cuda.synchronize(device)
    w2 = ws.view(2, 254 * 45)
    assert not w2.view(-1)[:2 * 8 * 45].any() and not kp[:8 * 18].any()
    assert bool((w2.view(-1)[2 * 8 * 45:] == 7.0).all())               # and nothing past the two blocks of 8 slots


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def robust_chain(name):
    """the CPU chain of the docstring: reference split, two reweighted passes in fp64 -> keypoints [1, OBJECTS, R, KP, 2]"""
    rec = E.scene(name)[0]
    slots = E.reference_chain(name)[0]
    return RL.run(rec, 36, 9, 27, 0, slots, E.OBJECTS * E.R, CUTOFF, 2, "fp64").kps[2].reshape(1, E.OBJECTS, E.R, KP, 2)


@pytest.mark.parametrize("name", E.NAMES)
def test_the_robust_reference_chain_on_the_cpu(name):
    """what BOUNDS are made of"""
    from casapose_amd.pose_estimation import pnp as P

    _, _, _, X, cam, planted = E.scene(name)
    ranks = E.reference_chain(name)[5]
    kps = robust_chain(name)
    e_kp = e_r = e_t = 0.0
    for i, (pose, yx) in enumerate(planted):
        e_kp = max(e_kp, float(np.abs(kps[0, 0, ranks[i]] - yx).max()))
        p6 = P.pnp_rvec_t(X[0], kps[0, 0, ranks[i]][:, ::-1], cam, rng=np.random.default_rng(0))
        dr, dt = E.pose_errors(np.concatenate([P.rodrigues(p6[:3]), p6[3:, None]], axis=1), pose)
        e_r, e_t = max(e_r, dr), max(e_t, dt)
    print("%s: robust reference chain against the planted values: keypoints %.3g px, |dR| %.3g, |dt| %.3g mm" % (name, e_kp, e_r, e_t))
    bk, br, bt = BOUNDS[name]
    assert e_kp <= bk / 2 * 1.005 and e_r <= br / 2 * 1.005 and e_t <= bt / 2 * 1.005      # the figures above, as printed: three digits


@pytest.fixture(scope="module")
def voted(device):
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    def run(name):
        out = torch.from_numpy(E.scene(name)[0]).to(device)
        seg, dirs, conf = torch.split(out, [9, 18, 9], dim=3)
        P = E.PARAMS
        voter = InstanceLSVoting("instances", num_classes=E.OBJECTS + 1, num_points=KP, max_instances=E.R, min_component=P["min_size"], split="votes",
                                 cell=P["cell"], vote_stride=E.STRIDE, min_votes=P["min_votes"], rel_percent=P["rel_percent"], nms_radius=P["nms_radius"],
                                 gate=P["gate"], voter="robust", cutoff=CUTOFF, passes=2)
        return voter, voter([seg, dirs, conf])
    return functools.lru_cache(maxsize=None)(run)


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.NAMES)
def test_touching_instances_end_to_end_keypoints(voted, name):
    voter, coords = voted(name)
    slots, inst, _, _, _, ranks = E.reference_chain(name)
    planted = E.scene(name)[5]
    assert tuple(coords.shape) == (1, E.OBJECTS, E.R, KP, 2) and coords.dtype == torch.float32
    assert np.array_equal(voter.last_labels.cpu().numpy(), slots) and np.array_equal(voter.last_counts.cpu().numpy(), inst[..., 0])
    got = coords.cpu().numpy().astype(np.float64)
    on = inst[..., 0] > 0
    assert not got[~on].any()
    err = max(float(np.abs(got[0, 0, ranks[i]] - yx).max()) for i, (_, yx) in enumerate(planted))
    print("%s: device keypoints against the planted ones: %.3g px (bound %.3g; the plain voter's bound %.3g)" % (name, err, BOUNDS[name][0], E.BOUNDS[name][0]))
    assert err <= BOUNDS[name][0] and err < E.BOUNDS[name][0] / 4
    kept = voter.last_kept
    assert kept.dtype == torch.float32 and tuple(kept.shape) == (1, E.OBJECTS, E.R, KP) and kept.is_cuda
    kept = kept.cpu().numpy()
    assert not kept[~on].any() and (kept[on] > 0.9).all() and (kept[on] < 1.0).any() and (kept <= 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.NAMES)
@pytest.mark.parametrize("path", ["host", "device"])
def test_touching_instances_end_to_end_poses(voted, device, name, path):
    from casapose_amd.pose_estimation.device_pnp import DevicePnP
    from casapose_amd.pose_estimation.instance_voting import poses_pnp_instances

    voter, coords = voted(name)
    _, _, _, X, cam, planted = E.scene(name)
    ranks = E.reference_chain(name)[5]
    solver = DevicePnP(device, KP) if path == "device" else None
    got = poses_pnp_instances(coords, voter.last_counts, X[None, :, None], cam, rng=np.random.default_rng(0), solver=solver)
    on = voter.last_counts.cpu().numpy() > 0
    assert on.sum() == len(planted) and not got[~on].any()
    worst_r = worst_t = 0.0
    for i, (pose, _) in enumerate(planted):
        dr, dt = E.pose_errors(got[0, 0, ranks[i]].astype(np.float64), pose)
        worst_r, worst_t = max(worst_r, dr), max(worst_t, dt)
    print("%s (%s PnP): |dR| %.3g (bound %.3g), |dt| %.3g mm (bound %.3g)" % (name, path, worst_r, BOUNDS[name][1], worst_t, BOUNDS[name][2]))
    assert worst_r <= BOUNDS[name][1] and worst_t <= BOUNDS[name][2]
