"""cp_ls_vote_slots_f32 (csrc/ls_vote.hip): the LS voter keyed by the slots of a slot map.  On the scenes of tests/ls_reference.py every object's
pixels are cut into R parts, the parts become slots, and the caller-owned sums are compared with the fp64 restatement summed per slot; the
keypoints with the restatement's solve of the device's own sums; the whole with the existing voter where both can be asked the same question.

The per-pixel arithmetic is the existing voter's and only the table row differs, so the gate of every case is FWD_GATE of
tests/test_gpu_ls_stages.py for the same layout, imported, on that file's measure |sum - ref| / sum |term|.  The largest value seen on an MI355X
stands beside each case.  At 8 slots the pixel sets are the whole objects: the values are those of the stage tests to the digit, and the sums
equal the existing voter's to 3e-16 of sum |term| (rec40: bit for bit).

How finely the objects are cut is this file's choice, and the measure depends on it.  FWD_GATE is four times the largest value seen on WHOLE
objects (the smallest has 180 pixels), and |sum - ref| / sum |term| is not free of the set's size: a term r00 = (1 - ny * ny) * w carries the
rounding of ny * ny near 1, about 6e-8 * w whatever is left after the subtraction, so a pixel whose direction is nearly parallel to an axis
adds its full error to the numerator and almost nothing to the denominator (ls_add_terms in csrc/ls_vote.hip; the stage tests name the same
entry, S00 of a keypoint with nearly parallel directions, as their worst).  A whole object mixes such pixels with well-conditioned ones; the
smaller the set, the more of the (set, keypoint) pairs consist of them alone, and the maximum is taken over more pairs.  The growth is therefore
faster than the 1 / sqrt(N) of independent errors -- measured on rec40: 3.44e-7 whole, 9.21e-7 halves, 2.12e-6 quarters, about 2.5 x per
halving -- and no cut finer than the whole object has a gate that follows from FWD_GATE by reasoning alone.  This file therefore takes the
coarsest cut that still gives an object more than one slot: two parts at any slot count, placed in the first and the last of its R slots.
That it stays under the imported gates is a measurement (the values beside the cases), not a derivation.  Quarters were measured once (R = 4,
sets of 45 - 65 pixels): rec36 3.76e-6 (gate 4.16e-6), rec40 2.12e-6 (1.38e-6), rec32 2.36e-6 (1.54e-6), rec36-sigmoid 7.11e-7 (5.36e-7) --
the kernel that agrees with the existing voter to 3e-16 on whole objects, measured on sets a quarter of the size of those the gate was taken
from."""
import functools

import numpy as np
import pytest
import torch

import ls_reference as L
from test_gpu_ls_stages import FWD_GATE, _labels_on_device, solve_tolerance, vote

pytestmark = pytest.mark.gpu

KP = 9
# (slots, R): object o has the slots (o - 1) * R + 1 .. (o - 1) * R + R; its two parts (one at R = 1) go to the first and the last of them, and
# the last part of object 5 is moved to the LAST slot, so the table's last row is used
SLOTS = {8: 1, 32: 4, 254: 2}
# id: (layout, gate of test_gpu_ls_stages, sigmoid weights, slot map one byte off alignment)        largest |err| / sum|term| seen on the MI355X
CASES = {
    "rec36": ("rec36", "rec36-labels", 0, False),                          # 1.29e-6 (S00 at both widths, 32 and 254 slots; 1.04e-6 at 8)
    "rec36-misaligned": ("rec36", "rec36-labels-misaligned", 0, True),     # 1.29e-6 (S00, 32 and 254 slots; 1.04e-6 at 8)
    "rec40": ("rec40", "rec40-labels", 0, False),                          # 9.21e-7 (S00 at W = 136, 32 and 254 slots; 3.44e-7 at 8)
    "rec32": ("rec32", "rec32-labels", 0, False),                          # 1.13e-6 (S00 at W = 136, 32 and 254 slots; 3.85e-7 at 8)
    "rec36-sigmoid": ("rec36", "rec36-sigmoid", 1, False),                 # 3.10e-7 (S00 at W = 139, 32 and 254 slots; 1.34e-7 at 8)
}
RUNS = [(c, w, s) for c in CASES for w in L.WIDTHS for s in SLOTS if not (CASES[c][3] and w % 4)]


def slot_map_of(labels, slots):
    """the label map (labels 1..5) cut into slots: up to two parts per object, blocks of 2 rows x 3 columns taken in turn"""
    r = SLOTS[slots]
    b, h, w = labels.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    part = ((yy // 2 + xx // 3) % min(r, 2) * (r - 1))[None]      # 0, or the object's last slot
    lab = labels.astype(np.int64)
    out = np.where(lab > 0, (lab - 1) * r + part + 1, 0)
    out[(lab == 5) & (part == r - 1)] = slots
    assert out.max() == slots
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(case, w, slots):
    layout, _, sigmoid, _ = CASES[case]
    s, t32 = _scene_terms(layout, w, sigmoid)
    sm = slot_map_of(s.labels, slots)
    ref, mag = L.sums(t32, sm, slots)
    return s, sm, ref, mag


@functools.lru_cache(maxsize=None)
def _scene_terms(layout, w, sigmoid):
    s = L.scene(w, **L.LAYOUTS[layout])         # no arg-max: the logits are NaN, and nothing may read them
    t32, _ = L.terms(s.field, s.ld, s.dir_off, s.conf_off, sigmoid, s.h)
    return s, t32


def vote_slots(lib, device, field, slot_map, lay, slots, sigmoid=0, misalign=False):
    """One call of cp_ls_vote_slots_f32; (sums_ws, keypoints) as NumPy arrays (prefilled with 7: the call owns both)."""
    from casapose_amd import _lib

    b, h, w, ld = field.shape
    f = torch.from_numpy(field).to(device)
    keep, ptr = _labels_on_device(slot_map, device, misalign)
    sums = torch.full((b, slots, KP, 5), 7.0, dtype=torch.float64, device=device)
    kp = torch.full((b, slots, KP, 2), 7.0, dtype=torch.float32, device=device)
    assert lib.cp_ls_vote_workspace_bytes(b, slots, KP) == sums.numel() * 8
    _lib.check(lib.cp_ls_vote_slots_f32(f.data_ptr(), ld, lay["dir_off"], lay["conf_off"], ptr, b, h, w, slots, KP, sigmoid, sums.data_ptr(), kp.data_ptr(),
                                        torch.cuda.current_stream(device).cuda_stream), "cp_ls_vote_slots_f32")
    torch.cuda.synchronize(device)
    del keep
    return sums.cpu().numpy(), kp.cpu().numpy()


@pytest.fixture(scope="module")
def slots_run(hip_lib, device):
    done = {}

    def run(case, w, slots):
        if (case, w, slots) not in done:
            layout, _, sigmoid, misalign = CASES[case]
            s, sm, _, _ = reference(case, w, slots)
            done[case, w, slots] = vote_slots(hip_lib, device, s.field, sm, L.LAYOUTS[layout], slots, sigmoid, misalign)
        return done[case, w, slots]
    return run


@pytest.mark.parametrize("case,w,slots", RUNS)
def test_sums_match_the_fp32_order_terms_per_slot(slots_run, case, w, slots):
    s, sm, ref, mag = reference(case, w, slots)
    got, kp = slots_run(case, w, slots)
    present = mag > 0
    empty = ~present.any((0, 2, 3))
    assert present[:, slots - 1].all() and empty.sum() >= slots - 5 * SLOTS[slots]          # the last row is used, and there are empty slots
    assert not got[:, empty].any() and not kp[:, empty].any()                              # a slot without pixels: exactly 0, like an absent object
    assert np.isfinite(got).all() and np.isfinite(kp).all()                                # no NaN of the logits or the background came through
    ratio = np.abs(got - ref) / np.where(present, mag, 1.0)
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s w=%d slots=%d: |err| / sum|term| per entry (S00 S01 S11 T0 T1) %s; worst at (image, slot, keypoint, entry) %s, %d pixels, condition number %.0f"
          % (case, w, slots, " ".join("%.2e" % v for v in ratio.max((0, 1, 2))), at, int((sm[at[0]] == at[1] + 1).sum()), L.condition(ref)[at[:3]]))
    assert ratio.max() <= FWD_GATE[CASES[case][1]], (case, w, slots, float(ratio.max()))


@pytest.mark.parametrize("case,w,slots", RUNS)
def test_keypoints_are_the_solve_of_the_device_sums(slots_run, case, w, slots):
    s, _, _, mag = reference(case, w, slots)
    sums, kp = slots_run(case, w, slots)
    ref, cond = L.solve(sums, s.h), L.condition(sums)
    present = mag.any((2, 3))
    assert np.isfinite(cond[present]).all() and not ref[~present].any()
    cond = np.where(present[..., None], cond, 0.0)
    err, tol = np.abs(kp - ref), solve_tolerance(ref, cond, s.h)
    assert (err <= tol).all(), (case, w, slots, float((err / np.where(tol > 0, tol, 1.0)).max()))


@pytest.mark.parametrize("case,w", [(c, w) for c, w, s in RUNS if s == 8 and L.LAYOUTS[CASES[c][0]]["objects"] == 8])
def test_eight_slots_agree_with_the_existing_voter(hip_lib, device, slots_run, case, w):
    """slots = 8 and the slot map given to cp_ls_vote_w_f32 as its label map: the same pixels into the same rows.  The order of the fp64 atomics
    is free in both, so the sums agree within twice the gate, not byte for byte."""
    layout, gate, sigmoid, misalign = CASES[case]
    s, sm, _, mag = reference(case, w, 8)
    got, kp = slots_run(case, w, 8)
    old_sums, old_kp = vote(hip_lib, device, s.field, sm, L.LAYOUTS[layout], sigmoid, misalign)
    old_sums, old_kp = old_sums.cpu().numpy(), old_kp.cpu().numpy()
    ratio = np.abs(got - old_sums) / np.where(mag > 0, mag, 1.0)
    print("%s w=%d: new against existing voter, |difference| / sum|term| %.2e" % (case, w, ratio.max()))
    assert ratio.max() <= 2 * FWD_GATE[gate]
    empty = ~(mag > 0).any((0, 2, 3))
    assert empty.sum() == 3 and np.array_equal(got[:, empty], old_sums[:, empty]) and np.array_equal(kp[:, empty], old_kp[:, empty])


def test_refusals(hip_lib, device):
    from casapose_amd import _lib

    f = torch.zeros(1, 16, 64, 36, device=device)
    sm = torch.zeros(1, 16, 64, dtype=torch.uint8, device=device)
    sums = torch.full((254 * 45,), 7.0, dtype=torch.float64, device=device)
    kp = torch.full((254 * 18,), 7.0, device=device)
    st = torch.cuda.current_stream(device).cuda_stream

    def call(ld=36, do=9, co=27, ptr=sm.data_ptr(), slots=8, k=9):
        return hip_lib.cp_ls_vote_slots_f32(f.data_ptr(), ld, do, co, ptr, 1, 16, 64, slots, k, 0, sums.data_ptr(), kp.data_ptr(), st)

    for kw, words in ((dict(ptr=None), "slot map is required"), (dict(slots=0), "slots must be in 1..254"), (dict(slots=255), "slots must be in 1..254"),
                      (dict(k=8), "built for 9 keypoints"), (dict(do=19), "offsets outside"), (dict(co=28), "offsets outside"), (dict(ld=34), "multiple of 4")):
        with pytest.raises(_lib.CasaposeHipError, match="cp_ls_vote_slots_f32: .*" + words):
            _lib.check(call(**kw), "cp_ls_vote_slots_f32")
    torch.cuda.synchronize(device)
    assert bool((sums == 7.0).all()) and bool((kp == 7.0).all())      # nothing was launched
    _lib.check(call(), "cp_ls_vote_slots_f32")                         # an all-background map: every sum and keypoint 0
    torch.cuda.synchronize(device)
    assert not sums[:8 * 45].any() and not kp[:8 * 18].any()
