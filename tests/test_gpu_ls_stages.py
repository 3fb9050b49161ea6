"""The LS voter (csrc/ls_vote.hip) checked stage by stage: the C ABI is called directly, the caller-owned buffers (sums_ws, keypoints, pu_ws,
dfield) are read back and compared with the fp64 restatement of tests/ls_reference.py -- the sums of all accumulate dispatches, the solve, the
backward's (p, u) table, both per-pixel backward kernels in overwrite and accumulate mode with and without the regulariser, the grid-stride wrap,
and the statistics and reprojection-loss kernels past their stride loops.  tests/test_ls_reference.py pins the restatement and the scenes.

The measured gates are four times the largest value seen on an MI355X against the fp64 reference (the margin covers the order of the fp64
atomics and the last bits of the hardware exp / log / rsqrt units); the value seen stands beside each.  The others are derived where they stand."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ls_reference as L

pytestmark = pytest.mark.gpu

KP = 9
# ---- measured gates: 4 x the value beside each -----------------------------------------------------------------------------------------------
FWD_GATE = {                          # |sum - ref| / sum |term| per entry, ref = fp64 sums of the fp32-order terms; the measurement's ceiling is 2e-6
    "rec36-argmax": 4 * 1.04e-6,             # S00 at W = 136 (4.82e-7 at W = 139); S01 2.8e-7, S11 5.7e-7, T0 2.9e-7, T1 5.1e-7
    "rec36-labels": 4 * 1.04e-6,             # the same sums as the arg-max dispatch, entry for entry
    "rec36-labels-misaligned": 4 * 1.04e-6,
    "rec40-argmax": 4 * 3.44e-7,             # S00 at W = 136 (1.63e-7 at W = 139)
    "rec40-labels": 4 * 3.44e-7,
    "rec32-labels": 4 * 3.85e-7,             # S00 at W = 136 (1.90e-7 at W = 139)
    "rec36-sigmoid": 4 * 1.34e-7,            # S00 at W = 139 (1.18e-7 at W = 136)
}
# The largest ratio (1.04e-6) is S00 of the 180-pixel object 3, keypoint 5, image 1 at W = 136, whose directions are nearly parallel (condition
# number 31): there 1 - n^2 cancels, the term keeps the ~1e-7 absolute rounding of n^2 while sum |term| shrinks with the cancellation.  The
# arithmetic accounts for it: ls_accumulate36_kernel's n = d * rsqrt(d . d), restated in NumPy fp32 with a correctly rounded rsqrt and softplus, is
# 7.5e-7 from the reference's division at that same entry, and the fp32-order reference itself 4.3e-7 from the fp64 terms on this measure.  The
# generic kernel divides like the reference; its 1 - n * n and r00 * cy + r01 * cx are contracted into fused multiply-adds.
BWD_GATE = {"bwd36": 4 * 7.52e-6, "generic40": 4 * 9.92e-6, "generic36": 4 * 7.52e-6}     # against the closed form on the device's own table; ceiling 2e-5
E2E_GATE = 4 * 6.32e-6                # forward + backward against the fp64 chain (autograd's, by test_ls_reference); ceiling 1e-4
WRAP_GATE = {"bwd36": 4 * 1.80e-6, "generic36": 4 * 1.86e-6}
CONF_SUM_GATE = 4 * 1.62e-9           # conf_sums, relative to the sum (all terms positive)
REPROJ_VALUE_GATE = 4 * 1.54e-9       # ceiling 1e-5 for both
REPROJ_GRAD_GATE = 4 * 1.91e-7        # per point, relative to the point's larger component


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _labels_on_device(labels, device, misalign=False):
    """(tensor that owns the bytes, pointer): the map itself, or a copy that starts one byte past a 4-byte boundary."""
    flat = torch.from_numpy(np.ascontiguousarray(labels).reshape(-1)).to(device)
    if not misalign:
        assert flat.data_ptr() % 4 == 0
        return flat, flat.data_ptr()
    buf = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device=device)
    buf[1:1 + flat.numel()] = flat
    assert buf.data_ptr() % 4 == 0
    return buf, buf.data_ptr() + 1


def vote(lib, device, field, labels, lay, sigmoid=0, misalign=False):
    """One call of cp_ls_vote_w_f32; (sums_ws, keypoints) as device tensors (prefilled with 7: the call owns both)."""
    from casapose_amd import _lib

    b, h, w, ld = field.shape
    f = field if isinstance(field, torch.Tensor) else torch.from_numpy(field).to(device)
    keep, lab_ptr = _labels_on_device(labels, device, misalign) if labels is not None else (None, None)
    sums = torch.full((b, lay["objects"], KP, 5), 7.0, dtype=torch.float64, device=device)
    kp = torch.full((b, lay["objects"], KP, 2), 7.0, dtype=torch.float32, device=device)
    _lib.check(lib.cp_ls_vote_w_f32(f.data_ptr(), ld, lay["seg_off"], lay["dir_off"], lay["conf_off"], lab_ptr, b, h, w, lay["objects"], KP, sigmoid,
                                    sums.data_ptr(), kp.data_ptr(), _stream(device)), "cp_ls_vote_w_f32")
    torch.cuda.synchronize(device)
    del keep
    return sums, kp


# ---- forward sums and solve ---------------------------------------------------------------------------------------------------------------------
FORWARD = {   # id: (layout, arg-max dispatch, sigmoid weights, labels one byte off alignment)
    "rec36-argmax": ("rec36", True, 0, False),             # ls_accumulate36_kernel<false>
    "rec36-labels": ("rec36", False, 0, False),            # ls_accumulate36_kernel<true>: label words at W = 136, bytes at W = 139
    "rec36-labels-misaligned": ("rec36", False, 0, True),  # ... bytes at W % 4 == 0
    "rec40-argmax": ("rec40", True, 0, False),             # ls_accumulate_kernel, every offset non-zero
    "rec40-labels": ("rec40", False, 0, False),
    "rec32-labels": ("rec32", False, 0, False),            # objects = 5
    "rec36-sigmoid": ("rec36", True, 1, False),            # the production record with the other weight: the generic kernel
}
FORWARD_CASES = [(c, w) for c in FORWARD for w in L.WIDTHS if not (FORWARD[c][3] and w % 4)]


@functools.lru_cache(maxsize=None)
def forward_reference(case, w):
    layout, argmax, sigmoid, _ = FORWARD[case]
    s = L.scene(w, argmax=argmax, **L.LAYOUTS[layout])
    lab = L.argmax_labels(s.field, s.seg_off, s.objects) if argmax else s.labels
    assert np.array_equal(lab, s.labels)
    t32, _ = L.terms(s.field, s.ld, s.dir_off, s.conf_off, sigmoid, s.h)
    ref, mag = L.sums(t32, lab, s.objects)
    return s, ref, mag


@pytest.fixture(scope="module")
def forward_run(hip_lib, device):
    done = {}

    def run(case, w):
        if (case, w) not in done:
            layout, argmax, sigmoid, misalign = FORWARD[case]
            s, _, _ = forward_reference(case, w)
            sums, kp = vote(hip_lib, device, s.field, None if argmax else s.labels, L.LAYOUTS[layout], sigmoid, misalign)
            done[case, w] = (sums.cpu().numpy(), kp.cpu().numpy())
        return done[case, w]
    return run


@pytest.mark.parametrize("case,w", FORWARD_CASES)
def test_forward_sums_match_the_fp32_order_terms(forward_run, case, w):
    s, ref, mag = forward_reference(case, w)
    got, kp = forward_run(case, w)
    present = mag > 0
    absent = ~present.any((0, 2, 3))
    assert absent.sum() == (3 if s.objects == 8 else 0) and present[:, ~absent].all()
    assert not got[:, absent].any() and not kp[:, absent].any()               # exactly 0
    assert np.isfinite(got).all() and np.isfinite(kp).all()                   # no NaN of the unused channels or the background came through
    ratio = np.abs(got - ref) / np.where(present, mag, 1.0)
    per_entry = ratio.max((0, 1, 2))
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s w=%d: |err| / sum|term| per entry (S00 S01 S11 T0 T1) %s, object %d (weights ~3e-7) %.2e; worst at (image, object, keypoint, entry) %s, "
          "condition number %.0f" % (case, w, " ".join("%.2e" % v for v in per_entry), L.TINY, ratio[:, L.TINY - 1].max(), at, L.condition(ref)[at[:3]]))
    assert ratio.max() <= FWD_GATE[case], (case, w, float(ratio.max()))


def solve_tolerance(ref, cond, h):
    """The device rounds p to fp32, then H, then the product: 3 * 2^-24 |ref|; its closed-form fp64 solve and the SVD of the reference differ by the
    system's conditioning: 1e-10 * cond * H covers cond * eps(fp64) many times."""
    return 3 * 2.0 ** -24 * np.abs(ref) + 1e-10 * cond[..., None] * h


@pytest.mark.parametrize("case,w", FORWARD_CASES)
def test_solve_matches_pinv_of_the_device_sums(forward_run, case, w):
    s, _, mag = forward_reference(case, w)
    sums, kp = forward_run(case, w)
    ref, cond = L.solve(sums, s.h), L.condition(sums)
    present = mag.any((2, 3))
    assert np.isfinite(cond[present]).all() and cond[present].max() <= 200 and not ref[~present].any()
    cond = np.where(present[..., None], cond, 0.0)
    err, tol = np.abs(kp - ref), solve_tolerance(ref, cond, s.h)
    assert (err <= tol).all(), (case, w, float((err / np.where(tol > 0, tol, 1.0)).max()))


# ---- backward -----------------------------------------------------------------------------------------------------------------------------------
BACKWARD = {   # id: (layout, dld, ddir_off, dconf_off)
    "bwd36": ("rec36", 64, 32, 50),           # ls_bwd36_kernel
    "generic40": ("rec40", 44, 3, 30),        # ls_bwd_kernel<9>
    "generic36": ("rec36", 30, 1, 20),        # the production record with a gradient row that fails the rec36 condition
}
MODES = list(itertools.product((0, 1), (True, False)))     # accumulate, regulariser given


def run_backward(lib, device, s, grad, accumulate, reg, dkp, coef, canary, sums=None):
    """Forward with given labels (unless sums are passed), then cp_ls_vote_bwd_f32.  Returns (sums, keypoints, pu, dfield) as NumPy arrays."""
    from casapose_amd import _lib

    dld, ddir_off, dconf_off = grad
    lay = dict(seg_off=s.seg_off, dir_off=s.dir_off, conf_off=s.conf_off, objects=s.objects)
    kp = None
    f = torch.from_numpy(s.field).to(device)
    if sums is None:
        sums, kp = vote(lib, device, f, s.labels, lay)
    lab, lab_ptr = _labels_on_device(s.labels, device)
    reg_t, reg_ptr = _labels_on_device(s.reg_labels, device) if reg else (None, None)
    coef_t = torch.from_numpy(coef).to(device) if reg else None
    dkp_t = torch.from_numpy(dkp).to(device)
    pu = torch.full((s.b, s.objects, KP, 4), 7.0, dtype=torch.float32, device=device)
    dfield = canary.to(device) if isinstance(canary, torch.Tensor) else torch.from_numpy(canary).to(device)
    assert dfield.shape == (s.b, s.h, s.w, dld) and dfield.dtype == torch.float32 and dfield.is_contiguous()
    _lib.check(lib.cp_ls_vote_bwd_f32(f.data_ptr(), s.ld, s.dir_off, s.conf_off, lab_ptr, s.b, s.h, s.w, s.objects, KP, sums.data_ptr(), dkp_t.data_ptr(),
                                      pu.data_ptr(), reg_ptr, coef_t.data_ptr() if reg else None, dfield.data_ptr(), dld, ddir_off, dconf_off, accumulate,
                                      _stream(device)), "cp_ls_vote_bwd_f32")
    torch.cuda.synchronize(device)
    del lab, reg_t
    return sums.cpu().numpy(), None if kp is None else kp.cpu().numpy(), pu.cpu().numpy(), dfield.cpu().numpy()


def canary_values(shape, seed):
    """Random fp32 values of magnitude 1e-3..2e-3, either sign, never zero."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(1e-3, 2e-3, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def slice_norms(s, idx, gd, gcf, reg):
    """Per listed pixel and keypoint, the largest reference magnitude of its slice: (image, object, keypoint) for the pixels with a label, separately for
    directions and confidences; (image, keypoint) over the pixels that only the regulariser touches."""
    lab, img = s.labels.reshape(-1)[idx], idx // (s.h * s.w)
    nd, nc = np.zeros(gcf.shape), np.zeros(gcf.shape)
    for bi in range(s.b):
        for o in range(s.objects + 1):
            m = (img == bi) & (lab == o)
            if m.any() and (o > 0 or reg):
                nd[m], nc[m] = np.abs(gd[m]).max((0, 2)), np.abs(gcf[m]).max(0)
    return nd, nc


def check_backward(s, grad, kernel36, accumulate, reg, coef, pu, canary, got, gate, what):
    """Every assertion of one backward call against the closed form on the table `pu`; returns the largest slice-relative error."""
    dld, ddir_off, dconf_off = grad
    n = s.b * s.h * s.w
    got, canary = got.reshape(n, dld), canary.reshape(n, dld)
    written = np.zeros(dld, bool)
    written[ddir_off:ddir_off + 18] = written[dconf_off:dconf_off + 9] = True
    idx, gd, gcf = L.pixel_grads(s.field, s.dir_off, s.conf_off, s.labels, s.reg_labels if reg else None, coef if reg else None, pu, s.h)
    lab = s.labels.reshape(-1)
    rlab = s.reg_labels.reshape(-1) if reg else np.zeros_like(lab)
    classes = [(lab > 0) & (rlab > 0), (lab > 0) & (rlab == 0), (lab == 0) & (rlab > 0), (lab == 0) & (rlab == 0)]
    assert all(c.any() for c in classes) if reg else (classes[1].any() and classes[3].any())
    assert np.array_equal(idx, np.flatnonzero(~classes[3]))
    # 1. nothing outside the written channels moved -- except the one float behind the 27 values that ls_bwd36_kernel zeroes in overwrite mode
    outside = ~written
    pad = ddir_off + 27
    if kernel36 and not accumulate:
        outside[pad] = False
        assert not got[:, pad].any(), what
    assert np.array_equal(bits(got[:, outside]), bits(canary[:, outside])), what
    # 2. pixels that neither map labels: exact zeros, or untouched
    quiet = np.flatnonzero(classes[3])
    if accumulate:
        assert np.array_equal(bits(got[quiet]), bits(canary[quiet])), what
    else:
        assert not got[quiet][:, written].any(), what
    # 3. the values
    base = canary[idx].astype(np.float64) if accumulate else np.zeros((idx.size, dld))
    want_d = base[:, ddir_off:ddir_off + 18].reshape(-1, KP, 2) + gd
    want_c = base[:, dconf_off:dconf_off + 9] + gcf
    got_d, got_c = got[idx, ddir_off:ddir_off + 18].reshape(-1, KP, 2).astype(np.float64), got[idx, dconf_off:dconf_off + 9].astype(np.float64)
    nd, nc = slice_norms(s, idx, gd, gcf, reg)
    # in accumulate mode the kernel's fp32 sum with the canary rounds once more: 2^-24 of the result, taken off before the ratio is formed
    extra = 2.0 ** -24 * 1.001 if accumulate else 0.0
    err_d = np.maximum(np.abs(got_d - want_d) - extra * np.abs(want_d), 0.0).max(-1)
    err_c = np.maximum(np.abs(got_c - want_c) - extra * np.abs(want_c), 0.0)
    only_reg = lab[idx] == 0
    assert not err_d[only_reg].any(), what                       # directions of a pixel that only the regulariser touches: 0 / the canary, exactly
    with np.errstate(divide="ignore", invalid="ignore"):         # a slice whose reference is all zero (a degenerate system) admits no error at all
        rd = float(np.where(err_d > 0, err_d / nd, 0.0)[~only_reg].max())
        rc = float(np.where(err_c > 0, err_c / nc, 0.0).max())
    # 4. zero directions: gd = 0 exactly, gcf = (u . e) sigmoid (in want_c)
    dz = ~s.field.reshape(n, s.ld)[idx][:, s.dir_off:s.dir_off + 18].reshape(-1, KP, 2).any(-1) & ~only_reg[:, None]
    assert 0.005 < dz.mean() < 0.03 and not gd[dz].any()
    assert np.array_equal(bits(got[idx, ddir_off:ddir_off + 18].reshape(-1, KP, 2)[dz]), bits(base[:, ddir_off:ddir_off + 18].reshape(-1, KP, 2)[dz].astype(np.float32))), what
    print("%s: directions %.2e, confidences %.2e of the slice's largest gradient" % (what, rd, rc))
    assert np.isfinite(got).all() and max(rd, rc) <= gate, (what, rd, rc)
    return max(rd, rc)


@functools.lru_cache(maxsize=None)
def backward_inputs(layout, w=139, rank_one=False):
    s = L.scene(w, reg=True, rank_one=rank_one, **L.LAYOUTS[layout])
    rng = np.random.default_rng(11)
    dkp = rng.normal(0, 1, (s.b, s.objects, KP, 2)).astype(np.float32)
    coef = (rng.normal(0, 1, (s.b, KP)) * 0.05).astype(np.float32)          # every image its own coefficients
    assert np.abs(coef[0] - coef[1]).min() > 1e-4 and np.abs(coef[0] - coef[2]).min() > 1e-4
    return s, dkp, coef


@pytest.mark.parametrize("accumulate,reg", MODES)
@pytest.mark.parametrize("case", sorted(BACKWARD))
def test_backward_pixels_match_the_closed_form_on_the_device_table(hip_lib, device, case, accumulate, reg):
    layout, *grad = BACKWARD[case]
    s, dkp, coef = backward_inputs(layout)
    canary = canary_values((s.b, s.h, s.w, grad[0]), 17)
    sums, kp, pu, got = run_backward(hip_lib, device, s, grad, accumulate, reg, dkp, coef, canary)
    check_backward(s, grad, case == "bwd36", accumulate, reg, coef, pu, canary, got, BWD_GATE[case],
                   "%s accumulate=%d %s" % (case, accumulate, "reg_labels + conf_coef" if reg else "no regulariser"))


@pytest.mark.parametrize("layout", ["rec36", "rec40"])
def test_backward_table_matches_cramer_on_the_device_sums(hip_lib, device, layout):
    """pu_ws = (p, u) rounded to fp32 (2^-23 covers the rounding twice); the device and the reference evaluate the same fp64 formula on the same sums,
    so they differ by a few eps(fp64) * cond of the value: 1e-10 * cond times the pair's magnitude covers that many times."""
    s, dkp, coef = backward_inputs(layout)
    grad = BACKWARD["bwd36" if layout == "rec36" else "generic40"][1:]
    sums, kp, pu, _ = run_backward(hip_lib, device, s, grad, 0, False, dkp, coef, canary_values((s.b, s.h, s.w, grad[0]), 1))
    ref, cond = L.prepare(sums, dkp, s.h)
    present = np.isfinite(cond)
    assert present[:, :5].all() and not present[:, 5:].any() and cond[present].max() <= 200
    assert not pu[~present].any() and pu[present].all()
    scale = np.concatenate([np.ones(ref.shape[:-1] + (2,)), np.repeat(np.abs(ref[..., 2:]).max(-1, keepdims=True), 2, -1)], -1)
    tol = 2.0 ** -23 * np.abs(ref) + 1e-10 * np.where(present, cond, 0.0)[..., None] * scale
    assert (np.abs(pu - ref) <= tol).all()
    assert (np.abs(kp - L.solve(sums, s.h)) <= solve_tolerance(L.solve(sums, s.h), np.where(present, cond, 0.0), s.h)).all()


def test_rank_one_object_votes_its_weighted_column_and_passes_no_gradient(hip_lib, device):
    """Every direction of object 5 is exactly (1, 0): r00 = r01 = 0, det = 0.  The forward gives y = 0 and x = sum w (x + .5) / sum w (its weights
    carry the forward's relative error, gate g <= 2e-6, and x - xbar spans at most W: 2 g W pixels); the backward calls the system degenerate."""
    s, dkp, coef = backward_inputs("rec36", rank_one=True)
    grad = BACKWARD["bwd36"][1:]
    canary = canary_values((s.b, s.h, s.w, grad[0]), 2)
    sums, kp, pu, got = run_backward(hip_lib, device, s, grad, 0, False, dkp, coef, canary)
    r1 = L.RANK_ONE - 1
    assert not sums[:, r1][..., [0, 1, 3]].any() and (sums[:, r1, :, 2] > 0).all()
    assert not kp[:, r1, :, 0].any()
    for bi in range(s.b):
        m = s.labels[bi] == L.RANK_ONE
        wgt = np.logaddexp(0.0, s.field[bi][m][:, s.conf_off:s.conf_off + KP].astype(np.float64))
        x = (wgt * (np.nonzero(m)[1] + 0.5)[:, None]).sum(0) / wgt.sum(0)
        assert np.abs(kp[bi, r1, :, 1] - x).max() <= 2 * 2e-6 * s.w
    assert not pu[:, r1].any() and pu[:, :4].all()                           # four exact zeros
    own = (s.labels == L.RANK_ONE).reshape(-1)
    g = got.reshape(-1, grad[0])[own]
    assert not g[:, grad[1]:grad[1] + 28].any()                              # no gradient through a degenerate system
    check_backward(s, grad, True, 0, False, coef, pu, canary, got, BWD_GATE["bwd36"], "bwd36 with the rank-one object")


def test_forward_and_backward_match_the_fp64_chain(hip_lib, device):
    """End to end: the device's forward sums, table and pixel pass against terms -> sums -> prepare -> pixel_grads wholly in fp64, which
    test_ls_reference pins to fp64 autograd of the reference voter (3e-12).  The fp32 (p, u) table alone costs 2.8e-6 of this on the CPU."""
    s, dkp, coef = backward_inputs("rec36")
    grad = BACKWARD["bwd36"][1:]
    canary = canary_values((s.b, s.h, s.w, grad[0]), 3)
    _, _, _, got = run_backward(hip_lib, device, s, grad, 0, True, dkp, coef, canary)
    _, t64 = L.terms(s.field, s.ld, s.dir_off, s.conf_off, 0, s.h)
    sm, _ = L.sums(t64, s.labels, s.objects)
    pu64, _ = L.prepare(sm, dkp, s.h)
    check_backward(s, grad, True, 0, True, coef, pu64, canary, got, E2E_GATE, "end to end, bwd36")


# ---- the grid-stride wrap -----------------------------------------------------------------------------------------------------------------------
WRAP_B, WRAP_H, WRAP_W, CAP = 2, 736, 720, 4096 * 256


@functools.lru_cache(maxsize=None)
def wrap_inputs():
    """2 x 736 x 720 = 1,059,840 pixels, 11,264 past the 4096 x 256 threads of the backward's grid: rows 721.. of image 1.  Labels and reg labels are a few
    rectangles (all four classes past the cap), random directions (systems near w/2 I), NaN wherever nothing is read."""
    rng = np.random.default_rng(23)
    b, h, w = WRAP_B, WRAP_H, WRAP_W
    lab, reg = np.zeros((b, h, w), np.uint8), np.zeros((b, h, w), np.uint8)
    lab[0, 5:40, 7:90], lab[0, 300:330, 600:720], lab[1, 0:20, 0:100] = 1, 2, 3
    lab[1, 700:736, 100:301], lab[1, 728:736, 650:720] = 1, 8
    reg[0, 20:60, 50:120], reg[1, 710:736, 200:401], reg[1, 10:30, 90:110] = 4, 2, 1
    field = np.full((b * h * w, 36), np.nan, np.float32)
    used = np.flatnonzero((lab > 0).reshape(-1) | (reg > 0).reshape(-1))
    rec = rng.normal(0, 1, (used.size, 27))
    rec[:, 18:] *= 1.5
    zero = rng.random((used.size, KP)) < 0.02
    d = rec[:, :18].reshape(-1, KP, 2)
    d[zero] = 0.0
    field[used, 9:] = rec
    s = SimpleNamespace(field=field.reshape(b, h, w, 36), labels=lab, reg_labels=reg, b=b, h=h, w=w, ld=36, seg_off=0, dir_off=9, conf_off=27, objects=8, kp=KP)
    dkp = rng.normal(0, 1, (b, 8, KP, 2)).astype(np.float32)
    coef = (rng.normal(0, 1, (b, KP)) * 1e-4).astype(np.float32)
    past = np.arange(b * h * w) >= CAP
    a, r = lab.reshape(-1) > 0, reg.reshape(-1) > 0
    assert b * h * w > CAP and all((past & m).any() for m in (a & r, a & ~r, ~a & r, ~a & ~r)) and lab.max() <= 8
    return s, dkp, coef


@pytest.mark.parametrize("case,accumulate", [("bwd36", 1), ("generic36", 0)])
def test_backward_covers_the_pixels_past_its_grid(hip_lib, device, case, accumulate):
    s, dkp, coef = wrap_inputs()
    grad = (28, 0, 18) if case == "bwd36" else (28, 0, 19)                   # dconf_off != ddir_off + 18: the generic kernel
    g = torch.Generator(device="cpu").manual_seed(5)
    canary = ((torch.rand((s.b, s.h, s.w, 28), generator=g) + 1.0) * 1e-3).numpy()
    sums, kp, pu, got = run_backward(hip_lib, device, s, grad, accumulate, True, dkp, coef, canary)
    cond = L.condition(sums)
    assert all(np.isfinite(cond[bi, o - 1]).all() and cond[bi, o - 1].max() < 2 for bi in range(s.b) for o in np.unique(s.labels[bi]) if o > 0)
    check_backward(s, grad, case == "bwd36", accumulate, True, coef, pu, canary, got, WRAP_GATE[case], "wrap %s accumulate=%d" % (case, accumulate))


# ---- statistics and reprojection loss -----------------------------------------------------------------------------------------------------------
def test_kp_stats_past_one_pass_of_its_grid(hip_lib, device):
    from casapose_amd import _lib

    b, h, w, classes, ld, conf_off = 2, 260, 256, 9, 12, 2                   # 66,560 pixels per image: 1,024 past the 256 x 256 threads of an image
    rng = np.random.default_rng(31)
    lab = rng.integers(0, classes, (b, h, w)).astype(np.uint8)
    lab[:, 100:200] = 0
    lab[1, 257:, 100:] = 7                                                    # bins that only the second pass fills differently per image
    est = rng.integers(0, classes, (b, h, w)).astype(np.uint8)
    est[rng.random((b, h, w)) < 0.1] = 9
    est[0, 258:, :50], est[1, 3, :7] = 200, 255
    assert lab.max() < classes and (est >= classes).sum() > 1000 and h * w > 65536
    field = np.full((b, h, w, ld), np.nan, np.float32)
    conf = rng.normal(0, 3, (b, h, w, KP))
    conf = np.where(rng.random(conf.shape) < 0.05, rng.uniform(-20, 20, conf.shape), conf)
    field[..., conf_off:conf_off + KP] = np.where((lab > 0)[..., None], conf, np.nan)
    f, lab_d, est_d = (torch.from_numpy(a).to(device) for a in (field, lab, est))
    counts = torch.full((2, b, classes), -5, dtype=torch.int32, device=device)
    cs = torch.full((b, KP), 7.0, dtype=torch.float64, device=device)
    _lib.check(hip_lib.cp_kp_stats_f32(f.data_ptr(), ld, conf_off, lab_d.data_ptr(), est_d.data_ptr(), b, h, w, classes, KP, counts.data_ptr(), cs.data_ptr(),
                                       _stream(device)), "cp_kp_stats_f32")
    want_counts, want_cs = L.kp_stats(field, conf_off, lab, est, classes)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    ratio = np.abs(cs.cpu().numpy() - want_cs) / want_cs
    print("conf_sums: %.2e of the sum" % ratio.max())
    assert ratio.max() <= CONF_SUM_GATE
    # without an estimated map the second table stays zero
    _lib.check(hip_lib.cp_kp_stats_f32(f.data_ptr(), ld, conf_off, lab_d.data_ptr(), None, b, h, w, classes, KP, counts.data_ptr(), cs.data_ptr(), _stream(device)),
               "cp_kp_stats_f32")
    got = counts.cpu().numpy()
    assert np.array_equal(got[0], want_counts[0]) and not got[1].any()


def test_kp_reproj_loss_past_one_pass_of_its_block(hip_lib, device):
    from casapose_amd import _lib

    coords, gt, A, avail, cap = L.reproj_case()
    b, objects, kp = coords.shape[:3]
    assert b * objects * kp == 288 > 256
    weight = 0.007
    want_v, want_g = L.kp_reproj_loss(coords, gt, A, avail, cap, weight)
    c_d, gt_d, a_d, av_d = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (coords, gt, A, avail))
    for av, (wv, wg) in ((av_d, (want_v, want_g)), (torch.zeros_like(av_d), (0.0, np.zeros_like(want_g)))):
        g = torch.full(coords.shape, 7.0, dtype=torch.float32, device=device)
        val = torch.full((1,), 7.0, dtype=torch.float64, device=device)
        _lib.check(hip_lib.cp_kp_reproj_loss_f32(c_d.data_ptr(), gt_d.data_ptr(), a_d.data_ptr(), av.data_ptr(), b, objects, kp, cap, weight, g.data_ptr(),
                                                 val.data_ptr(), _stream(device)), "cp_kp_reproj_loss_f32")
        got_g, got_v = g.cpu().numpy().astype(np.float64), float(val.item())
        if wv == 0.0:
            assert got_v == 0.0 and not got_g.any()                          # nothing available: value 0, zero gradients
            continue
        point = np.abs(wg).max(-1)
        zero = point == 0
        assert zero[1, 2].all() and zero[3, 7].all() and zero[2, 3, 4] and zero.sum() == 19 and not got_g[zero].any()
        rv = abs(got_v - wv) / wv
        rg = (np.abs(got_g - wg).max(-1)[~zero] / point[~zero]).max()
        print("reprojection loss: value %.2e, gradient %.2e of the point's larger component" % (rv, rg))
        assert rv <= REPROJ_VALUE_GATE and rg <= REPROJ_GRAD_GATE
