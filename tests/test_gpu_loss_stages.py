"""The training losses (csrc/loss_kernels.hip: cp_pose_loss_f32, up to five kernels; csrc/loss_functional.hip: cp_pose_loss_sep_f32, two) checked
stage by stage: the C ABI is called directly, what the kernels left in the caller's workspace is read through cp_pose_loss_workspace_layout /
cp_pose_loss_sep_workspace_layout and compared with the fp64 restatement of tests/loss_reference.py --
  a. the filtered foreground map and its counts (exactly),  b. the proxy filter's per-object pixel counts and flags (exactly), sums and reported
  values (1e-5),  c. the three loss sums (1e-5; a term that is exactly 0 in the reference: below 1e-12),  d. the gradient, per image and there
  separately for the logit columns and the direction columns (max |got - ref| / max |ref| of the block < 2e-5; a block that is zero in the reference
  and every column outside the two blocks: exactly zero).
The bounds are those of test_gpu_train.py::test_pose_loss_value_and_gradient, applied per block so that a small block cannot hide behind a large one.
The inputs and the properties each is chosen for are in tests/loss_cases.py; those properties are asserted on the reference before the kernel's
result is looked at.  Workspace, gradient rows, sums and values are pre-filled: nothing may depend on what they held, and a second call on the
same workspace gives the same maps and (to fp64 summation order) the same sums."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_cases as Cs

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
SUM_TOL, GRAD_TOL, PATHS_TOL, REPEAT_TOL = 1e-5, 2e-5, 1e-6, 1e-12
W = Cs.WEIGHTS


def up4(n):
    return (n + 3) // 4 * 4


def device_record(c, ld, device, misalign=False):
    """the case's tight record re-laid with row stride ld, the padding columns NaN; 16-byte aligned, or one float past an aligned address"""
    b, h, w, n = c.out.shape
    assert ld >= n
    rec = np.full((b * h * w, ld), np.nan, np.float32)
    rec[:, :n] = c.out.reshape(-1, n)
    buf = torch.empty(rec.size + 4, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + rec.size] if misalign else buf[:rec.size]
    view.copy_(torch.from_numpy(rec.ravel()))
    return view


def garbage(n, dtype, device):
    return torch.tensor(([float("nan"), 1e30, -7.0] * n)[:n], dtype=dtype, device=device)


def to_device(c, device):
    return tuple(torch.from_numpy(np.array(a)).to(device) for a in (c.labels_ce, c.labels_fg, c.kpts))


def run_merged(lib, device, c, seg, prox, ld, dld, vert_off, fill, misalign=False, calls=1):
    """`calls` calls of cp_pose_loss_f32 on ONE workspace pre-filled (once) with the byte `fill`; what each left behind, as NumPy arrays"""
    from casapose_amd import _lib

    b, h, w = c.labels_fg.shape
    px, objects = b * h * w, c.K - 1
    offs = (C.c_size_t * 5)()
    _lib.check(lib.cp_pose_loss_workspace_layout(b, h, w, offs), "cp_pose_loss_workspace_layout")
    nbytes = lib.cp_pose_loss_workspace_bytes(b, h, w)
    sizes = [px, 4 * b, 8 * b * 64, 4 * b * 64, b * 64]
    assert all(offs[i] + sizes[i] <= (offs[i + 1] if i < 4 else nbytes) for i in range(5))
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    rec = device_record(c, ld, device, misalign)
    ce, fg, kpts = to_device(c, device)
    dout = torch.full((px, dld), 5.0, device=device)
    sums, vals = garbage(3, torch.float64, device), garbage(b * objects, torch.float32, device)
    results = []
    for _ in range(calls):
        _lib.check(lib.cp_pose_loss_f32(rec.data_ptr(), ld, c.K, c.kp, ce.data_ptr(), fg.data_ptr(), kpts.data_ptr(), objects, b, h, w, int(seg), int(prox),
                                        *W, ws.data_ptr(), dout.data_ptr(), dld, vert_off, sums.data_ptr(), vals.data_ptr(),
                                        torch.cuda.current_stream(device).cuda_stream), "cp_pose_loss_f32")
        torch.cuda.synchronize(device)
        raw = ws.cpu().numpy()
        part = lambda i, dtype, n: raw[offs[i]:offs[i] + n * np.dtype(dtype).itemsize].view(dtype).copy()   # noqa: E731
        results.append(SimpleNamespace(fg=part(0, "u1", px).reshape(b, h, w), count=part(1, "<i4", b), objsum=part(2, "<f8", b * objects).reshape(b, objects),
                                       objcnt=part(3, "<i4", b * objects).reshape(b, objects), bad=part(4, "u1", b * objects).reshape(b, objects),
                                       values=vals.cpu().numpy().reshape(b, objects), sums=sums.cpu().numpy(),
                                       dout=dout.cpu().numpy().reshape(b, h, w, dld)))
    return results


def run_sep(lib, device, c, seg, ld, dld, vert_off, fill, calls=1):
    from casapose_amd import _lib

    b, h, w = c.labels_fg.shape
    px, objects = b * h * w, c.K - 1
    offs = (C.c_size_t * 2)()
    _lib.check(lib.cp_pose_loss_sep_workspace_layout(b, h, w, c.K, offs), "cp_pose_loss_sep_workspace_layout")
    nbytes = lib.cp_pose_loss_sep_workspace_bytes(b, h, w, c.K)
    assert offs[0] + px <= offs[1] and offs[1] % 4 == 0 and offs[1] + 4 * b * c.K <= nbytes
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    rec = device_record(c, ld, device)
    ce, fg, kpts = to_device(c, device)
    dout = torch.full((px, dld), 5.0, device=device)
    sums = garbage(3, torch.float64, device)
    results = []
    for _ in range(calls):
        _lib.check(lib.cp_pose_loss_sep_f32(rec.data_ptr(), ld, c.K, c.kp, ce.data_ptr(), fg.data_ptr(), kpts.data_ptr(), objects, b, h, w, int(seg), *W,
                                            ws.data_ptr(), dout.data_ptr(), dld, vert_off, sums.data_ptr(), torch.cuda.current_stream(device).cuda_stream),
                   "cp_pose_loss_sep_f32")
        torch.cuda.synchronize(device)
        raw = ws.cpu().numpy()
        results.append(SimpleNamespace(fg=raw[offs[0]:offs[0] + px].reshape(b, h, w).copy(), counts=raw[offs[1]:offs[1] + 4 * b * c.K].view("<i4").reshape(b, c.K).copy(),
                                       sums=sums.cpu().numpy(), dout=dout.cpu().numpy().reshape(b, h, w, dld)))
    return results


def block_error(got, ref):
    """max |got - ref| / max |ref| of one block; a block that is zero in the reference must be zero: inf otherwise"""
    scale = np.abs(ref).max() if ref.size else 0.0
    if scale == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(np.abs(got.astype(np.float64) - ref).max() / scale)


def check_sums(got, ref, failed):
    for i, name in enumerate(("mask", "vertex", "proxy")):
        want, have = getattr(ref, name), float(got.sums[i])
        err = abs(have - want)
        print("   %s %.9g reference %.9g (%.2e)" % (name, have, want, err / abs(want) if want else err))
        if not (err < 1e-12 if want == 0.0 else err < SUM_TOL * abs(want)):
            failed.append("c. %s loss: %.9g, reference %.9g" % (name, have, want))


def check_gradient(dout, blocks, ref_of, failed, tol=GRAD_TOL, what="reference"):
    """blocks: [(name, first column, width)]; ref_of(name) -> [b,h,w,width].  Per image and block, and exact zeros everywhere else"""
    b = dout.shape[0]
    used = np.zeros(dout.shape[-1], bool)
    worst = 0.0
    for name, first, width in blocks:
        used[first:first + width] = True
        ref = ref_of(name)
        for n in range(b):
            err = block_error(dout[n, :, :, first:first + width], ref[n])
            worst = max(worst, err)
            if not err < tol:
                failed.append("d. gradient, image %d, %s columns: %.3g of the block's maximum %.3g (%s)" % (n, name, err, np.abs(ref[n]).max(), what))
    print("   gradient blocks against the %s: worst %.2e" % (what, worst))
    if dout[..., ~used].any():
        failed.append("d. gradient: %d non-zero entries outside the logit and direction columns" % np.count_nonzero(dout[..., ~used]))


def check_merged(got, ref, c, prox, vert_off, with_objects=True):
    failed = []
    want_fg, want_count = (ref.fg1, ref.count1) if prox else (ref.fg0, ref.count0)
    if not np.array_equal(got.fg, want_fg):
        failed.append("a. foreground map: %d pixels differ" % int((got.fg != want_fg).sum()))
    if not np.array_equal(got.count, want_count):
        failed.append("a. counts %s, reference %s" % (got.count.tolist(), want_count.tolist()))
    if with_objects:
        if not np.array_equal(got.objcnt, ref.objcnt):
            failed.append("b. objcnt %s, reference %s" % (got.objcnt.tolist(), ref.objcnt.tolist()))
        if not np.array_equal(got.bad != 0, ref.bad) or not np.isin(got.bad, (0, 1)).all():
            failed.append("b. bad %s, reference %s" % (got.bad.tolist(), ref.bad.astype(int).tolist()))
        for name, have, want in (("objsum", got.objsum, ref.objsum), ("value", got.values, ref.value)):
            if not (np.abs(have - want) <= SUM_TOL * np.abs(want)).all():
                failed.append("b. %s %s, reference %s" % (name, have.tolist(), want.tolist()))
    check_sums(got, ref, failed)
    refs = {"logit": ref.grad_logits, "direction": ref.grad_dirs}
    check_gradient(got.dout, [("logit", 0, c.K), ("direction", vert_off, 2 * c.kp)], refs.__getitem__, failed)
    return failed


def check_repeat(first, second, names, failed):
    for n in names:
        if not np.array_equal(getattr(first, n), getattr(second, n)):
            failed.append("second call on the same workspace: %s differs" % n)
    if not (np.abs(first.sums - second.sums) <= REPEAT_TOL * np.abs(first.sums)).all():
        failed.append("second call on the same workspace: sums %s, then %s" % (first.sums.tolist(), second.sums.tolist()))
    if not np.array_equal(first.dout, second.dout):
        failed.append("second call on the same workspace: the gradient differs")


# ---- cp_pose_loss_f32 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill%02X" % f)
@pytest.mark.parametrize("seg", (False, True), ids=("nofilter", "segfilter"))
@pytest.mark.parametrize("name", Cs.MERGED)
def test_merged_stages(hip_lib, device, name, seg, fill):
    c = Cs.checked(name)                                    # the case's properties are asserted in here, on the reference
    ld, dld, vert_off = up4(c.K + 2 * c.kp), 64, 32
    failed = []
    for prox in (False, True):
        ref = Cs.reference(name, seg_filter=seg, proxy_filter=prox)
        first, second = run_merged(hip_lib, device, c, seg, prox, ld, dld, vert_off, fill, calls=2)
        print("%s seg %d prox %d: counts %s" % (name, seg, prox, first.count.tolist()))
        failed += ["[proxy filter %s] %s" % (("off", "on")[prox], f) for f in check_merged(first, ref, c, prox, vert_off)]
        check_repeat(first, second, ("fg", "count", "objcnt", "bad", "values"), failed)
    assert not failed, " | ".join(failed[:12])


def merged_layouts(K, kp):
    """[(name, ld, dld, vert_off, misaligned, float4 path)] that CP_REQUIRE admits: vert_off >= K, vert_off + 2kp <= dld <= 64; duplicates dropped.
    The last entry restates the launcher's choice: float4 rows iff ld % 4 == 0, dld == 64, vert_off == 32, both pointers 16-byte aligned and
    the logits' quads inside the row."""
    n, r4 = K + 2 * kp, up4(K + 2 * kp)
    seen, out = set(), []
    for name, ld, dld, vert_off, mis in (("float4", r4, 64, 32, False), ("ld_odd", n, 64, 32, False), ("pvnet", r4, 64, K, False), ("tight", n, n, K, False),
                                         ("misaligned", r4, 64, 32, True)):
        if vert_off < K or vert_off + 2 * kp > dld or dld > 64 or (ld, dld, vert_off, mis) in seen:
            continue
        seen.add((ld, dld, vert_off, mis))
        out.append((name, ld, dld, vert_off, mis, ld % 4 == 0 and dld == 64 and vert_off == 32 and not mis and up4(K) <= ld))
    return out


@pytest.mark.parametrize("K,kp", Cs.RECORD_SHAPES, ids=lambda v: str(v))
def test_merged_layout_sweep(hip_lib, device, K, kp):
    """every record shape through the float4 and the scalar instantiation of loss_main_kernel: both equal the reference, and each other to 1e-6
    per block (the arithmetic is the same; only the argument association of __expf / __logf may differ)"""
    c = Cs.checked("subset_fg", K, kp)
    ref = Cs.reference("subset_fg", K, kp, seg_filter=True)
    layouts = merged_layouts(K, kp)
    assert [l[5] for l in layouts].count(True) == 1 and [l[5] for l in layouts].count(False) >= 1, layouts
    failed, results = [], {}
    for name, ld, dld, vert_off, mis, vec in layouts:
        got, = run_merged(hip_lib, device, c, True, False, ld, dld, vert_off, 0xA5, misalign=mis)
        print("%s (ld %d, dld %d, vert_off %d): %s path" % (name, ld, dld, vert_off, "float4" if vec else "scalar"))
        failed += ["[%s] %s" % (name, f) for f in check_merged(got, ref, c, False, vert_off)]
        results[name] = (got, vert_off)
    wide, wide_off = results["float4"]
    for name, (got, vert_off) in results.items():
        if name != "float4":
            theirs = {"logit": wide.dout[..., :K].astype(np.float64), "direction": wide.dout[..., wide_off:wide_off + 2 * kp].astype(np.float64)}
            check_gradient(got.dout, [("logit", 0, K), ("direction", vert_off, 2 * kp)], theirs.__getitem__, failed, PATHS_TOL, "float4 path's result [%s]" % name)
    assert not failed, " | ".join(failed[:12])


def test_merged_second_trip(hip_lib, device):
    """more pixels per image than 512 blocks of 256 threads: the grid-stride loops of all five kernels take a second trip, in the float4 and in the
    scalar instantiation; both filters on"""
    c = Cs.checked("second_trip_merged")
    b, h, w = c.labels_fg.shape
    assert h * w > Cs.MERGED_GRID_CAP
    ref = Cs.reference("second_trip_merged", seg_filter=True, proxy_filter=True)
    failed = []
    for name, ld, dld, vert_off, mis, vec in merged_layouts(c.K, c.kp):
        if name in ("float4", "tight"):
            assert vec == (name == "float4")
            got, = run_merged(hip_lib, device, c, True, True, ld, dld, vert_off, 0xA5)
            failed += ["[%s] %s" % (name, f) for f in check_merged(got, ref, c, True, vert_off)]
    assert not failed, " | ".join(failed[:12])


# ---- cp_pose_loss_sep_f32 ---------------------------------------------------------------------------------------------------------------------------
def check_sep(got, ref, c, vert_off):
    failed = []
    if not np.array_equal(got.fg, ref.fg):
        failed.append("a. foreground map: %d pixels differ" % int((got.fg != ref.fg).sum()))
    if not np.array_equal(got.counts, ref.counts):
        failed.append("a. counts %s, reference %s" % (got.counts.tolist(), ref.counts.tolist()))
    check_sums(got, ref, failed)
    width = 2 * c.kp
    refs = {"logit": ref.grad_logits}
    refs.update({"object %d" % (o + 1): ref.grad_dirs[..., o * width:(o + 1) * width] for o in range(c.K - 1)})
    blocks = [("logit", 0, c.K)] + [("object %d" % (o + 1), vert_off + o * width, width) for o in range(c.K - 1)]
    check_gradient(got.dout, blocks, refs.__getitem__, failed)
    return failed


def sep_layouts(K, kp):
    """the plan's rows (a multiple of 32 floats, directions from column K) and the tight ones"""
    n = K + (K - 1) * 2 * kp
    return (("plan", (n + 31) // 32 * 32, (n + 31) // 32 * 32, K), ("tight", n, n, K))


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill%02X" % f)
@pytest.mark.parametrize("seg", (False, True), ids=("nofilter", "segfilter"))
@pytest.mark.parametrize("K", Cs.SEP_K, ids=lambda k: "K%d" % k)
@pytest.mark.parametrize("name", Cs.SEP)
def test_separated_stages(hip_lib, device, name, K, seg, fill):
    c = Cs.checked(name, K, 9, True)
    ref = Cs.reference(name, K, 9, True, seg_filter=seg)
    failed = []
    for lname, ld, dld, vert_off in sep_layouts(K, c.kp):
        first, second = run_sep(hip_lib, device, c, seg, ld, dld, vert_off, fill, calls=2)
        print("%s K %d seg %d %s: counts %s" % (name, K, seg, lname, first.counts.tolist()))
        failed += ["[%s] %s" % (lname, f) for f in check_sep(first, ref, c, vert_off)]
        check_repeat(first, second, ("fg", "counts"), failed)
    assert not failed, " | ".join(failed[:12])


def test_separated_second_trip(hip_lib, device):
    """more pixels per image than 1024 blocks of 256 threads: both kernels take a second trip"""
    c = Cs.checked("second_trip_sep")
    b, h, w = c.labels_fg.shape
    assert h * w > Cs.SEP_GRID_CAP
    ref = Cs.reference("second_trip_sep", sep=True, seg_filter=True)
    (lname, ld, dld, vert_off), _ = sep_layouts(c.K, c.kp)
    got, = run_sep(hip_lib, device, c, True, ld, dld, vert_off, 0xA5)
    failed = check_sep(got, ref, c, vert_off)
    assert not failed, " | ".join(failed[:12])
