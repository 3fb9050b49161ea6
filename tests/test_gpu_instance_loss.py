"""cp_pose_loss_inst_f32 (csrc/loss_kernels.hip: the pose loss with an instance axis) checked stage by stage through the C ABI, in the manner of
test_gpu_loss_stages.py and with its bounds: what the kernels left in the caller's workspace is read through cp_pose_loss_inst_workspace_layout
and compared with the fp64 restatement of tests/instance_loss_reference.py --
  maps, counts and flags exactly; object sums, reported values and the three loss sums 1e-5; the gradient per image and there separately for
  the logit columns and the direction columns, max |got - ref| / max |ref| < 2e-5; zero blocks and every column outside the two blocks exactly 0.
Workspace, gradient rows, sums and values are pre-filled (0x00 / 0xFF / 0xA5), and a second call on the same workspace repeats the first.
The inputs and the property each is built for are in tests/instance_loss_cases.py; the properties, and outside the two tie cases the margin by
which the reference's choice of an instance stands clear of a tie, are asserted on the reference before the kernel's result is looked at.  No
pixel is exempt from a comparison.  Absent keypoints hold NaN: no NaN may appear in any result."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import instance_loss_cases as Ci
import loss_cases as Cs
from test_gpu_loss_stages import FILLS, REPEAT_TOL, check_merged, check_repeat, device_record, garbage, merged_layouts, run_merged, up4

pytestmark = pytest.mark.gpu
W = Ci.WEIGHTS
ENTRY = "cp_pose_loss_inst_f32"


def run_inst(lib, device, c, kpts, counts, imap, seg, prox, ld, dld, vert_off, fill, misalign=False, calls=1, instances=None, call_ld=None, expect_error=None):
    """`calls` calls of cp_pose_loss_inst_f32 on ONE workspace pre-filled (once) with the byte `fill`; what each left behind, as NumPy arrays.
    c: anything with out / labels_ce / labels_fg / K / kp.  call_ld: the stride the call is told (the record keeps ld).  expect_error: the call must fail; returns the buffers as they are afterwards."""
    from casapose_amd import _lib

    b, h, w = c.labels_fg.shape
    px, objects = b * h * w, c.K - 1
    offs, offs0 = (C.c_size_t * 5)(), (C.c_size_t * 5)()
    _lib.check(lib.cp_pose_loss_inst_workspace_layout(b, h, w, offs), "cp_pose_loss_inst_workspace_layout")
    _lib.check(lib.cp_pose_loss_workspace_layout(b, h, w, offs0), "cp_pose_loss_workspace_layout")
    nbytes = lib.cp_pose_loss_inst_workspace_bytes(b, h, w)
    assert list(offs) == list(offs0) and nbytes == lib.cp_pose_loss_workspace_bytes(b, h, w)      # the five products are where cp_pose_loss_f32 keeps them
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    rec = device_record(c, ld, device, misalign)
    ce, fg = (torch.from_numpy(np.array(a)).to(device) for a in (c.labels_ce, c.labels_fg))
    kd = None if kpts is None else torch.from_numpy(np.array(kpts)).to(device)
    cd = None if counts is None else torch.from_numpy(np.array(counts, np.int32)).to(device)
    md = None if imap is None else torch.from_numpy(np.array(imap)).to(device)
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    dout = torch.full((px, dld), 5.0, device=device)
    sums, vals = garbage(3, torch.float64, device), garbage(b * objects, torch.float32, device)
    I = instances if instances is not None else kpts.shape[2]
    results = []
    for _ in range(calls):
        st = lib.cp_pose_loss_inst_f32(rec.data_ptr(), ld if call_ld is None else call_ld, c.K, c.kp, ce.data_ptr(), fg.data_ptr(), ptr(kd), objects, I, ptr(cd), ptr(md), b, h, w, int(seg),
                                       int(prox), *W, ws.data_ptr(), dout.data_ptr(), dld, vert_off, sums.data_ptr(), vals.data_ptr(),
                                       torch.cuda.current_stream(device).cuda_stream)
        torch.cuda.synchronize(device)
        if expect_error is not None:
            msg = lib.cp_last_error().decode()
            assert st != 0 and ENTRY in msg and expect_error in msg, (st, msg)
            return SimpleNamespace(ws=ws.cpu().numpy(), dout=dout.cpu().numpy(), sums=sums.cpu().numpy(), values=vals.cpu().numpy())
        _lib.check(st, ENTRY)
        raw = ws.cpu().numpy()
        part = lambda i, dtype, n: raw[offs[i]:offs[i] + n * np.dtype(dtype).itemsize].view(dtype).copy()   # noqa: E731
        results.append(SimpleNamespace(fg=part(0, "u1", px).reshape(b, h, w), count=part(1, "<i4", b), objsum=part(2, "<f8", b * objects).reshape(b, objects),
                                       objcnt=part(3, "<i4", b * objects).reshape(b, objects), bad=part(4, "u1", b * objects).reshape(b, objects),
                                       values=vals.cpu().numpy().reshape(b, objects), sums=sums.cpu().numpy(),
                                       dout=dout.cpu().numpy().reshape(b, h, w, dld)))
    return results


def no_nan(got, failed, what):
    for n in ("objsum", "values", "sums", "dout"):
        if not np.isfinite(getattr(got, n)).all():
            failed.append("%s: %s holds a NaN or an infinity" % (what, n))


def rules(c):
    return (False, True) if c.imap is not None else (False,)


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill%02X" % f)
@pytest.mark.parametrize("seg", (False, True), ids=("nofilter", "segfilter"))
@pytest.mark.parametrize("name", Ci.SMALL)
def test_instance_stages(hip_lib, device, name, seg, fill):
    c = Ci.checked(name)                                    # the case's properties and margins are asserted in here, on the reference
    ld, dld, vert_off = up4(c.K + 2 * c.kp), 64, 32
    failed, by_rule = [], {}
    for use_map in rules(c):
        for prox in (False, True):
            ref = Ci.reference(name, use_map=use_map, seg=seg, prox=prox)
            first, second = run_inst(hip_lib, device, c, c.kpts, c.counts, c.imap if use_map else None, seg, prox, ld, dld, vert_off, fill, calls=2)
            what = "[%s rule, proxy filter %s]" % (("nearest", "map")[use_map], ("off", "on")[prox])
            print("%s %s seg %d: counts %s" % (name, what, seg, first.count.tolist()))
            failed += ["%s %s" % (what, f) for f in check_merged(first, ref, c, prox, vert_off)]
            no_nan(first, failed, what)
            check_repeat(first, second, ("fg", "count", "objcnt", "bad", "values"), failed)
            by_rule[use_map, prox] = first
    if name == "two_discs":                                 # the map and the nearest rule coincide: so do the two calls' results
        for prox in (False, True):
            a, m = by_rule[False, prox], by_rule[True, prox]
            for n in ("fg", "count", "objcnt", "bad", "values", "dout"):
                if not np.array_equal(getattr(a, n), getattr(m, n)):
                    failed.append("two_discs: %s differs between the two rules" % n)
            if not (np.abs(a.sums - m.sums) <= REPEAT_TOL * np.abs(a.sums)).all():
                failed.append("two_discs: sums %s and %s" % (a.sums.tolist(), m.sums.tolist()))
    assert not failed, " | ".join(failed[:12])


@pytest.mark.parametrize("shape", Ci.LAYOUT_SHAPES, ids=str)
def test_instance_layouts(hip_lib, device, shape):
    """(K, kp, I) through the row layouts that take the 16-byte path and the element path of loss_main_kernel, with the keypoint table staged in
    LDS and, for the last shape, read from global memory; both rules"""
    c = Ci.checked("layouts", *shape)
    layouts = merged_layouts(c.K, c.kp)
    assert [l[5] for l in layouts].count(True) == 1 and [l[5] for l in layouts].count(False) >= 1, layouts
    failed = []
    for use_map in (False, True):
        ref = Ci.reference("layouts", *shape, use_map=use_map, seg=True)
        for lname, ld, dld, vert_off, mis, vec in layouts:
            got, = run_inst(hip_lib, device, c, c.kpts, c.counts, c.imap if use_map else None, True, False, ld, dld, vert_off, 0xA5, misalign=mis)
            failed += ["[%s, %s rule] %s" % (lname, ("nearest", "map")[use_map], f) for f in check_merged(got, ref, c, False, vert_off)]
            no_nan(got, failed, lname)
    assert not failed, " | ".join(failed[:12])


def test_instance_second_trip(hip_lib, device):
    """more pixels per image than 512 blocks of 256 threads: the grid-stride loops take a second trip, in the float4 and the scalar instantiation,
    both filters on, both rules"""
    c = Ci.checked("second_trip")
    b, h, w = c.labels_fg.shape
    assert h * w > Cs.MERGED_GRID_CAP
    failed = []
    for use_map in (False, True):
        ref = Ci.reference("second_trip", use_map=use_map, seg=True, prox=True)
        for lname, ld, dld, vert_off, mis, vec in merged_layouts(c.K, c.kp):
            if lname in ("float4", "tight"):
                got, = run_inst(hip_lib, device, c, c.kpts, c.counts, c.imap if use_map else None, True, True, ld, dld, vert_off, 0xA5)
                failed += ["[%s, %s rule] %s" % (lname, ("nearest", "map")[use_map], f) for f in check_merged(got, ref, c, True, vert_off)]
    assert not failed, " | ".join(failed[:12])


@pytest.mark.parametrize("name", Cs.MERGED)
def test_one_instance_is_cp_pose_loss_f32(hip_lib, device, name):
    """instances == 1, every count 1, no map: fg, count, the object products and every byte of dout equal cp_pose_loss_f32's; the sums agree to the
    fp64 summation order.  Both row paths, all four filter combinations."""
    c = Cs.checked(name)
    kpts, counts = Ci.single_instance(c)
    failed = []
    for lname, ld, dld, vert_off, mis, vec in merged_layouts(c.K, c.kp):
        if lname not in ("float4", "tight"):
            continue
        for seg in (False, True):
            for prox in (False, True):
                old, = run_merged(hip_lib, device, c, seg, prox, ld, dld, vert_off, 0xA5)
                new, = run_inst(hip_lib, device, c, kpts, counts, None, seg, prox, ld, dld, vert_off, 0xA5)
                for n in ("fg", "count", "objsum", "objcnt", "bad", "values"):
                    if not np.array_equal(getattr(old, n), getattr(new, n)):
                        failed.append("[%s seg %d prox %d] %s differs" % (lname, seg, prox, n))
                if old.dout.tobytes() != new.dout.tobytes():
                    failed.append("[%s seg %d prox %d] dout: %d entries differ" % (lname, seg, prox, int((old.dout != new.dout).sum())))
                if not (np.abs(old.sums - new.sums) <= REPEAT_TOL * np.abs(old.sums)).all():
                    failed.append("[%s seg %d prox %d] sums %s, cp_pose_loss_f32 %s" % (lname, seg, prox, new.sums.tolist(), old.sums.tolist()))
    assert not failed, " | ".join(failed[:12])


def test_refusals_launch_nothing(hip_lib, device):
    """a null inst_counts, instances outside 1..16 and what cp_pose_loss_f32 refuses: an error that names the entry, and the pre-filled workspace,
    gradient rows, sums and values as they were"""
    c = Ci.checked("occluding")
    ld, dld, vert_off = up4(c.K + 2 * c.kp), 64, 32
    good = dict(kpts=c.kpts, counts=c.counts, dld=dld, vert_off=vert_off, instances=None, call_ld=None)
    bad = [("null pointer", dict(counts=None)), ("outside 1..16", dict(instances=0)), ("outside 1..16", dict(instances=17)),
           ("null pointer", dict(kpts=None)), ("ld <", dict(call_ld=c.K + 2 * c.kp - 1)), ("does not fit dld", dict(vert_off=c.K - 1)),
           ("does not fit dld", dict(dld=vert_off + 2 * c.kp - 1)), ("64-float rows", dict(dld=65))]
    for fill in FILLS:
        for expect, change in bad:
            a = dict(good, **change)
            left = run_inst(hip_lib, device, c, a["kpts"], a["counts"], c.imap, True, True, ld, a["dld"], a["vert_off"], fill, instances=c.I if a["instances"] is None else a["instances"],
                            call_ld=a["call_ld"], expect_error=expect)
            assert (left.ws == fill).all() and (left.dout == 5.0).all(), (expect, change)
            assert np.array_equal(left.sums, garbage(3, torch.float64, "cpu").numpy(), equal_nan=True)
            assert np.array_equal(left.values, garbage(left.values.size, torch.float32, "cpu").numpy(), equal_nan=True)
    b, h, w = c.labels_fg.shape
    assert hip_lib.cp_pose_loss_inst_workspace_layout(b, h, w, None) == -1 and b"cp_pose_loss_inst_workspace_layout" in hip_lib.cp_last_error()
    assert hip_lib.cp_pose_loss_inst_workspace_layout(0, h, w, (C.c_size_t * 5)()) == -1 and b"bad shape" in hip_lib.cp_last_error()
