#!/usr/bin/env python3
"""What the covariance per slot (cp_ls_slot_covariance_f32: the moments pass and its finish) costs, and that the two slot voters it shares its
kernels' source with cost what they cost before, at the bench shape: batch 16, 480 x 640, 8 objects, R = 4 (32 slots), the production record,
the ellipse masks of `bench.py --mode vote` (tools/probe_instance_vote.py's inputs) labelled by cp_ccl_instance_labels.

    python tools/probe_slot_cov.py [--parent-lib <libcasapose_hip.so of the parent commit>] [--out profiles/slot_cov_probe.txt]

With --parent-lib the plain voter (cp_ls_vote_slots_f32) and the robust voter at passes = 0 and 1 (cp_ls_vote_slots_robust_f32) are timed in
that library (a build of the commit before the covariance) and in this tree's, alternated inside every repeat: `--repeats` rounds of `--calls`
calls each between two device events, after a warm-up round of each; a line gives the median, the minimum and the maximum over the rounds in
microseconds per call.  A reweighted pass is (passes = 1) - (passes = 0) of the same library and round.  Then the new call with and without a
cut-off against this library's reweighted pass, and what it returns on this input."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from casapose_amd import _lib  # noqa: E402
from probe_instance_vote import B, H, KP, K, W, inputs  # noqa: E402

R = 4
SLOTS = (K - 1) * R
CUTOFF = 4.0


def bind_parent(path):
    lib = C.CDLL(path)
    lib.cp_ls_vote_slots_f32.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    lib.cp_ls_vote_slots_robust_f32.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_int] + [C.c_void_p] * 3
    if hasattr(lib, "cp_ls_slot_covariance_f32"):
        raise SystemExit("%s exports cp_ls_slot_covariance_f32: it is not a build of the parent commit" % path)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_slot_cov.py needs a ROCm GPU: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    rec, lab = inputs(dev)
    new = _lib.load()
    old = bind_parent(args.parent_lib) if args.parent_lib else None
    st = torch.cuda.current_stream(dev).cuda_stream

    def ok(rc, what):
        if rc != 0:
            raise SystemExit("%s failed (%d)" % (what, rc))

    ws = torch.empty(new.cp_ccl_instance_workspace_bytes(B, H, W, K - 1, R), dtype=torch.uint8, device=dev)
    slots, inst = torch.empty_like(lab), torch.empty(B, K - 1, R, 2, dtype=torch.int32, device=dev)
    ok(new.cp_ccl_instance_labels(lab.data_ptr(), B, H, W, K - 1, R, 50, ws.data_ptr(), slots.data_ptr(), inst.data_ptr(), st), "cp_ccl_instance_labels")

    calls, outs = {}, {}
    for tag, lib in (("parent", old), ("new", new)):
        if lib is None:
            continue
        sums, kp = torch.empty(B, SLOTS, KP, 5, dtype=torch.float64, device=dev), torch.empty(B, SLOTS, KP, 2, device=dev)

        def plain(lib=lib, sums=sums, kp=kp):
            ok(lib.cp_ls_vote_slots_f32(rec.data_ptr(), 36, 9, 27, slots.data_ptr(), B, H, W, SLOTS, KP, 0, sums.data_ptr(), kp.data_ptr(), st), "cp_ls_vote_slots_f32")

        calls["%s: cp_ls_vote_slots_f32" % tag] = plain
        outs[tag, "plain"] = kp
        for p in (0, 1):
            rws, rkp = torch.empty(2, B, SLOTS, KP, 5, dtype=torch.float64, device=dev), torch.empty(B, SLOTS, KP, 2, device=dev)

            def robust(lib=lib, p=p, rws=rws, rkp=rkp):
                ok(lib.cp_ls_vote_slots_robust_f32(rec.data_ptr(), 36, 9, 27, slots.data_ptr(), B, H, W, SLOTS, KP, 0, CUTOFF, p, rws.data_ptr(), rkp.data_ptr(), st),
                   "cp_ls_vote_slots_robust_f32")

            calls["%s: cp_ls_vote_slots_robust_f32, passes = %d" % (tag, p)] = robust
            outs[tag, p] = rkp
    kps = outs["new", 1]
    for name, cutoff in (("cut-off %g px" % CUTOFF, CUTOFF), ("no cut-off", 0.0)):
        sums = torch.empty(B, SLOTS, KP, 5, dtype=torch.float64, device=dev)
        cov, stat = torch.empty(B, SLOTS, KP, 3, device=dev), torch.empty(B, SLOTS, KP, 2, device=dev)

        def covariance(cutoff=cutoff, sums=sums, cov=cov, stat=stat):
            _lib.check(new.cp_ls_slot_covariance_f32(rec.data_ptr(), 36, 9, 27, slots.data_ptr(), B, H, W, SLOTS, KP, 0, cutoff, kps.data_ptr(), sums.data_ptr(),
                                                     cov.data_ptr(), stat.data_ptr(), st), "cp_ls_slot_covariance_f32")

        calls["new: cp_ls_slot_covariance_f32, %s" % name] = covariance
        outs["cov", cutoff] = (cov, stat)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3      # microseconds per call

    calls["new: cp_ls_vote_slots_robust_f32, passes = 1"]()     # the keypoints the covariance is asked about
    times = {name: [] for name in calls}
    for rep in range(args.repeats + 1):                       # round 0 is the warm-up
        for name, fn in calls.items():                        # alternated: every round times every call
            t = timed(fn)
            if rep:
                times[name].append(t)
    lines = ["probe_slot_cov: batch %d, %d x %d, 8 objects, R = %d (%d slots), record 36, ellipse masks (%.1f %% foreground), cut-off %g px; "
             "%d rounds of %d calls, us per call: median (min .. max)" % (B, H, W, R, SLOTS, 100.0 * float((lab > 0).float().mean()), CUTOFF, args.repeats, args.calls),
             "device: %s" % torch.cuda.get_device_name(dev)]
    for name, c in times.items():
        lines.append("%-58s %7.1f (%7.1f .. %7.1f)" % (name, np.median(c), min(c), max(c)))

    def a_pass(tag):
        return np.array(times["%s: cp_ls_vote_slots_robust_f32, passes = 1" % tag]) - np.array(times["%s: cp_ls_vote_slots_robust_f32, passes = 0" % tag])

    new_pass = a_pass("new")
    if old is not None:
        base = times["parent: cp_ls_vote_slots_f32"]
        lines.append("cp_ls_vote_slots_f32, new against parent: %+.1f us (the parent's own rounds spread over %.1f us)"
                     % (np.median(times["new: cp_ls_vote_slots_f32"]) - np.median(base), max(base) - min(base)))
        old_pass = a_pass("parent")
        lines.append("a reweighted pass, parent %.1f us (%.1f .. %.1f), new %.1f us (%.1f .. %.1f): %+.1f us (the parent's own rounds spread over %.1f us)"
                     % (np.median(old_pass), old_pass.min(), old_pass.max(), np.median(new_pass), new_pass.min(), new_pass.max(),
                        np.median(new_pass) - np.median(old_pass), old_pass.max() - old_pass.min()))
    else:
        lines.append("a reweighted pass: %.1f us (%.1f .. %.1f)" % (np.median(new_pass), new_pass.min(), new_pass.max()))
    for name in ("cut-off %g px" % CUTOFF, "no cut-off"):
        c = np.array(times["new: cp_ls_slot_covariance_f32, %s" % name])
        lines.append("the moments pass with its finish, %s: %.1f us, %.2f x the reweighted pass of the same run (whose rounds spread over %.1f us)"
                     % (name, np.median(c), np.median(c) / np.median(new_pass), new_pass.max() - new_pass.min()))
    for fn in calls.values():
        fn()
    torch.cuda.synchronize(dev)
    if old is not None:
        lines.append("new against parent: keypoints of the plain voter differ by at most %.3g px, of the robust voter after one pass by at most %.3g px"
                     % (float((outs["new", "plain"] - outs["parent", "plain"]).abs().max()), float((outs["new", 1] - outs["parent", 1]).abs().max())))
    for cutoff in (CUTOFF, 0.0):
        cov, stat = outs["cov", cutoff]
        has = torch.isfinite(cov).all(-1)
        lines.append("covariance at cut-off %g px: %d of %d keypoints have one; sigma2 median %.3g px^2, kept median %.3f, variances median %.3g, largest %.3g px^2"
                     % (cutoff, int(has.sum()), has.numel(), float(stat[..., 0][has].median()), float(stat[..., 1][has].median()),
                        float(cov[has][:, [0, 2]].median()), float(cov[has][:, [0, 2]].max())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
