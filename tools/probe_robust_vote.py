#!/usr/bin/env python3
"""The labelling + voter pair for several instances per object (cp_ccl_instance_labels + cp_ls_vote_slots_f32) against the same labelling with the
robust voter (cp_ls_vote_slots_robust_f32) at passes = 0, 1, 2, 3, at the bench shape: batch 16, 480 x 640, 8 objects, R = 4 (32 slots), the
production record, the ellipse masks of `bench.py --mode vote` (tools/probe_instance_vote.py's inputs).

    python tools/probe_robust_vote.py [--parent-lib <libcasapose_hip.so of the parent commit>] [--out profiles/robust_vote_probe.txt]

Parent pair: with --parent-lib both calls are made in that library (a build of the commit before the robust entry point); without it in this
tree's library, whose two entry points are the same code.  All pairs are alternated inside every repeat: `--repeats` rounds of `--calls` calls each
between two device events, after a warm-up round of each; the line of a pair gives the median, the minimum and the maximum over the rounds, per
call of the labelling, of the voter, and of both.  Below them: what a reweighted pass costs, (voter at passes = k - voter at passes = 0) / k from
the medians, beside the parent's voter (one accumulate + solve on the same input), and the keypoints at passes = 0 against the parent's."""
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
PASSES = (0, 1, 2, 3)


def bind_parent(path):
    lib = C.CDLL(path)
    lib.cp_ccl_instance_workspace_bytes.restype = C.c_size_t
    lib.cp_ccl_instance_workspace_bytes.argtypes = [C.c_int] * 5
    lib.cp_ccl_instance_labels.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4
    lib.cp_ls_vote_slots_f32.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    if hasattr(lib, "cp_ls_vote_slots_robust_f32"):
        raise SystemExit("%s exports cp_ls_vote_slots_robust_f32: it is not a build of the parent commit" % path)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_robust_vote.py needs a ROCm GPU: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    rec, lab = inputs(dev)
    new = _lib.load()
    old = bind_parent(args.parent_lib) if args.parent_lib else new
    st = torch.cuda.current_stream(dev).cuda_stream

    def ok(rc, what):
        if rc != 0:
            raise SystemExit("%s failed (%d)" % (what, rc))

    def labelling(lib):
        ws = torch.empty(lib.cp_ccl_instance_workspace_bytes(B, H, W, K - 1, R), dtype=torch.uint8, device=dev)
        slots, inst = torch.empty_like(lab), torch.empty(B, K - 1, R, 2, dtype=torch.int32, device=dev)

        def ccl():
            ok(lib.cp_ccl_instance_labels(lab.data_ptr(), B, H, W, K - 1, R, 50, ws.data_ptr(), slots.data_ptr(), inst.data_ptr(), st), "cp_ccl_instance_labels")
        return ccl, slots

    ccl_old, slots_old = labelling(old)
    sums_old, kp_old = torch.empty(B, SLOTS, KP, 5, dtype=torch.float64, device=dev), torch.empty(B, SLOTS, KP, 2, device=dev)

    def vote_old():
        ok(old.cp_ls_vote_slots_f32(rec.data_ptr(), 36, 9, 27, slots_old.data_ptr(), B, H, W, SLOTS, KP, 0, sums_old.data_ptr(), kp_old.data_ptr(), st),
           "cp_ls_vote_slots_f32")

    parent = "parent pair (%s)" % ("parent library" if args.parent_lib else "this library's unchanged entry points")
    pairs = {parent: (ccl_old, vote_old)}
    ccl_new, slots_new = labelling(new)
    outs = {}
    for p in PASSES:
        ws = torch.empty(new.cp_ls_vote_robust_workspace_bytes(B, SLOTS, KP), dtype=torch.uint8, device=dev)
        kps = torch.empty(B, SLOTS, KP, 2, device=dev)
        outs[p] = (ws, kps)

        def vote(p=p, ws=ws, kps=kps):
            _lib.check(new.cp_ls_vote_slots_robust_f32(rec.data_ptr(), 36, 9, 27, slots_new.data_ptr(), B, H, W, SLOTS, KP, 0, CUTOFF, p, ws.data_ptr(),
                                                       kps.data_ptr(), st), "cp_ls_vote_slots_robust_f32")

        pairs["robust voter, passes = %d" % p] = (ccl_new, vote)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3      # microseconds per call

    times = {name: ([], [], []) for name in pairs}
    for rep in range(args.repeats + 1):                       # round 0 is the warm-up
        for name, (ccl, vote) in pairs.items():               # alternated: every round times every pair
            t = (timed(ccl), timed(vote), timed(lambda: (ccl(), vote())))
            if rep:
                for k in range(3):
                    times[name][k].append(t[k])
    lines = ["probe_robust_vote: batch %d, %d x %d, 8 objects, R = %d (%d slots), record 36, ellipse masks (%.1f %% foreground), cut-off %g px; "
             "%d rounds of %d calls, us per call: median (min .. max)" % (B, H, W, R, SLOTS, 100.0 * float((lab > 0).float().mean()), CUTOFF, args.repeats, args.calls),
             "device: %s" % torch.cuda.get_device_name(dev)]
    for name, cols in times.items():
        lines.append("%-58s ccl %s   vote %s   both %s" % (name, *("%7.1f (%7.1f .. %7.1f)" % (np.median(c), min(c), max(c)) for c in cols)))
    base = np.median(times[parent][1])
    spread = max(times[parent][1]) - min(times[parent][1])
    v0 = np.median(times["robust voter, passes = 0"][1])
    lines.append("passes = 0 against the parent's voter: %+.1f us (the parent's own rounds spread over %.1f us)" % (v0 - base, spread))
    for p in PASSES[1:]:
        per = (np.median(times["robust voter, passes = %d" % p][1]) - v0) / p
        lines.append("a reweighted pass at passes = %d: %.1f us, %.2f x the parent's voter (%.1f us: one accumulate + solve)" % (p, per, per / base, base))
    # the same answer at passes = 0; what the passes move and keep on this input
    ccl_old(), vote_old(), ccl_new()
    for p in PASSES:
        pairs["robust voter, passes = %d" % p][1]()
    torch.cuda.synchronize(dev)
    lines.append("passes = 0 against the parent pair: slot maps equal %s, keypoints differ by at most %.3g px"
                 % (bool(torch.equal(slots_new, slots_old)), float((outs[0][1] - kp_old).abs().max())))
    for p in PASSES[1:]:
        s = outs[p][0].view(torch.float64).view(2, B, SLOTS, KP, 5)
        weight, kept = s[0, ..., 0] + s[0, ..., 2], s[1, ..., 0] + s[1, ..., 2]
        share = (kept / weight)[weight > 0]
        lines.append("passes = %d: keypoints move by at most %.3g px against passes = %d; share of the plain weight kept: median %.3f, least %.3f"
                     % (p, float((outs[p][1] - outs[p - 1][1]).abs().max()), p - 1, float(share.median()), float(share.min())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
