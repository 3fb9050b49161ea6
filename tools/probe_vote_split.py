#!/usr/bin/env python3
"""Splitting instances by centre votes (cp_vote_split_labels + cp_ls_vote_slots_f32) against splitting them by components
(cp_ccl_instance_labels + cp_ls_vote_slots_f32), at the bench shape: batch 16, 480 x 640, 8 objects, the production record, the ellipse masks of
`bench.py --mode vote` (tools/probe_instance_vote.py builds them), keypoint 0 of every object pointing at its ellipse's centre with 0.05 rad of
noise, R = 4.

    python tools/probe_vote_split.py [--parent-lib <libcasapose_hip.so of the parent commit>] [--out profiles/vote_split_probe.txt]

Component pair: with --parent-lib both entry points are called in that library (a build of the commit before cp_vote_split_labels); without it in
this tree's library, where they are the same code.  Vote pair at vote_stride 1 and 2 with the defaults otherwise (cell 4, min_votes 12,
rel_percent 25, nms_radius 2, gate 4, min_size 50).  The three are alternated inside every repeat: `--repeats` rounds of `--calls` calls each
between two device events, after a warm-up round of each; a line gives the median, the minimum and the maximum over the rounds, per call, of
the labelling, of the voter, and of both.  The kernels of cp_vote_split_labels apart from each other come from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/probe_vote_split.py --repeats 1 --calls 20 --strides 1, and again with --strides 2)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from casapose_amd import _lib  # noqa: E402
from probe_instance_vote import B, H, K, KP, W, inputs  # noqa: E402

R = 4
PARAMS = dict(cell=4, min_votes=12, rel_percent=25, nms_radius=2, gate=4.0, min_size=50)


def centre_field(rec, dev):
    """keypoint 0 of the record's directions: towards the ellipse's centre, 0.05 rad of noise"""
    g = torch.Generator(device="cpu").manual_seed(4711)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5, torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
    d0 = torch.zeros(B, H, W, 2)
    for o in range(K - 1):
        cy, cx = H * (0.25 + 0.5 * (o // 4)), W * (0.125 + 0.25 * (o % 4))
        m = ((yy - cy) / (H * 0.2)) ** 2 + ((xx - cx) / (W * 0.1)) ** 2 <= 1.0
        ang = torch.atan2(cy - yy[m], cx - xx[m])[None] + 0.05 * torch.randn(B, int(m.sum()), generator=g)
        d0[:, m] = torch.stack([torch.sin(ang), torch.cos(ang)], -1)
    rec[..., 9:11] = d0.to(dev)
    return rec


def bind_parent(path):
    lib = C.CDLL(path)
    lib.cp_ccl_instance_workspace_bytes.restype = C.c_size_t
    lib.cp_ccl_instance_workspace_bytes.argtypes = [C.c_int] * 5
    lib.cp_ccl_instance_labels.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4
    lib.cp_ls_vote_slots_f32.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    if hasattr(lib, "cp_vote_split_labels"):
        raise SystemExit("%s exports cp_vote_split_labels: it is not a build of the parent commit" % path)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--strides", default="1,2", help="the vote strides to time, e.g. 1 for a kernel trace of one of them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_vote_split.py needs a ROCm GPU: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    rec, lab = inputs(dev)
    rec = centre_field(rec, dev)
    new = _lib.load()
    old = bind_parent(args.parent_lib) if args.parent_lib else new
    st = torch.cuda.current_stream(dev).cuda_stream
    slots_n = 8 * R

    def ok(rc, what):
        if rc != 0:
            raise SystemExit("%s failed (%d)" % (what, rc))

    ws_c = torch.empty(old.cp_ccl_instance_workspace_bytes(B, H, W, K - 1, R), dtype=torch.uint8, device=dev)
    slots_c, inst_c = torch.empty_like(lab), torch.empty(B, K - 1, R, 2, dtype=torch.int32, device=dev)
    sums_c = torch.empty(B, slots_n, KP, 5, dtype=torch.float64, device=dev)
    kps_c = torch.empty(B, slots_n, KP, 2, device=dev)

    def comp_label():
        ok(old.cp_ccl_instance_labels(lab.data_ptr(), B, H, W, K - 1, R, 50, ws_c.data_ptr(), slots_c.data_ptr(), inst_c.data_ptr(), st),
           "cp_ccl_instance_labels")

    def comp_vote():
        ok(old.cp_ls_vote_slots_f32(rec.data_ptr(), 36, 9, 27, slots_c.data_ptr(), B, H, W, slots_n, KP, 0, sums_c.data_ptr(), kps_c.data_ptr(), st),
           "cp_ls_vote_slots_f32")

    pairs = {"components (%s)" % ("parent library" if args.parent_lib else "this library's unchanged entry points"): (comp_label, comp_vote)}
    outs = {}
    strides = [int(v) for v in args.strides.split(",")]
    for stride in strides:
        ws = torch.empty(new.cp_vote_split_workspace_bytes(B, H, W, K - 1, R, PARAMS["cell"]), dtype=torch.uint8, device=dev)
        slots, inst = torch.empty_like(lab), torch.empty(B, K - 1, R, 4, dtype=torch.int32, device=dev)
        peaks = torch.empty(B, K - 1, R, 2, device=dev)
        sums = torch.empty(B, slots_n, KP, 5, dtype=torch.float64, device=dev)
        kps = torch.empty(B, slots_n, KP, 2, device=dev)
        outs[stride] = (slots, inst, kps)

        def label(stride=stride, ws=ws, slots=slots, inst=inst, peaks=peaks):
            _lib.check(new.cp_vote_split_labels(lab.data_ptr(), rec.data_ptr(), 36, 9, 0, B, H, W, K - 1, R, PARAMS["cell"], stride, PARAMS["min_votes"],
                                                PARAMS["rel_percent"], PARAMS["nms_radius"], PARAMS["gate"], PARAMS["min_size"], ws.data_ptr(),
                                                slots.data_ptr(), inst.data_ptr(), peaks.data_ptr(), st), "cp_vote_split_labels")

        def vote(slots=slots, sums=sums, kps=kps):
            _lib.check(new.cp_ls_vote_slots_f32(rec.data_ptr(), 36, 9, 27, slots.data_ptr(), B, H, W, slots_n, KP, 0, sums.data_ptr(), kps.data_ptr(), st),
                       "cp_ls_vote_slots_f32")

        pairs["centre votes, vote_stride %d" % stride] = (label, vote)

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
        for name, (label, vote) in pairs.items():             # alternated: every round times every pair
            t = (timed(label), timed(vote), timed(lambda: (label(), vote())))
            if rep:
                for k in range(3):
                    times[name][k].append(t[k])
    lines = ["probe_vote_split: batch %d, %d x %d, 8 objects, record 36, ellipse masks (%.1f %% foreground), R = %d; %d rounds of %d calls, us per call: "
             "median (min .. max)" % (B, H, W, 100.0 * float((lab > 0).float().mean()), R, args.repeats, args.calls),
             "device: %s" % torch.cuda.get_device_name(dev)]
    for name, cols in times.items():
        lines.append("%-44s label %s   vote %s   both %s" % (name, *("%8.1f (%8.1f .. %8.1f)" % (np.median(c), min(c), max(c)) for c in cols)))
    base = np.median(next(iter(times.values()))[2])
    for name, cols in list(times.items())[1:]:
        lines.append("%s: %.2f times the component pair" % (name, np.median(cols[2]) / base))
    # the same answer on these masks: one ellipse per object, so both rules find one instance of every object with all of its pixels
    torch.cuda.synchronize(dev)
    for stride in strides:
        slots, inst, kps = outs[stride]
        lines.append("vote_stride %d: instances per (image, object) %d .. %d, pixels equal the components' %s, slot maps equal %s, keypoints differ by at "
                     "most %.3g px" % (stride, int((inst[..., 0] > 0).sum(-1).min()), int((inst[..., 0] > 0).sum(-1).max()),
                                       bool(torch.equal(inst[..., 0], inst_c[..., 0])), bool(torch.equal(slots, slots_c)), float((kps - kps_c).abs().max())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
