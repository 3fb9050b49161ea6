#!/usr/bin/env python3
"""The component filter and the LS voter for one instance per object against the pair for several (cp_ccl_instance_labels +
cp_ls_vote_slots_f32), at the bench shape: batch 16, 480 x 640, 8 objects, the production record, the ellipse masks of `bench.py --mode vote`.

    python tools/probe_instance_vote.py [--parent-lib <libcasapose_hip.so of the parent commit>] [--out profiles/instance_vote_probe.txt]

Parent pair: cp_ccl_filter_labels(rank 1) + cp_ls_vote_w_f32 with the filtered labels.  With --parent-lib both are called in that library (a build
of the commit before the instance entry points); without it in this tree's library, whose two entry points are the same code.  New pair at R = 1
and R = 4.  The three are alternated inside every repeat: `--repeats` rounds of `--calls` calls each between two device events, after a warm-up
round of each; the line of a pair gives the median, the minimum and the maximum over the rounds, per call of CCL, of the voter, and of both.
The new pair at R = 1 is also compared with the parent pair on the same input (keypoints of the 8 objects)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from casapose_amd import _lib  # noqa: E402

B, H, W, K, KP = 16, 480, 640, 9, 9


def inputs(dev):
    """bench_vote's inputs: 8 elliptical masks, the exact unit field towards random keypoints + N(0, 0.05 rad), confidences N(0, 1)"""
    g = torch.Generator(device="cpu").manual_seed(1237)
    lab = torch.zeros(B, H, W, dtype=torch.long)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32) + 0.5, torch.arange(W, dtype=torch.float32) + 0.5, indexing="ij")
    direct = torch.zeros(B, H, W, KP, 2)
    for o in range(K - 1):
        cy, cx = H * (0.25 + 0.5 * (o // 4)), W * (0.125 + 0.25 * (o % 4))
        ry, rx = H * 0.2, W * 0.1
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        lab[:, m] = o + 1
        kp = torch.stack([cy + ry * (2 * torch.rand(B, KP, generator=g) - 1), cx + rx * (2 * torch.rand(B, KP, generator=g) - 1)], -1)
        d = kp[:, None, :, :] - torch.stack([yy[m], xx[m]], -1)[None, :, None, :]
        ang = torch.atan2(d[..., 0], d[..., 1]) + 0.05 * torch.randn(d.shape[:-1], generator=g)
        direct[:, m] = torch.stack([torch.sin(ang), torch.cos(ang)], -1)
    seg = 10.0 * torch.nn.functional.one_hot(lab, K).float()
    conf = torch.randn(B, H, W, KP, generator=g)
    rec = torch.cat([seg, direct.reshape(B, H, W, 2 * KP), conf], 3).contiguous().to(dev)
    return rec, lab.to(torch.uint8).to(dev)


def bind_parent(path):
    lib = C.CDLL(path)
    lib.cp_ccl_workspace_bytes.restype = C.c_size_t
    lib.cp_ccl_workspace_bytes.argtypes = [C.c_int] * 4
    lib.cp_ccl_filter_labels.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    lib.cp_ls_vote_w_f32.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    for name in ("cp_ccl_instance_labels", "cp_ls_vote_slots_f32"):
        if hasattr(lib, name):
            raise SystemExit("%s exports %s: it is not a build of the parent commit" % (path, name))
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_instance_vote.py needs a ROCm GPU: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    rec, lab = inputs(dev)
    new = _lib.load()
    old = bind_parent(args.parent_lib) if args.parent_lib else new
    st = torch.cuda.current_stream(dev).cuda_stream
    ws_old = torch.empty(old.cp_ccl_workspace_bytes(B, H, W, K - 1), dtype=torch.uint8, device=dev)
    kept = torch.empty_like(lab)
    sums8, kp8 = torch.empty(B, 8, KP, 5, dtype=torch.float64, device=dev), torch.empty(B, 8, KP, 2, device=dev)

    def ok(rc, what):
        if rc != 0:
            raise SystemExit("%s failed (%d)" % (what, rc))

    def parent_ccl():
        ok(old.cp_ccl_filter_labels(lab.data_ptr(), B, H, W, K - 1, 50, 1, ws_old.data_ptr(), kept.data_ptr(), st), "cp_ccl_filter_labels")

    def parent_vote():
        ok(old.cp_ls_vote_w_f32(rec.data_ptr(), 36, 0, 9, 27, kept.data_ptr(), B, H, W, K - 1, KP, 0, sums8.data_ptr(), kp8.data_ptr(), st), "cp_ls_vote_w_f32")

    pairs = {"parent pair (%s)" % ("parent library" if args.parent_lib else "this library's unchanged entry points"): (parent_ccl, parent_vote)}
    outs = {}
    for r in (1, 4):
        ws = torch.empty(new.cp_ccl_instance_workspace_bytes(B, H, W, K - 1, r), dtype=torch.uint8, device=dev)
        slots, inst = torch.empty_like(lab), torch.empty(B, K - 1, r, 2, dtype=torch.int32, device=dev)
        sums = torch.empty(B, 8 * r, KP, 5, dtype=torch.float64, device=dev)
        kps = torch.empty(B, 8 * r, KP, 2, device=dev)
        outs[r] = (slots, inst, kps)

        def ccl(r=r, ws=ws, slots=slots, inst=inst):
            _lib.check(new.cp_ccl_instance_labels(lab.data_ptr(), B, H, W, K - 1, r, 50, ws.data_ptr(), slots.data_ptr(), inst.data_ptr(), st),
                       "cp_ccl_instance_labels")

        def vote(r=r, slots=slots, sums=sums, kps=kps):
            _lib.check(new.cp_ls_vote_slots_f32(rec.data_ptr(), 36, 9, 27, slots.data_ptr(), B, H, W, 8 * r, KP, 0, sums.data_ptr(), kps.data_ptr(), st),
                       "cp_ls_vote_slots_f32")

        pairs["new pair, R = %d (%d slots)" % (r, 8 * r)] = (ccl, vote)

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
    lines = ["probe_instance_vote: batch %d, %d x %d, 8 objects, record 36, ellipse masks (%.1f %% foreground); %d rounds of %d calls, us per call: "
             "median (min .. max)" % (B, H, W, 100.0 * float((lab > 0).float().mean()), args.repeats, args.calls),
             "device: %s" % torch.cuda.get_device_name(dev)]
    for name, cols in times.items():
        lines.append("%-58s ccl %s   vote %s   both %s" % (name, *("%7.1f (%7.1f .. %7.1f)" % (np.median(c), min(c), max(c)) for c in cols)))
    # the same answer: R = 1 keeps the largest component of every ellipse, as the filter does on these masks
    parent_ccl(), parent_vote()
    pairs["new pair, R = 1 (8 slots)"][0](), pairs["new pair, R = 1 (8 slots)"][1]()
    torch.cuda.synchronize(dev)
    lines.append("R = 1 against the parent pair: label maps equal %s, keypoints differ by at most %.3g px"
                 % (bool(torch.equal(outs[1][0], kept)), float((outs[1][2] - kp8).abs().max())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
