#!/usr/bin/env python3
"""What the LS voter has to read on the benchmark batch, and how long it takes.

Builds the network and the batch exactly as `bench.py` does (seed 1237, randomised normalisation statistics), runs one forward, the arg-max
and the component filter, and reports for the filtered label map the voter is given:
  * the fraction of non-zero (kept) pixels,
  * the fraction of 64-pixel row segments (64 columns x 1 row of a 64 x 16 strip) that hold a kept pixel -- the segments whose records
    the voter requests,
  * the bytes per image that makes (segments x 64 x 144 B records + the label map), beside the H*W*144 B of reading every record.
Then times cp_ls_vote_f32 (memset + accumulation + solve) with HIP events on that batch, and on a batch in which every pixel is kept
(`all_kept`: the dense case, every row segment read).  One JSON line.

    python tools/voter_kept_fraction.py [--batch 16 --height 480 --width 640 --iters 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()

    import numpy as np
    import torch

    from casapose_amd import _lib, ops
    from casapose_amd.pose_models.tfkeras import Classifiers

    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    seg_dim, ver_dim, kp = 9, 27, 9
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=ver_dim, seg_dim=seg_dim, input_shape=(H, W, 3), weights=None, base_model="resnet18", device=dev, seed=1237)
    rng = np.random.default_rng(1237)
    params = net.get_parameters()
    for k, v in params.items():
        if k.endswith(".gamma") or k.endswith(".moving_variance"):
            params[k] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif k.endswith(".beta") or k.endswith(".moving_mean"):
            params[k] = (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    net.set_parameters(params)
    gen = torch.Generator(device="cpu").manual_seed(1237)
    img = (2.0 * torch.rand(B, H, W, 3, generator=gen) - 1.0).to(dev)
    out = net([img], training=False).clone()

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    lab0 = ops.argmax_labels(out, classes=seg_dim)
    ws = torch.empty(lib.cp_ccl_workspace_bytes(B, H, W, seg_dim - 1), dtype=torch.uint8, device=dev)
    labels = torch.empty_like(lab0)
    _lib.check(lib.cp_ccl_filter_labels(lab0.data_ptr(), B, H, W, seg_dim - 1, 50, 1, ws.data_ptr(), labels.data_ptr(), stream), "cp_ccl_filter_labels")

    def segments(lab):
        """fraction of (row, 64-column strip) segments with a non-zero label, per image"""
        pad = (-W) % 64
        nz = torch.nn.functional.pad(lab != 0, (0, pad))
        return nz.reshape(B, H, -1, 64).any(-1).float().mean((1, 2))

    def timed(rec, lab):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            ops.ls_vote(rec, 0, seg_dim, seg_dim + 2 * kp, seg_dim - 1, kp, labels=lab)
        runs = []
        for _ in range(5):   # five groups: their spread is the run-to-run noise of this figure
            e0.record()
            for _ in range(args.iters):
                ops.ls_vote(rec, 0, seg_dim, seg_dim + 2 * kp, seg_dim - 1, kp, labels=lab)
            e1.record()
            e1.synchronize()
            runs.append(round(1e3 * e0.elapsed_time(e1) / args.iters, 2))
        return runs

    fg = (lab0 != 0).float().mean((1, 2))
    kept = (labels != 0).float().mean((1, 2))
    seg = segments(labels)
    nseg = H * ((W + 63) // 64)
    bytes_now = seg * nseg * 64 * 144 + H * W
    result = {
        "batch": B, "height": H, "width": W,
        "foreground_fraction_mean": round(float(fg.mean()), 5),
        "kept_pixel_fraction": {"mean": round(float(kept.mean()), 5), "min": round(float(kept.min()), 5), "max": round(float(kept.max()), 5)},
        "row_segments_read_fraction": {"mean": round(float(seg.mean()), 5), "min": round(float(seg.min()), 5), "max": round(float(seg.max()), 5)},
        "voter_bytes_per_image": {"now_mean": int(bytes_now.mean()), "every_record": H * W * 144},
        "ls_vote_us_bench_batch": timed(out, labels),
    }
    # the dense case: every pixel kept (eight vertical bands), the same records
    dense = (1 + (torch.arange(W, device=dev) * 8 // W)).to(torch.uint8)[None, None, :].expand(B, H, W).contiguous()
    result["ls_vote_us_all_kept"] = timed(out, dense)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
