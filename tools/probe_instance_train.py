#!/usr/bin/env python3
"""What training on several instances of one object costs, at the bench shape: batch 32, 448 x 448, K = 9 classes, 9 keypoints, the production
record (36 floats per pixel in, the 64-float gradient row out).

    python tools/probe_instance_train.py [--parent-lib <libcasapose_hip.so of the parent commit>] [--out profiles/instance_train_probe.txt]

Loss: cp_pose_loss_f32 of this build against the parent commit's library (--parent-lib; without it this build stands in and the line says so),
and cp_pose_loss_inst_f32 at I = 1, 2, 4 without and with an instance map.  All variants are alternated inside every round: `--repeats` rounds of
`--calls` calls each between two device events, after a warm-up round of each.  The parent is timed TWICE per round (A and B): the distance between
its two medians, and each one's minimum and maximum over the rounds, are the run-to-run spread every other line is read against.  A line gives
the median, minimum and maximum over the rounds in microseconds per call and the ratio of its median to the parent's (A).
Scenes: DeviceScenes' kernels (the ray-caster, and for I > 1 the slot-label pass) on prepared records, 8 objects, I = 1 against I = 4.

    python tools/probe_instance_train.py --part outcome [--seconds S] [--out FILE (appended)]

Outcome, no threshold: casapose_c_gcu5 on ResNet-18, 2 objects, 224 x 288, batch 8, decoder 2 conditioned on the true labels, trained from one
initialisation for S seconds of steps each on (a) scenes with up to 2 instances per object under the map rule, (b) the same scenes under the
nearest-centre rule, (c) one-instance scenes, the control.  Then InstanceLSVoting (R = 2; the component split, and the vote split) over each
network's field on 64 held-out scenes in which object 1 and object 2 both show two instances, with the true labels as segmentation.  Found
slots are matched to the true instances by nearest centre (keypoint 0); an instance counts as found when a slot's centre lies within 10 px of
it and no nearer true instance claims that slot.  Reported per run: the loss over the run in ten parts, the share of true instances found and
the median keypoint error of the found ones, over all held-out scenes and over those where two instances of one object touch."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from casapose_amd import _lib  # noqa: E402

B, H, W, K, KP, LD, DLD, VERT_OFF = 32, 448, 448, 9, 9, 36, 64, 32
WEIGHTS = (1.0, 0.5, 0.015)


def bind_parent(path):
    lib = C.CDLL(path)
    if hasattr(lib, "cp_pose_loss_inst_f32"):
        raise SystemExit("%s exports cp_pose_loss_inst_f32: it is not a build of the parent commit" % path)
    lib.cp_pose_loss_f32.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float] * 3 + [C.c_void_p] * 2
                                     + [C.c_int] * 2 + [C.c_void_p] * 3)
    return lib


def inputs(dev, instances):
    g = torch.Generator(device="cpu").manual_seed(1237)
    lab = torch.zeros(B, H, W, dtype=torch.uint8)
    for o in range(K - 1):      # eight blocks of 100 x 100 pixels: 40 % foreground
        y0, x0 = 20 + 210 * (o // 4), 8 + 110 * (o % 4)
        lab[:, y0:y0 + 100, x0:x0 + 100] = o + 1
    rec = torch.randn(B, H, W, LD, generator=g)
    kpts = torch.rand(B, K - 1, instances, KP, 2, generator=g) * 448.0
    counts = torch.full((B, K - 1), instances, dtype=torch.int32)
    imap = torch.randint(0, instances, (B, H, W), generator=g, dtype=torch.uint8)
    return tuple(t.contiguous().to(dev) for t in (rec, lab, kpts, counts, imap))


def loss_variants(lib, parent, dev):
    st = lambda: torch.cuda.current_stream(dev).cuda_stream      # noqa: E731
    ws = torch.empty(lib.cp_pose_loss_inst_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    dout = torch.empty(B * H * W, DLD, device=dev)
    sums, vals = torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(B * (K - 1), device=dev)
    keep, variants = [], []
    rec, lab, kp1, _, _ = inputs(dev, 1)
    kp_flat = kp1.reshape(B, K - 1, KP, 2).contiguous()
    keep += [rec, lab, kp1, kp_flat]

    def old(which):
        def call():
            rc = which.cp_pose_loss_f32(rec.data_ptr(), LD, K, KP, lab.data_ptr(), lab.data_ptr(), kp_flat.data_ptr(), K - 1, B, H, W, 0, 0, *WEIGHTS, ws.data_ptr(),
                                        dout.data_ptr(), DLD, VERT_OFF, sums.data_ptr(), None, st())
            assert rc == 0
        return call

    variants += [("cp_pose_loss_f32, parent (A)", old(parent)), ("cp_pose_loss_f32, parent (B)", old(parent)), ("cp_pose_loss_f32, this build", old(lib))]
    for instances in (1, 2, 4):
        _, _, kpts, counts, imap = inputs(dev, instances)
        keep += [kpts, counts, imap]
        for with_map in (False, True):
            def call(kpts=kpts, counts=counts, imap=imap if with_map else None, instances=instances):
                _lib.check(lib.cp_pose_loss_inst_f32(rec.data_ptr(), LD, K, KP, lab.data_ptr(), lab.data_ptr(), kpts.data_ptr(), K - 1, instances, counts.data_ptr(),
                                                     imap.data_ptr() if imap is not None else None, B, H, W, 0, 0, *WEIGHTS, ws.data_ptr(), dout.data_ptr(), DLD,
                                                     VERT_OFF, sums.data_ptr(), None, st()), "cp_pose_loss_inst_f32")
            variants.append(("cp_pose_loss_inst_f32, I = %d, %s" % (instances, "map" if with_map else "nearest centre"), call))
    return variants, keep + [ws, dout, sums, vals]


def scene_variants(dev):
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

    variants, keep = [], []
    for instances in (1, 4):
        ds = SyntheticSceneDataset(K - 1, (H, W), length=64, seed=3, instances=instances)
        scenes = ds.device_scenes(dev)
        records = scenes.host_half(range(B))["records"].to(dev)
        keep += [ds, records]

        def call(scenes=scenes, records=records):
            scenes._render(records, True, dev, torch.cuda.current_stream(dev).cuda_stream)
        variants.append(("scene kernels, 8 objects, I = %d" % instances, call))
    return variants, keep


def measure(variants, dev, calls, repeats):
    times = {name: [] for name, _ in variants}
    for name, fn in variants:      # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    for _ in range(repeats):
        for name, fn in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1000.0 / calls)
    return {name: (float(np.median(t)), min(t), max(t)) for name, t in times.items()}


# ---- outcome ------------------------------------------------------------------------------------------------------------------------
OH, OW, OBS, OOC = 224, 288, 8, 2


def train_run(dev, instances, rule, seconds):
    import time
    from types import SimpleNamespace

    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.training import Adam, train_step
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler, PiecewiseConstantDecay

    os.environ["CASAPOSE_TRAIN_INSTANCE_RULE"] = rule
    k = OOC + 1
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=k, input_shape=(OH, OW, 3), input_segmentation_shape=(OH, OW, k), weights=None,
                                             base_model="resnet18", device=dev, seed=3)
    ds = SyntheticSceneDataset(OOC, (OH, OW), length=1 << 30, seed=100, instances=instances)
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=False, max_keypoint_pixel_error=12.5, confidence_regularization=False,
                          use_bpnp_reprojection_loss=False)
    lf = LossWeightHandler(1.0, 0.5, 0.015, 0.0, filter_vertex_with_segmentation=True)
    optim = Adam(learning_rate=PiecewiseConstantDecay([1 << 30], [1e-3, 1e-3]))
    hist, t0, i, said = [], time.time(), 0, 0.0
    while time.time() - t0 < seconds:
        hist.append(train_step(net, ds.batch(i, OBS, device=dev), lf, optim, opt))
        i += 1
        if time.time() - t0 - said >= 30.0:      # a sign of life for whoever watches the log
            said = time.time() - t0
            print("  ... %d steps, loss %.4g" % (i, hist[-1][0]), flush=True)
    return net, np.array(hist)


def held_out(dev, wanted=64):
    """two-instance scenes the training streams never drew: both objects show two instances with at least 300 pixels each"""
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

    ds = SyntheticSceneDataset(OOC, (OH, OW), length=1 << 30, seed=977, instances=2)
    kept, i = [], 0
    while len(kept) < wanted:
        bt = ds.batch(i, 1)
        i += 1
        lab, iseg = bt["filtered_seg"][0, ..., 0].numpy(), bt["instance_seg"][0].numpy()
        sizes = [((lab == o + 1) & (iseg == r)).sum() for o in range(OOC) for r in range(2)]
        if bt["instance_count"].min() == 2 and min(sizes) >= 300:
            touch = False
            for o in range(OOC):
                a, b = (lab == o + 1) & (iseg == 0), (lab == o + 1) & (iseg == 1)
                touch |= bool((a[1:] & b[:-1]).any() or (a[:-1] & b[1:]).any() or (a[:, 1:] & b[:, :-1]).any() or (a[:, :-1] & b[:, 1:]).any())
            kept.append((bt, touch))
    return kept


def evaluate(net, scenes, dev, split):
    from casapose_amd.pose_estimation.instance_voting import InstanceLSVoting

    k = OOC + 1
    voter = InstanceLSVoting("probe_votes", k, 9, max_instances=2, split=split)
    rows = []      # (touching, found, median keypoint error of the instance)
    for bt, touch in scenes:
        img, seg = bt["img"].to(dev), bt["target_seg"].to(dev)
        out = net([img, seg], training=False)
        dirs, conf = out[..., k:k + 18].contiguous(), out[..., k + 18:k + 27].contiguous()
        coords = voter([(10.0 * seg).contiguous(), dirs, conf]).cpu().numpy()[0]          # [oc, R, kp, 2]
        counts = voter.last_counts.cpu().numpy()[0]
        gt = bt["target_vert"][0].numpy()
        for o in range(OOC):
            slots = [r for r in range(2) if counts[o, r] > 0 and np.isfinite(coords[o, r]).all()]
            for r in range(2):
                best, err = None, np.inf
                for s_ in slots:
                    d = np.linalg.norm(coords[o, s_, 0] - gt[o, r, 0])
                    other = np.linalg.norm(coords[o, s_, 0] - gt[o, 1 - r, 0])
                    if d < 10.0 and d <= other and d < err:
                        best, err = s_, d
                rows.append((touch, best is not None, float(np.median(np.linalg.norm(coords[o, best] - gt[o, r], axis=-1))) if best is not None else np.nan))
    return rows


def outcome(dev, seconds, out_path):
    lines = ["outcome: casapose_c_gcu5 / ResNet-18, %d objects, %d x %d, batch %d, Adam 1e-3, %d s of steps per run, one initialisation; held-out: 64 scenes with "
             "two instances of both objects" % (OOC, OH, OW, OBS, seconds)]
    scenes = held_out(dev)
    lines.append("held-out scenes in which two instances of one object touch: %d of %d" % (sum(t for _, t in scenes), len(scenes)))
    for name, instances, rule in (("instances = 2, map rule", 2, "map"), ("instances = 2, nearest-centre rule", 2, "nearest"), ("instances = 1 (control)", 1, "map")):
        net, hist = train_run(dev, instances, rule, seconds)
        parts = np.array_split(hist, 10)
        lines.append("%s: %d steps" % (name, len(hist)))
        for col, what in ((0, "loss"), (2, "vertex"), (3, "proxy")):
            lines.append("    %-7s %s" % (what, " ".join("%.4g" % p[:, col].mean() for p in parts if len(p))))
        for split in ("components", "votes"):
            rows = evaluate(net, scenes, dev, split)
            for label, sel in (("all scenes", [r for r in rows]), ("touching", [r for r in rows if r[0]]), ("apart", [r for r in rows if not r[0]])):
                found = [r for r in sel if r[1]]
                lines.append("    split = %-10s %-10s found %3d of %3d true instances (%.1f %%), median keypoint error of the found %.2f px"
                             % (split, label, len(found), len(sel), 100.0 * len(found) / max(len(sel), 1), float(np.median([r[2] for r in found])) if found else float("nan")))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("timing", "outcome"), default="timing")
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_instance_train.py measures on a ROCm GPU; there is none")
    dev = torch.device("cuda:0")
    if a.part == "outcome":
        return outcome(dev, a.seconds, a.out)
    lib = _lib.load()
    parent = bind_parent(a.parent_lib) if a.parent_lib else lib
    lines = ["pose loss, batch %d, %d x %d, K = %d, kp = %d, record %d floats, gradient row %d floats; %d rounds of %d calls, microseconds per call"
             % (B, H, W, K, KP, LD, DLD, a.repeats, a.calls),
             "parent library: %s" % ("a build of the parent commit" if a.parent_lib else "NOT GIVEN -- this build stands in for it")]
    variants, keep = loss_variants(lib, parent, dev)
    res = measure(variants, dev, a.calls, a.repeats)
    base = res["cp_pose_loss_f32, parent (A)"][0]
    bytes_moved = B * H * W * (LD + DLD) * 4.0
    for name, _ in variants:
        med, lo, hi = res[name]
        lines.append("  %-48s median %8.1f  min %8.1f  max %8.1f  x%.3f of the parent  (%.2f TB/s of record + gradient row)"
                     % (name, med, lo, hi, med / base, bytes_moved / med / 1e6))
    svariants, skeep = scene_variants(dev)
    sres = measure(svariants, dev, max(a.calls // 4, 1), a.repeats)
    lines.append("scene kernels, batch %d, %d x %d, microseconds per batch" % (B, H, W))
    sbase = sres[svariants[0][0]][0]
    for name, _ in svariants:
        med, lo, hi = sres[name]
        lines.append("  %-48s median %8.1f  min %8.1f  max %8.1f  x%.3f of I = 1" % (name, med, lo, hi, med / sbase))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
