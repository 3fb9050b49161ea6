#!/usr/bin/env python3
"""Copy ONE run's profile artefacts from gpurun_out/<tag>/ (written by tools/profile_round.sh on the GPU box) into profiles/<tag>_*, stamp them
(profiles/<tag>_STAMP.json: the source / binary stamp of `python bench.py --stamp`, git HEAD, file list) and regenerate profiles/<tag>_summary.md.
Refuses a set whose stamp changed during the run or differs from the working tree's (round-2 verdict: stale PMC files next to a newer binary).
usage: python tools/make_summary.py [tag]"""
import csv
import json
import os
import shutil
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
G, P = os.path.join(R, "gpurun_out"), os.path.join(R, "profiles")
HISTORY_R01 = ("History of this round (images/s): 332 -> 600 (direct kernels: producer/consumer implicit GEMM, halo tiles, fused heads), -> 852 (Winograd "
           "F(4x4,3x3) for the nine deep 3x3 layers), -> 887 (persistent cross-tile pipelined GEMM for the Winograd planes), -> 916 (vectorised arg-max), "
           "-> 926 (partial-conv tap masks once per tile), -> 971-975 (halo kernel: transposed accumulators = lane per pixel, 16-byte epilogue accesses, "
           "register-resident fused head, deeper weight ring for the 32-channel layers), -> 980 (prefetching LS voting kernel), -> 988-997 (LDS-halo stem kernel; "
           "boxes differ by about 1 %).")
TRAIN_HISTORY_R01 = ("257 images/s with direct kernels only; 308 with Winograd forward + data gradient; 358 with the Winograd weight gradient; 379-382 with the "
                 "vectorised loss kernel; 400 with the Winograd GEMMs on the split-bf16 kernel (training default) and the single-gather weight refresh")


def copy(src, dst):
    if os.path.exists(os.path.join(G, src)):
        shutil.copyfile(os.path.join(G, src), os.path.join(P, dst))
        COPIED.append(dst)
        return True
    print("missing", src)
    return False


def stats_table(path, rows=24, width=70):
    out = ["| kernel | calls | total ms | avg us | % |", "|---|---|---|---|---|"]
    for i, r in enumerate(csv.DictReader(open(path))):
        if i >= rows:
            break
        name = r["Name"].replace("(anonymous namespace)::", "")[:width]
        out.append("| `%s` | %s | %.3f | %.1f | %.1f |" % (name, r["Calls"], float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3, float(r["Percentage"])))
    return "\n".join(out)


# ---- one stamp for the whole set: every file of profiles/<tag>_* comes from ONE run of tools/profile_round.sh on ONE source tree ----------------
COPIED = []
T = "%s/" % tag
stamp_path = os.path.join(G, tag, "stamp.json")
if not os.path.exists(stamp_path):
    sys.exit("no %s: run `gpurun -- bash tools/profile_round.sh %s` first" % (stamp_path, tag))
stamp, stamp_end = json.load(open(stamp_path)), json.load(open(os.path.join(G, tag, "stamp_end.json")))
if stamp != stamp_end:
    sys.exit("the tree changed while the profile set was being produced (%s vs %s): refusing to summarise mixed stamps" % (stamp, stamp_end))
import subprocess  # noqa: E402

here = json.loads(subprocess.run([sys.executable, os.path.join(R, "bench.py"), "--stamp"], capture_output=True, text=True, check=True).stdout)
if here["src_sha256"] != stamp["src_sha256"]:
    sys.exit("profiles in gpurun_out/%s were measured on source stamp %s, the working tree is %s: re-run tools/profile_round.sh on this tree "
             "(the bench line would refuse their PMC traffic anyway)" % (tag, stamp["src_sha256"], here["src_sha256"]))
# nothing of an earlier stamp survives under this tag -- FILES of the standard set only: profiles/probes/ (tools/probes_round.sh, one-off probe outputs
# DESIGN.md cites, each with its own stamp line) is a directory and is never touched (round-4 verdict, weak #7)
for old in [f for f in os.listdir(P) if f.startswith(tag + "_") and os.path.isfile(os.path.join(P, f))]:
    os.remove(os.path.join(P, old))
copy(T + "bench.json", "%s_bench.json" % tag)
copy(T + "bench_bs32.json", "%s_bench_bs32.json" % tag)
copy(T + "bench_f32.json", "%s_bench_infer_f32.json" % tag)
copy(T + "bench_split.json", "%s_bench_infer_split.json" % tag)
copy(T + "bench_bf16.json", "%s_bench_infer_bf16.json" % tag)
copy(T + "bench_profiled.json", "%s_bench_profiled.json" % tag)
copy(T + "trace/bench_kernel_stats.csv", "%s_bench_kernel_stats.csv" % tag)
copy(T + "layer_times.txt", "%s_layer_times.txt" % tag)
copy(T + "layer_times_f32.txt", "%s_layer_times_conv_mode_f32.txt" % tag)
copy(T + "layer_times_split.txt", "%s_layer_times_conv_mode_split.txt" % tag)
copy(T + "pmc_traffic/traffic.json", "%s_pmc_traffic.json" % tag)
copy(T + "pmc_traffic/summary.txt", "%s_pmc_traffic.txt" % tag)
copy(T + "pmc_mfma/summary.txt", "%s_pmc_mfma.txt" % tag)
copy(T + "bench_train.json", "%s_bench_train.json" % tag)
copy(T + "bench_train_f32.json", "%s_bench_train_conv_mode_f32.json" % tag)
copy(T + "bench_train_bf16.json", "%s_bench_train_conv_mode_bf16.json" % tag)
copy(T + "bench_train_exact.json", "%s_bench_train_exact.json" % tag)
copy(T + "train_trace/train_kernel_stats.csv", "%s_train_kernel_stats.csv" % tag)
copy(T + "train_times.txt", "%s_train_times.txt" % tag)
copy(T + "bench_vote.json", "%s_bench_vote.json" % tag)
copy(T + "vote_trace/vote_kernel_stats.csv", "%s_vote_kernel_stats.csv" % tag)
# GPU suite logs written next to the profile set (tools/profile_round.sh <tag> suites): only those of the SAME tree -- gpurun merges files into
# gpurun_out/ without deleting older ones, so logs of an earlier tree can still lie there (gputests_stamp.json says which tree they belong to)
gst = os.path.join(G, tag, "gputests_stamp.json")
same_tree = os.path.exists(gst) and json.load(open(gst)).get("src_sha256") == stamp["src_sha256"]
for extra in sorted(os.listdir(os.path.join(G, tag))):
    if extra.startswith("gputests_") and extra.endswith(".log"):
        if same_tree:
            copy(T + extra, "%s_%s" % (tag, extra))
        else:
            stale = os.path.join(P, "%s_%s" % (tag, extra))
            if os.path.exists(stale):
                os.remove(stale)
            print("skipped %s: written on another source tree" % extra)
git_head = subprocess.run(["git", "-C", R, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
dirty = bool(subprocess.run(["git", "-C", R, "status", "--porcelain", "--", "casapose_amd", "include", "bench.py"], capture_output=True, text=True).stdout.strip())
json.dump({"tag": tag, "stamp": stamp, "git_head_when_summarised": git_head, "tracked_sources_dirty": dirty,
           "what": "every profiles/%s_* file listed here was produced by ONE run of tools/profile_round.sh on the source tree identified by "
                   "stamp.src_sha256 (sha256 over casapose_amd/csrc, include/, the engine files and bench.py: `python bench.py --stamp`); bench.py "
                   "quotes PMC traffic only from a profile whose stamp equals the running tree's" % tag,
           "files": sorted(COPIED)}, open(os.path.join(P, "%s_STAMP.json" % tag), "w"), indent=1)


def load(name):
    p = os.path.join(P, "%s_%s" % (tag, name))
    if not os.path.exists(p):
        return None
    return json.loads(open(p).read().strip().splitlines()[-1])


def tests_line(name):
    p = os.path.join(P, "%s_%s" % (tag, name))
    if not os.path.exists(p):
        return None
    lines = [l for l in open(p).read().strip().splitlines() if " passed" in l or " failed" in l]
    return lines[-1].strip("= ") if lines else None


b, t = load("bench.json"), load("bench_train.json")
rf, dom, wg = b["roofline"], b["roofline"]["dominant_family"], b["roofline"]["winograd"]
# bench.json is produced BEFORE the PMC passes of the same run, so its `traffic` was looked up in the PREVIOUS round's committed profile (and
# refused for its other stamp).  The PMC files of THIS run have been copied and stamped above: look the dominant family up again, the way the
# next `python bench.py` on this tree will (round-3 verdict: the summary said "not quoted" while the driver's line quoted it).
sys.path.insert(0, R)
import bench as _bench  # noqa: E402

_tile = next((k for k, v in _bench.TILE_NAMES.items() if v == dom["kernel"]), None)
if _tile is not None:
    _traffic, _src = _bench.measured_traffic(_tile)
    if _traffic is not None:
        rf["traffic"], rf["traffic_source"] = _traffic, _src
md = ["# Round %s profile summary (MI355X)\n" % tag[1:].lstrip("0")]
md.append("Generated by `python tools/make_summary.py {0}` from ONE run of `tools/profile_round.sh {0}` on the GPU box (`gpurun_out/{0}/`); source stamp "
          "`{1}` (`python bench.py --stamp`; `profiles/{0}_STAMP.json` lists the files) -- the generator refuses a set whose stamp differs from the working "
          "tree's.  Files: `bench.json` (`python bench.py --steps 20 --warmup 5 --full`, un-profiled), `bench_bs32.json`, `bench_infer_f32.json` / "
          "`bench_infer_bf16.json` (the other conv modes), `bench_profiled.json` + `bench_kernel_stats.csv` (`rocprofv3 --kernel-trace --stats`), "
          "`layer_times*.txt` (`tools/layer_times.py`), `pmc_traffic.{{json,txt}}` (FETCH_SIZE and WRITE_SIZE in separate `--pmc` passes, FETCH doubled as the "
          "microarchitecture guide prescribes for gfx950), `pmc_mfma.txt` (SQ MFMA-busy counters, per-dispatch join), `bench_train*.json` + "
          "`train_kernel_stats.csv` + `train_times.txt`, `bench_vote.json` + `vote_kernel_stats.csv`, `gputests_*.log` (the `-m gpu` suite per conv mode).\n".format(tag, stamp["src_sha256"]))
md.append("## Inference (BASELINE configs[1]: bs 16, 480x640, K = 9)\n")
bs32 = load("bench_bs32.json")
pp = rf["per_pipe"]
fam = "; ".join("%s %.2f ms at %.1f TFLOP/s" % (k, v["ms"], v["tflops"]) for k, v in sorted(rf["families"].items()))
pipes = "; ".join("%s pipe: %.2f ms, %.1f TFLOP/s executed = %.3f of %.0f" % (k, v["ms_per_step"], v["tflops"], v["frac_of_its_peak"], v["peak"]) for k, v in sorted(pp.items()))
md.append("Headline (conv mode `%s`: %s): **%.1f images/s**, %.2f ms/step%s.  `roofline.frac` = time-weighted mean, over all convolution time incl. the "
          "Winograd transform passes, of each kernel family's executed FLOP rate / the dense peak of ITS matrix pipe = **%.3f** (%s; transforms %.2f ms with no "
          "FLOPs); direct-convolution-equivalent rate of the whole forward %.0f TFLOP/s.  Dominant family `%s`: %.1f TFLOP/s = %.3f of its peak, %d launches/step, "
          "%.0f us average, measured traffic %s MB vs %.0f MB algorithmic per launch (%s).  Families: %s.  Winograd layers: %.2f ms/step = %.2f GEMM + %.2f transforms.\n"
          % (b["config"].get("conv_mode"), b["dtype"][:60] + "...", b["value"], b["ms_per_step"], ("; bs 32: %.0f images/s, frac %.3f" % (bs32["value"], bs32["roofline"]["frac"])) if bs32 else "",
             rf["frac"], pipes, rf["winograd_transform_ms_per_step"], rf["direct_equivalent_tflops"], dom["kernel"], dom["achieved"], dom["frac"], dom["launches_per_step"],
             dom["avg_launch_us"], ("%.0f" % (rf["traffic"] / 1e6)) if rf.get("traffic") else "n/a", dom["algorithmic_bytes_per_launch"] / 1e6, rf.get("traffic_source"), fam,
             wg["ms_per_step"], wg["gemm_ms"], wg["transform_ms"]))
o = b.get("exact_fp32_mfma")
if o:
    orf = o.get("roofline") or {}
    md.append("Same run on the fp32 MFMA everywhere (`exact_fp32_mfma`, conv mode `f32`, the headline of rounds 1-2): **%.1f images/s**, %.2f ms/step, roofline "
              "frac %.3f of %.1f (MFMA families alone %.3f); largest logit difference between the two forwards %.1e (relative).\n"
              % (o["value"], o["ms_per_step"], orf.get("frac", float("nan")), orf.get("peak", float("nan")),
                 (orf.get("per_pipe", {}).get("f32", {}) or {}).get("frac_of_its_peak", float("nan")), o.get("max_logit_difference_vs_headline_rel", float("nan"))))
o2 = b.get("exact_bf16_split")
if o2:
    orf = o2.get("roofline") or {}
    md.append("Same run with exact three-way bf16 splits (`exact_bf16_split`, conv mode `split`, the headline of round 3): **%.1f images/s**, %.2f ms/step, roofline "
              "frac %.3f; largest logit difference from the headline forward %.1e (relative).\n"
              % (o2["value"], o2["ms_per_step"], orf.get("frac", float("nan")), o2.get("max_logit_difference_vs_headline_rel", float("nan"))))
acc = (b.get("cpu_baseline") or {}).get("accuracy_vs_fp64")
if acc:
    md.append("Accuracy inside the same line (`cpu_baseline.accuracy_vs_fp64`): logits %s, vector field %s -- %s.\n"
              % (json.dumps(acc["per_conv_mode"]), json.dumps(acc.get("vector_field_per_conv_mode")), acc["what"]))
gd = b["config"].get("f16x2_guard")
if gd:
    md.append("f16x2 range guard on the timed plan (`config.f16x2_guard`): %d layers checked, not plain f16x2: %s.\n" % (gd["layers_checked"], json.dumps(gd["not_plain_f16x2"]) if gd["not_plain_f16x2"] else "none"))
md.append("`useful_tflops` %.1f = %.3f of the fp32-level peak of this arithmetic (%.0f TFLOP/s = dense 2-byte peak / %d products per fp32 product).\n"
          % (rf["useful_tflops"], rf["useful_frac_of_fp32_equiv_peak"], rf["fp32_equiv_peak"], int(rf.get("products_per_fp32_product", 6))))
alone = []
for name, label in (("bench_infer_f32.json", "`CASAPOSE_INFER_CONV_MODE=f32` as its own run"), ("bench_infer_split.json", "`=split` (exact three-way bf16 splits)"), ("bench_infer_bf16.json", "`=bf16` (operands rounded to bf16, NOT fp32-equivalent)")):
    x = load(name)
    if x:
        alone.append("%s %.0f images/s (%.2f ms, frac %.3f)" % (label, x["value"], x["ms_per_step"], x["roofline"]["frac"]))
if alone:
    md.append("Separate runs: %s.\n" % "; ".join(alone))
tl = b.get("training_leg")
if tl and "value" in tl:
    tb = b.get("training_leg_bf16_convs") or {}
    md.append("Training leg inside the --full line (3 steps at bs 32, 448x448): %.1f images/s, %.1f ms/step%s.\n"
              % (tl["value"], tl["ms_per_step"], ("; the same leg with bf16 convolution operands (BASELINE configs[2] as named): %.1f images/s, %.1f ms/step"
                                                  % (tb["value"], tb["ms_per_step"])) if "value" in tb else ""))
c = b.get("cpu_baseline")
if c:
    md.append("CPU baseline on the same box (%s): **%.2f images/s** -- %s, %s (`%s`; host has %s logical CPUs%s; one process x %s threads: %s images/s).\n"
              % (c.get("cpu"), c["value"], c.get("what"), c.get("shape", "one process"), c.get("sample"), c.get("host_cores"),
                 (", of which the cgroup grants %g CPUs of run time" % c["cpu_quota"]) if c.get("cpu_quota") else "",
                 (c.get("single_process") or {}).get("threads", c.get("cores")), (c.get("single_process") or {}).get("value", c["value"])))
md.append(stats_table(os.path.join(P, "%s_bench_kernel_stats.csv" % tag), rows=18))
mf = os.path.join(P, "%s_pmc_mfma.txt" % tag)
if os.path.exists(mf):
    md.append("\nrocprof MFMA utilisation per kernel (`%s_pmc_mfma.txt`):\n\n```\n%s```\n" % (tag, open(mf).read()))
tf = os.path.join(P, "%s_pmc_traffic.txt" % tag)
if os.path.exists(tf):
    md.append("HBM traffic per launch (`%s_pmc_traffic.txt`, first rows):\n\n```\n%s\n```\n" % (tag, "\n".join(open(tf).read().splitlines()[:16])))
for name, label in (("layer_times.txt", "default (f16x2)"), ("layer_times_conv_mode_split.txt", "`CASAPOSE_INFER_CONV_MODE=split`"), ("layer_times_conv_mode_f32.txt", "`CASAPOSE_INFER_CONV_MODE=f32`")):
    p_ = os.path.join(P, "%s_%s" % (tag, name))
    if os.path.exists(p_):
        md.append("Per-layer times, %s: `%s_%s`." % (label, tag, name))
md.append("\nGPU test suite (`python -m pytest tests -m gpu -q`) per mode:\n")
for name in sorted(f for f in os.listdir(P) if f.startswith(tag + "_gputests_")):
    l = tests_line(name[len(tag) + 1:])
    if l:
        md.append("* `%s`: %s" % (name, l))
md.append("\n## Training step (BASELINE configs[2]: bs 32, 448x448, K = 9; `python bench.py --mode train`)\n")
tr = t["roofline"]
extra = []
for name, label in (("bench_train_conv_mode_f32.json", "`CASAPOSE_CONV_MODE=f32 CASAPOSE_WINO_GEMM=f32` (fp32 MFMA everywhere)"),
                    ("bench_train_conv_mode_bf16.json", "`CASAPOSE_CONV_MODE=bf16` (operands rounded to bf16)"),
                    ("bench_train_exact.json", "`CASAPOSE_TRAIN_FWD=split CASAPOSE_TRAIN_BWD=split` (forward and backward on the exact three-way bf16 split: the default of rounds 2-5)")):
    x = load(name)
    if x:
        extra.append("%s: %.0f images/s (%.1f ms)" % (label, x["value"], x["ms_per_step"]))
md.append("Default of the training plan (%s): **%.1f images/s**, %.1f ms/step; %s.  `roofline`: executed %.0f GFLOP fp32-MFMA + %.0f GFLOP bf16-MFMA "
          "per step; %s = %.3f.  Per op: `%s_train_times.txt`.\n" % (t["dtype"][:120] + "...", t["value"], t["ms_per_step"], "; ".join(extra), tr["executed_f32_gflop_per_step"],
                                                                    tr["executed_bf16_gflop_per_step"], tr["frac_definition"], tr["frac"], tag))
md.append(stats_table(os.path.join(P, "%s_train_kernel_stats.csv" % tag), rows=26))
v = load("bench_vote.json")
if v:
    vr, rs = v["roofline"], v["ransac"]
    md.append("\n## Voting stage alone (`python bench.py --mode vote`)\n")
    md.append("Component filter + LS voter **%.0f images/s** (%.3f ms per 16-image batch); accumulation kernel %.0f us = %.0f GB/s = %.3f of the 8 TB/s HBM roofline; "
              "RANSAC voter %.2f ms per 16-image round = %.3g cosine tests/s%s.\n" % (v["value"], v["ms_per_step"], vr["avg_launch_us"], vr["achieved"], vr["frac"],
                                                                                  rs["ms_per_call"], rs["cosine_tests_per_s"],
                                                                                  (" = %.2f of the fp32 VALU issue rate at %.1f vector instructions per test" % (rs["valu"]["frac"], rs["valu"]["instructions_per_test"])) if "valu" in rs else ""))
    md.append(stats_table(os.path.join(P, "%s_vote_kernel_stats.csv" % tag), rows=12))
open(os.path.join(P, "%s_summary.md" % tag), "w").write("\n".join(md) + "\n")
print("wrote profiles/%s_summary.md and profiles/%s_STAMP.json (%d files)" % (tag, tag, len(COPIED)))
