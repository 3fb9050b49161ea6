"""bench.py's plain line and its `--full` line: a plain run measures the headline and nothing else; `--full` adds the annotations (roofline
tables, the other fp32 arithmetics, training legs, CPU baseline) after the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "gpus_requested", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "binary"}
FULL_ONLY = {"roofline", "roofline_bs32", "exact_fp32_mfma", "exact_bf16_split", "training_leg", "training_leg_exact_split", "training_leg_bf16_convs",
             "cpu_baseline"}
TINY = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--height", "64", "--width", "96"]


def _line(extra, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + TINY + extra, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("mode", ["train", "vote"])
def test_full_is_refused_outside_the_headline_mode(mode):
    """--mode train / vote measure their own workload only: --full there is an argument error, raised before anything touches a GPU"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", mode, "--full"], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(device):
    d = _line([], 600)
    assert set(d) == HEADLINE, sorted(set(d) ^ HEADLINE)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["unit"] == "images/s"
    assert abs(d["value"] - 2 / (d["ms_per_step"] / 1e3)) < 0.02 * d["value"]


@pytest.mark.gpu
def test_full_line_adds_the_annotations(device):
    """--full without the training legs and the CPU baseline (tests of their own): the roofline tables and the other fp32 arithmetics beside the
    same headline keys"""
    d = _line(["--full", "--no-train-leg", "--no-cpu-baseline"], 900)
    assert HEADLINE <= set(d) and not ({"training_leg", "cpu_baseline"} & set(d))
    assert d["roofline"]["frac"] > 0 and "error" not in d["roofline_bs32"]
    others = [k for k in ("exact_fp32_mfma", "exact_bf16_split") if k in d]
    assert all(d[k]["value"] > 0 for k in others)
    if d["config"]["conv_mode"] in ("split", "f16x2"):   # (the other arithmetics are measured beside these two headline modes)
        assert "exact_fp32_mfma" in others
