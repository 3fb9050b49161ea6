"""bench.py --dump-outputs: what the last timed step computed, as float32 .npy files under the 64 MB cap, the same files for the same
arguments -- so that two builds of the project can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CAP = 64 << 20


def _sizes(d):
    return {n: os.path.getsize(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_small_output_is_dumped_whole(tmp_path):
    out = torch.arange(2 * 5 * 7 * 36, dtype=torch.float32).reshape(2, 5, 7, 36)
    kpts = torch.rand(2, 8, 9, 2)
    bench.dump_outputs(str(tmp_path), out, kpts)
    assert set(os.listdir(tmp_path)) == {"network_output.npy", "keypoints.npy"}
    rec, kp = np.load(tmp_path / "network_output.npy"), np.load(tmp_path / "keypoints.npy")
    assert rec.dtype == np.float32 and kp.dtype == np.float32
    assert np.array_equal(rec, out.reshape(-1, 36).numpy()) and np.array_equal(kp, kpts.numpy())


def test_headline_shape_is_sampled_by_a_fixed_seed_under_the_cap(tmp_path):
    """bs 16 at 480 x 640: 707 MB of network output -> DUMP_PIXELS records, the same ones on every call, in (b, y, x) order."""
    b, h, w = 16, 480, 640
    pix = torch.arange(b * h * w, dtype=torch.float32)
    out = pix.reshape(b, h, w, 1).expand(b, h, w, 36)   # every record holds its own pixel index (a view: no 707 MB on the host)
    kpts = torch.zeros(b, 8, 9, 2)
    a, c = tmp_path / "a", tmp_path / "c"
    bench.dump_outputs(str(a), out, kpts)
    bench.dump_outputs(str(c), out, kpts)
    assert sum(_sizes(a).values()) <= CAP
    ra, rc = np.load(a / "network_output.npy"), np.load(c / "network_output.npy")
    assert ra.shape == (bench.DUMP_PIXELS, 36) and np.array_equal(ra, rc)
    idx = ra[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < b * h * w and np.all(ra == ra[:, :1])
    assert np.unique(idx // (h * w)).size == b   # every image of the batch is represented


@pytest.mark.gpu
def test_bench_line_and_dump_on_the_device(tmp_path, device):
    """a tiny headline run: --steps is the number of timed steps, ms_per_step is in the line, the dump is there and finite."""
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--height", "64",
                        "--width", "96", "--no-cpu-baseline", "--no-roofline", "--no-optin", "--no-train-leg", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    rec, kp = np.load(d / "network_output.npy"), np.load(d / "keypoints.npy")
    assert rec.shape == (2 * 64 * 96, 36) and kp.shape == (2, 8, 9, 2)
    assert rec.dtype == np.float32 and np.isfinite(rec).all() and np.isfinite(kp).all()
