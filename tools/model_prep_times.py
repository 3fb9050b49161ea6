#!/usr/bin/env python3
"""Times of ModelPrep (keypoints and models_info from the meshes): the device call (cp_model_prep_f32, csrc/models.hip) by device events, its host
twin (cp_model_prep_host_f32) and a chunked NumPy brute force of the diameter by wall clock, in one process, after a warm-up.

Cases: a unit sphere of 10^4, 10^5 and 5 * 10^5 vertices, and a set of 20 objects of mixed sizes (500 to 200 000 vertices) in one call.  Medians over
ROUNDS rounds with the spread (min - max); the pair rate (vertex pairs of the upper triangle per second of the whole device call, keypoints
included) and that rate as a share of the part's fp64 vector rate.  A pair costs nine fp64 vector operations, none of them fused (three
differences, three products, two sums, one compare-select), each of which takes the issue slot of one FMA: the share is 9 * pairs/s over the FMA
rate, 39.3e12 per second (78.6 TFLOPS of fp64 vector peak, two operations per FMA).  The host twin is quadratic and serial: it is run up to
--host-max vertices (default 10^5), NumPy up to --numpy-max (default 10^4); beyond that the line says so and scales the last measured time by N^2."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from casapose_amd.data_handler.model_prep import ModelPrep
if not torch.cuda.is_available():
    raise SystemExit("model_prep_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
ROUNDS, WARMUP, K = 5, 2, 9
FP64_FMA_PER_S, OPS_PER_PAIR = 39.3e12, 9
spread = lambda v: "%.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))  # noqa: E731

def sphere(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

def numpy_diameter_sq(v32):
    v, best = v32.astype(np.float64), 0.0
    for lo in range(0, len(v), 256):
        d = v[lo:lo + 256, None, :] - v[None, :, :]
        best = max(best, float(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max()))
    return best

def device_ms(prep, meshes):
    p = prep.pack(meshes, list(meshes))
    d = prep.upload(p, len(meshes), K)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(WARMUP): prep.launch(d, len(meshes), p["total"], K, stream)
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); prep.launch(d, len(meshes), p["total"], K, stream); e1.record()
        e1.synchronize(); ms.append(e0.elapsed_time(e1))
    assert (d["status"].cpu().numpy() == 0).all()
    return ms, d["diameter_sq"].cpu().numpy()

def wall_s(fn, rounds):
    out, s = None, []
    for _ in range(rounds):
        t0 = time.perf_counter(); out = fn(); s.append(time.perf_counter() - t0)
    return s, out

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-max", type=int, default=100000)
    ap.add_argument("--numpy-max", type=int, default=10000)
    a = ap.parse_args()
    prep, host = ModelPrep(dev), ModelPrep(None)
    sizes = [int(n) for n in np.geomspace(500, 200000, 20)]
    cases = [("sphere, %d vertices" % n, {0: sphere(n, n)}) for n in (10000, 100000, 500000)]
    cases.append(("20 objects, %d to %d vertices" % (sizes[0], sizes[-1]), {i: sphere(n, i) * (1.0 + i) for i, n in enumerate(sizes)}))
    last = {}   # the last measured (seconds, pairs) of the host twin and of NumPy, for the N^2 estimate
    for name, meshes in cases:
        pairs = sum(len(v) * (len(v) - 1) // 2 for v in meshes.values())
        largest = max(len(v) for v in meshes.values())
        ms, diam = device_ms(prep, meshes)
        rate = pairs / (np.median(ms) * 1e-3)
        line = "%s: %.3g pairs; device %s ms by device events, %.3g pairs/s = %.1f %% of the fp64 vector rate" % (
            name, pairs, spread(ms), rate, 100.0 * rate * OPS_PER_PAIR / FP64_FMA_PER_S)
        for what, limit, fn in (("host twin", a.host_max, lambda: host.outputs(meshes, K, host=True)["diameter_sq"]),
                                ("NumPy brute force (diameter only)", a.numpy_max, lambda: np.array([numpy_diameter_sq(v) for v in meshes.values()]))):
            if largest <= limit and len(meshes) == 1:
                s, got = wall_s(fn, 3 if largest <= 20000 else 1)
                assert got.tobytes() == diam.tobytes(), (what, got, diam)   # the same bits as the device
                last[what] = (np.median(s), pairs)
                line += "; %s %s s (%.0f x the device)" % (what, spread(s), np.median(s) * 1e3 / np.median(ms))
            elif what in last:
                est = last[what][0] * pairs / last[what][1]
                line += "; %s not run, about %.0f s by N^2 from the last measured size (%.0f x the device)" % (what, est, est * 1e3 / np.median(ms))
        print(line)

if __name__ == "__main__":
    main()
