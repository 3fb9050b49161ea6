#!/usr/bin/env python3
"""Times of the mask renderer: the host twin (cp_render_masks_host_u8, serial) against the device (csrc/masks.hip) in one process, the two
alternating.

Scene: 480 x 640, 8 instances of a subdivision-5 icosphere stretched to an ellipsoid (20 480 triangles each; LM's scale).  Cases: one frame, and a
chunk of 32 frames (the poses jittered per frame).  Per round: the twin once by wall clock; the kernels alone (the five launches of one call, inputs
and workspace resident) by device events over CALLS calls; MaskRenderer.render (pack, upload, kernels, labels and records back) by wall clock; and,
for the chunk, the converter's end of it -- render_chunks with every label map encoded to a PNG on the I/O pool -- by wall clock, next to the PNG
encoding alone.  Medians over ROUNDS rounds with the spread (min - max)."""
import io, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from concurrent.futures import ThreadPoolExecutor
import numpy as np, torch
from PIL import Image
import raster_reference as RR
from casapose_amd import _lib
from casapose_amd.data_handler.bop_converter import RECORD, MaskRenderer
if not torch.cuda.is_available():
    raise SystemExit("mask_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
ROUNDS, CALLS = 3, 10
H, W, NEAR, FAR = 480, 640, 100.0, 2000.0
CAM = (572.4114, 573.57043, 325.2611, 242.04899)
spread = lambda v: "%.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))  # noqa: E731

def frames_of(n):
    rng, out = np.random.default_rng(8), []
    for _ in range(n):
        inst = [(0, 10 + 30 * k, RR.pose_at(CAM, 120.0 + 60.0 * k + rng.uniform(-10, 10), 240.0 + rng.uniform(-120, 120), 500.0 + 90.0 * k,
                                            RR.rotation(rng.normal(size=3), rng.uniform(0, 3)))) for k in range(8)]
        out.append(dict(cam=CAM, instances=inst))
    return out

def png(label):
    buf = io.BytesIO(); Image.fromarray(label).save(buf, format="PNG"); return buf.tell()

def main():
    v, f = RR.icosphere(5)
    r = MaskRenderer(dev, {0: ((v * np.array([60.0, 45.0, 80.0])).astype(np.float32), f)})
    lib, pool = _lib.load(), ThreadPoolExecutor(min(16, os.cpu_count()))
    for n in (1, 32):
        frames = frames_of(n)
        p = r.pack(frames)
        d = {k: torch.from_numpy(a).to(dev) for k, a in p.items()}
        labels, records = torch.empty((n, H, W), dtype=torch.uint8, device=dev), torch.empty((n, 8, RECORD), dtype=torch.int32, device=dev)
        ws = torch.empty(lib.cp_render_masks_workspace_bytes(n, 8, H, W), dtype=torch.uint8, device=dev)
        def kernels():
            _lib.check(lib.cp_render_masks_u8(r.d_mesh[0].data_ptr(), r.d_mesh[1].data_ptr(), r.vmax, r.d_mesh[2].data_ptr(), r.d_mesh[3].data_ptr(), r.tmax, 1,
                                              d["cams"].data_ptr(), d["inst_counts"].data_ptr(), d["inst_obj"].data_ptr(), d["inst_label"].data_ptr(),
                                              d["poses"].data_ptr(), n, 8, H, W, NEAR, FAR, 0.5, labels.data_ptr(), records.data_ptr(), ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream().cuda_stream), "cp_render_masks_u8")
        for _ in range(2): kernels(); r.render(frames, H, W, NEAR, FAR)
        torch.cuda.synchronize()
        twin_s, kernel_ms, render_ms, end_ms, png_ms = [], [], [], [], []
        for _ in range(ROUNDS):
            t0 = time.perf_counter(); host = r.render_host(frames, H, W, NEAR, FAR); twin_s.append(time.perf_counter() - t0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS): kernels()
            e1.record(); e1.synchronize(); kernel_ms.append(e0.elapsed_time(e1) / CALLS)
            t0 = time.perf_counter()
            for _ in range(CALLS): got = r.render(frames, H, W, NEAR, FAR)
            render_ms.append((time.perf_counter() - t0) * 1e3 / CALLS)
            assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])
            t0 = time.perf_counter(); list(pool.map(png, list(host[0]))); png_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            jobs = [pool.submit(png, np.array(l)) for _, ls, _ in r.render_chunks(frames, H, W, NEAR, FAR, 0.5, (8 if n > 1 else 1) * ws.numel() // n) for l in ls]
            [j.result() for j in jobs]; end_ms.append((time.perf_counter() - t0) * 1e3)
        print("%2d frame(s), 480 x 640, 8 instances x 20480 triangles: twin %s s; kernels alone %s ms by device events; MaskRenderer.render %s ms; "
              "rendered in chunks of %d with the PNGs encoded on the pool %s ms, the PNG encoding alone %s ms; twin / render %.0f x"
              % (n, spread(twin_s), spread(kernel_ms), spread(render_ms), 8 if n > 1 else 1, spread(end_ms), spread(png_ms), np.median(twin_s) * 1e3 / np.median(render_ms)))

main()
