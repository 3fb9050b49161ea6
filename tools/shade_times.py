#!/usr/bin/env python3
"""Times of the shaded mesh renderer (csrc/shade.hip) and of the source built on it (data_handler/mesh_scene.py), in the style of mask_times.py:
the sides of a comparison alternate in one process, ROUNDS rounds, medians with the spread (min - max), device events for kernels.

Scene: 8 instances of a subdivision-5 icosphere stretched to an ellipsoid (20 480 triangles each), vertex colours, the procedural background,
noise on.  Cases: a batch of 32 at 448 x 448 and one frame at 480 x 640.
  (default)        (a) cp_render_shaded_f32 (clear, raster, shade) against cp_render_masks_u8 (clear, records, raster, resolve, finish) on the
                   same resident frames, by device events over CALLS calls; (d) the host twin per image by wall clock.
  --kernels-only   CALLS calls of cp_render_shaded_f32 on the batch of 32 and nothing else: the process to put under a kernel trace for the
                   time of each of the two kernels.
  --masks-only     cp_render_masks_u8 alone through a bare ctypes binding of the library CASAPOSE_HIP_LIB names (or this build's): (b), run
                   once per library by the caller, alternating, to show that the mask renderer did not move.
  --dataset        (c) MeshSceneDataset with 8 such objects against SyntheticSceneDataset's device scenes with 8 objects at 448 x 448, batch 32:
                   a batch end to end (host half, upload, kernels, labels) by wall clock around a synchronise, the host half alone, and
                   images/s of training.train_step fed a fresh batch every step by generate_dataset(device=, prefetch=2).
  --outcome S      no threshold: casapose_c_gcu5 / ResNet-18, 2 objects, 224 x 288, batch 8, Adam 1e-3, decoder 2 conditioned on the true labels,
                   S seconds of steps on `meshes:` of two coloured icospheres and, the same recipe, on `synthetic` ellipsoids; then the LS voter
                   over each network's field with the true labels on 32 held-out scenes of its own source: the keypoint error in pixels."""
import ctypes as C, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import raster_reference as RR
if not torch.cuda.is_available():
    raise SystemExit("shade_times.py needs a ROCm GPU: a CPU run gives no device time")
dev = torch.device("cuda:0")
ROUNDS, CALLS = 3, 10
NEAR, FAR = 100.0, 2000.0
CAM = (572.4114, 573.57043, 325.2611, 242.04899)
CASES = ((32, 448, 448), (1, 480, 640))
AXES = np.array([60.0, 45.0, 80.0])
spread = lambda v: "%.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))  # noqa: E731

def frames_of(n, H, W):
    rng, out = np.random.default_rng(8), []
    cam = (CAM[0], CAM[1], CAM[2] - (640 - W) / 2, CAM[3] - (480 - H) / 2)
    for _ in range(n):
        inst = [(0, 10 + 30 * k, RR.pose_at(cam, W * (k + 0.5) / 8.0 + rng.uniform(-10, 10), H / 2.0 + rng.uniform(-0.25 * H, 0.25 * H), 500.0 + 90.0 * k,
                                            RR.rotation(rng.normal(size=3), rng.uniform(0, 3)))) for k in range(8)]
        out.append(dict(cam=cam, instances=inst))
    return out

def mesh():
    v, f = RR.icosphere(5)
    return (v * AXES).astype(np.float32), f

def timed(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / calls

def masks_call(lib, d_mesh, vmax, tmax, d, n, H, W):
    from casapose_amd.data_handler.bop_converter import RECORD
    labels, records = torch.empty((n, H, W), dtype=torch.uint8, device=dev), torch.empty((n, 8, RECORD), dtype=torch.int32, device=dev)
    ws = torch.empty(n * 8 * H * W * 4, dtype=torch.uint8, device=dev)
    def call():
        rc = lib.cp_render_masks_u8(d_mesh[0].data_ptr(), d_mesh[1].data_ptr(), vmax, d_mesh[2].data_ptr(), d_mesh[3].data_ptr(), tmax, 1, d["cams"].data_ptr(),
                                    d["inst_counts"].data_ptr(), d["inst_obj"].data_ptr(), d["inst_label"].data_ptr(), d["poses"].data_ptr(), n, 8, H, W, NEAR, FAR,
                                    0.5, labels.data_ptr(), records.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    return call, labels

def shaded_call(r, d, lights, n, H, W, noise=True):
    ws = torch.empty(r.workspace_bytes(n, H, W) // 8, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    keep = {}
    def call():
        keep["out"] = r.call(r.masks.d_mesh, r.d_colors, r.d_flat, d, lights, None, noise, n, H, W, NEAR, FAR, 0.5, True, ws, dev, st)
    return call, keep

def renderer():
    from casapose_amd.data_handler.mesh_scene import ShadedRenderer
    v, f = mesh()
    return ShadedRenderer(dev, {0: (v, f)}, {0: np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8)}, {0: (0.5, 0.5, 0.5)})

def lights_of(n):
    from casapose_amd.data_handler.mesh_scene import frame_record
    return np.stack([frame_record((0.36, 0.48, -0.8), 0.3, 0.6, 99 + f, 16.0, 96.0) for f in range(n)])

def kernel_times(kernels_only=False):
    from casapose_amd import _lib
    lib, r = _lib.load(), renderer()
    for n, H, W in CASES[:1] if kernels_only else CASES:
        frames = frames_of(n, H, W)
        d = {k: torch.from_numpy(a).to(dev) for k, a in r.masks.pack(frames).items()}
        lights = torch.from_numpy(lights_of(n)).to(dev)
        shaded, keep = shaded_call(r, d, lights, n, H, W)
        masks, labels = masks_call(lib, r.masks.d_mesh, r.masks.vmax, r.masks.tmax, d, n, H, W)
        for _ in range(2): shaded(); masks()
        torch.cuda.synchronize()
        assert torch.equal(keep["out"]["label"], labels)
        if kernels_only:
            print("%d calls of cp_render_shaded_f32, %d frames of %d x %d: %.3f ms per call" % (CALLS, n, H, W, timed(shaded)))
            return
        clean, _ = shaded_call(r, d, lights, n, H, W, noise=False)
        clean(); torch.cuda.synchronize()
        shaded_ms, masks_ms, clean_ms, twin_s = [], [], [], []
        for _ in range(ROUNDS):
            shaded_ms.append(timed(shaded)); masks_ms.append(timed(masks)); clean_ms.append(timed(clean))
            t0 = time.perf_counter(); host = r.render_host(frames[:1], lights_of(1), H, W, NEAR, FAR, noise=True); twin_s.append(time.perf_counter() - t0)
        assert np.array_equal(host["label"][0], labels[0].cpu().numpy())
        covered = float((labels > 0).float().mean())
        print("%2d frame(s), %d x %d, 8 instances x 20480 triangles, %.0f %% of the pixels covered: cp_render_shaded_f32 %s ms per call by device events, "
              "cp_render_masks_u8 on the same frames %s ms (shaded / masks %.2f), cp_render_shaded_f32 without noise %s ms; the host twin %s s per image"
              % (n, H, W, 100 * covered, spread(shaded_ms), spread(masks_ms), np.median(shaded_ms) / np.median(masks_ms), spread(clean_ms), spread(twin_s)))

def masks_only():
    # the named library serves the timed call alone; the package (MaskRenderer's packing) binds this build's, which has every declared symbol
    path = os.environ.pop("CASAPOSE_HIP_LIB", None) or os.path.join(ROOT, "casapose_amd", "libcasapose_hip.so")
    lib = C.CDLL(path)
    i, p, dbl = C.c_int, C.c_void_p, C.c_double
    lib.cp_render_masks_u8.argtypes = [p, p, i, p, p, i, i, p, p, p, p, p, i, i, i, i, dbl, dbl, dbl, p, p, p, C.c_size_t, p]
    from casapose_amd.data_handler.bop_converter import MaskRenderer
    v, f = mesh()
    r = MaskRenderer(dev, {0: (v, f)})
    out = []
    for n, H, W in CASES:
        d = {k: torch.from_numpy(a).to(dev) for k, a in r.pack(frames_of(n, H, W)).items()}
        masks, labels = masks_call(lib, r.d_mesh, r.vmax, r.tmax, d, n, H, W)
        for _ in range(2): masks()
        torch.cuda.synchronize()
        out.append("%d x %d x %d: %s ms" % (n, H, W, spread([timed(masks) for _ in range(ROUNDS)])))
    print("cp_render_masks_u8 of %s: %s" % (os.path.relpath(path, ROOT), "; ".join(out)))

def write_folder(root, objects, subdivisions=5):
    from casapose_amd.data_handler.model_prep import write_keypoints_ply
    v, f = RR.icosphere(subdivisions)
    rng = np.random.default_rng(3)
    info = {}
    for o in range(objects):
        axes = rng.uniform(35.0, 70.0, 3)
        col = rng.integers(30, 256, (len(v), 3))
        stem = "obj_%06d" % (o + 1)
        with open(os.path.join(root, stem + ".ply"), "w") as out:
            out.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                      "property uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
            out.write("".join("%.9g %.9g %.9g %d %d %d\n" % (*(p * axes), *c) for p, c in zip(v, col)))
            out.write("".join("3 %d %d %d\n" % tuple(t) for t in f))
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * axes
        write_keypoints_ply(os.path.join(root, stem + "_keypoints.ply"), np.concatenate([np.zeros((1, 3)), corners]))
        info[stem] = {"diameter": 2.0 * float(axes.max())}
    json.dump(info, open(os.path.join(root, "models_info.json"), "w"))

def dataset_times():
    from types import SimpleNamespace
    from casapose_amd import training as TR
    from casapose_amd.data_handler.mesh_scene import MeshSceneDataset
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler
    oc, (H, W), bs = 8, (448, 448), 32
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, oc)
        sources = {"meshes": MeshSceneDataset(root, oc, (H, W), length=1 << 20, seed=1), "synthetic": SyntheticSceneDataset(oc, (H, W), length=1 << 20, seed=1)}
    for ds in sources.values():
        for i in range(2): ds.batch(i, bs, device=dev)
    torch.cuda.synchronize()
    batch_ms, half_ms = {k: [] for k in sources}, {k: [] for k in sources}
    for r in range(ROUNDS):
        for name, ds in sources.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(CALLS): ds.batch(r * CALLS + i, bs, device=dev)
            torch.cuda.synchronize(); batch_ms[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
            t0 = time.perf_counter()
            for i in range(CALLS): ds.device_scenes(dev).host_half(range(i * bs, (i + 1) * bs))
            half_ms[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
    for name in sources:
        print("%s, 448 x 448, 8 objects, batch 32: a device batch end to end %s ms, of which the host half %s ms" % (name, spread(batch_ms[name]), spread(half_ms[name])))
    net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=oc + 1, input_shape=(H, W, 3), input_segmentation_shape=(H, W, oc + 1), weights=None,
                                             base_model="resnet18", device=dev, seed=3)
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=True, max_keypoint_pixel_error=12.5, confidence_regularization=True,
                          use_bpnp_reprojection_loss=False)
    lf, optim = LossWeightHandler(1.0, 0.5, 0.015, 0.007, filter_vertex_with_segmentation=True), TR.Adam(learning_rate=1e-3)
    feeds = {name: ds.generate_dataset(bs, device=dev, prefetch=2)[0] for name, ds in sources.items()}
    fixed = next(feeds["synthetic"])
    for name in feeds: TR.train_step(net, next(feeds[name]), lf, optim, opt)
    rates, steps = {"meshes": [], "synthetic": [], "one resident batch": []}, 10
    for _ in range(ROUNDS):
        for name in rates:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps): TR.train_step(net, fixed if name == "one resident batch" else next(feeds[name]), lf, optim, opt)
            torch.cuda.synchronize(); rates[name].append(steps * bs / (time.perf_counter() - t0))
    print("train_step, 448 x 448, 8 objects, batch 32, a fresh batch every step (prefetch 2): " + "; ".join("%s %s images/s" % (k, spread(v)) for k, v in rates.items()))

def outcome(seconds):
    from types import SimpleNamespace
    from casapose_amd import training as TR
    from casapose_amd.data_handler.mesh_scene import MeshSceneDataset
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset
    from casapose_amd.pose_estimation.voting_layers_2d import CoordLSVotingWeighted
    from casapose_amd.pose_models.tfkeras import Classifiers
    from casapose_amd.utils.learning_rate_schedules import LossWeightHandler, PiecewiseConstantDecay
    oc, (H, W), bs, k = 2, (224, 288), 8, 3
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, oc, 3)
        sources = {"meshes (two coloured icospheres, 1280 triangles each)": lambda seed: MeshSceneDataset(root, oc, (H, W), length=1 << 30, seed=seed),
                   "synthetic (two ellipsoids)": lambda seed: SyntheticSceneDataset(oc, (H, W), length=1 << 30, seed=seed)}
        sources = {name: (make(100), make(977)) for name, make in sources.items()}
    opt = SimpleNamespace(train_vectors_with_ground_truth=True, estimate_coords=False, max_keypoint_pixel_error=12.5, confidence_regularization=False,
                          use_bpnp_reprojection_loss=False)
    for name, (train, held) in sources.items():
        net = Classifiers.get("casapose_c_gcu5")(ver_dim=27, seg_dim=k, input_shape=(H, W, 3), input_segmentation_shape=(H, W, k), weights=None,
                                                 base_model="resnet18", device=dev, seed=3)
        lf, optim = LossWeightHandler(1.0, 0.5, 0.015, 0.0, filter_vertex_with_segmentation=True), TR.Adam(learning_rate=PiecewiseConstantDecay([1 << 30], [1e-3, 1e-3]))
        feed, hist, t0 = train.generate_dataset(bs, 1, 2, device=dev)[0], [], time.time()
        while time.time() - t0 < seconds:
            hist.append(TR.train_step(net, next(feed), lf, optim, opt))
            if len(hist) % 2000 == 0: print("  ... %d steps, loss %.4g" % (len(hist), hist[-1][0]), flush=True)
        voter = CoordLSVotingWeighted(name="coords_ls_voting", num_classes=k, num_points=9, filter_estimates=False)
        errs = []
        for i in range(32):
            bt = held.batch(i, 1, device=dev)
            seg = bt["target_seg"]
            out = net([bt["img"], seg], training=False)
            coords = voter([(10.0 * seg).contiguous(), out[..., k:k + 18].contiguous(), out[..., k + 18:k + 27].contiguous()]).cpu().numpy()[0]
            gt, px = bt["target_vert"][0, :, 0].numpy(), bt["pixel_gt_count"][0, :, 0, 0].numpy()
            errs += [np.linalg.norm(coords[o] - gt[o], axis=-1) for o in range(oc) if px[o] >= 300]
        errs, parts = np.concatenate(errs), np.array_split(np.array(hist), 10)
        print("%s: %d steps in %d s (%.0f steps/s)" % (name, len(hist), seconds, len(hist) / seconds))
        for col, what in ((0, "loss"), (1, "mask"), (2, "vertex"), (3, "proxy")):
            print("    %-7s in ten parts of the run: %s" % (what, " ".join("%.4g" % q[:, col].mean() for q in parts if len(q))))
        print("    LS voter with the true labels on 32 held-out scenes, %d keypoints of objects with at least 300 px: median error %.2f px, 90th percentile %.2f px, "
              "within 2 px %.1f %%" % (len(errs), np.median(errs), np.percentile(errs, 90), 100.0 * (errs < 2.0).mean()))

if "--outcome" in sys.argv:
    outcome(int(sys.argv[sys.argv.index("--outcome") + 1]))
elif "--kernels-only" in sys.argv:
    kernel_times(True)
elif "--masks-only" in sys.argv:
    masks_only()
elif "--dataset" in sys.argv:
    dataset_times()
else:
    kernel_times()
