"""cp_mask_edt_host_u16 and cp_contour_step_host_f64 -- the host twins of the mask refinement's kernels, the same header the device kernels
compile -- against SciPy and the NumPy restatement (tests/contour_reference.py), and `DeviceMaskRefiner.refine(host=True)` against the
reference's loop.  No GPU is needed.  The helpers and the case tables also serve tests/test_gpu_mask_refine.py."""
import ctypes as C
import os

import numpy as np
import pytest

import contour_cases as CC
import contour_reference as CR
import icp_reference as IR
import vsd_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
GATE, DAMPING, MIN_PIXELS = CR.GATE, CR.DAMPING, CR.MIN_PIXELS
PLANE_FILL = 0x5A5A      # what a plane holds before the call: a refused job leaves it


# ---- the distance field through the entry point ---------------------------------------------------------------------------------------------
def blobs(H, W, seed, labels=(1, 2, 3)):
    """a label map of overlapping discs, later ones on top"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((H, W), np.uint8)
    for l in labels:
        for _ in range(2):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(3, min(H, W) / 3)
            out[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = l
    return out


def edt_cases():
    """name -> (labels uint8 [images, H, W], jobs [(image, label)], G); the jobs are all in range"""
    if not _edt_cases:
        a, b = CC.label_map(48, 64), CC.label_map(37, 50)
        frame = np.full((20, 30), 4, np.uint8)
        frame[6:12, 8:20] = 0                                                    # label 4 touches all four borders; its seeds ring the hole
        one = np.zeros((9, 11), np.uint8)
        one[4, 6] = 9
        high = blobs(30, 41, 3, (255, 1))
        _edt_cases.update({
            "48 x 64": (a[None], [(0, 1), (0, 2), (0, 3)], GATE),
            "37 x 50": (np.stack([b, CC.label_map(37, 50, 0)]), [(0, 1), (1, 1), (0, 3), (0, 2)], GATE),
            "G = 1": (a[None], [(0, 1), (0, 3)], 1),
            "G = 12": (a[None], [(0, 1), (0, 2)], 12),
            "G = 255 at 37 x 50": (b[None], [(0, 1), (0, 2), (0, 3)], 255),
            "no seeds": (a[None], [(0, 77), (0, 1)], 5),
            "all four borders": (frame[None], [(0, 4)], 7),
            "label 255": (high[None], [(0, 255), (0, 1)], 6),
            "one pixel": (one[None], [(0, 9)], 4),
            "W = 65": (np.stack([blobs(40, 65, 1), blobs(40, 65, 2)]), [(1, 3), (0, 1), (0, 2), (1, 1)], 9),
            "W = 300": (blobs(33, 300, 4)[None], [(0, 1), (0, 2)], 40),          # more than one 256-column block of a row
        })
        for labels, _, _ in _edt_cases.values():
            labels.setflags(write=False)
    return _edt_cases


_edt_cases = {}


def run_edt(labels, jobs, G, device=None, fill=0xA5):
    """cp_mask_edt_u16 on `device`, or its host twin (device None); the workspace pre-filled with the byte `fill`, the planes with PLANE_FILL
    -> dict(planes uint16 [njobs, H, W], status [njobs], rows uint16 [njobs, H, W]) as NumPy arrays"""
    from casapose_amd import _lib, twin

    lib = _lib.load()
    images, H, W = labels.shape
    jobs = np.asarray(jobs, np.int32).reshape(-1, 2)
    n = len(jobs)
    size = int(lib.cp_mask_edt_workspace_bytes(n, H, W))
    assert size == n * H * W * 2
    stream = None
    if device is not None:
        import torch

        stream = torch.cuda.current_stream(device).cuda_stream
    arg = dict(labels=twin.array(labels, np.uint8, device), jobs=twin.array(jobs, np.int32, device),
               planes=twin.array(np.full((n, H, W), PLANE_FILL, np.uint16), np.uint16, device),
               status=twin.array(np.full(n, -7, np.int32), np.int32, device), work=twin.array(np.full(size, fill, np.uint8), np.uint8, device))
    twin.call("cp_mask_edt_u16", arg["labels"], images, H, W, arg["jobs"], n, int(G), arg["planes"], arg["status"], arg["work"], size,
              host=device is None, stream=stream)
    back = lambda t: t if device is None else t.cpu().numpy()   # noqa: E731
    return dict(planes=back(arg["planes"]), status=back(arg["status"]), rows=back(arg["work"]).view(np.uint16).reshape(n, H, W))


def host_edt(name):
    if name not in _host_edt:
        _host_edt[name] = run_edt(*edt_cases()[name])
    return _host_edt[name]


_host_edt = {}


@pytest.mark.parametrize("name", list(edt_cases()))
def test_field_twin_equals_scipy_bit_for_bit(name):
    labels, jobs, G = edt_cases()[name]
    got = host_edt(name)
    assert got["planes"].dtype == np.uint16 and not got["status"].any()
    for n, (m, l) in enumerate(jobs):
        want = CR.field(labels[m], l, G)
        assert got["planes"][n].tobytes() == want.tobytes(), (name, n, np.argwhere(got["planes"][n] != want)[:4].tolist())
    if name == "no seeds":
        assert (got["planes"][0] == 26).all() and (got["planes"][1] == 0).any()
    if name == "G = 255 at 37 x 50":
        assert got["planes"].max() < 255 * 255              # the window is larger than the image: nothing is clamped
    if name == "one pixel":
        assert got["planes"][0, 4, 6] == 0 and (got["planes"][0] == 0).sum() == 1 and got["planes"][0, 0, 0] == 17


def test_occlusion_and_border_edges_make_no_seed():
    """label 1: a rectangle against the left border whose right part lies under label 2.  Its seeds are its upper and lower edges; the edge
    towards label 2 and the edge at the border have none, except where they end on the upper and lower edges."""
    lab = np.zeros((1, 12, 16), np.uint8)
    lab[0, 3:9, 0:7] = 1
    lab[0, 2:10, 7:11] = 2
    got = run_edt(lab, [(0, 1), (0, 2)], 4)
    seeds = got["planes"][0] == 0
    want = np.zeros((12, 16), bool)
    want[3, 0:7] = want[8, 0:7] = True
    assert np.array_equal(seeds, want)
    assert got["planes"][0, 5, 0] == 4 and got["planes"][0, 5, 6] == 4          # border column, occlusion column: two rows from a seed
    seeds2 = got["planes"][1] == 0
    assert seeds2[2:10, 10].all() and seeds2[2, 7:11].all() and seeds2[9, 7:11].all() and not seeds2[3:9, 7].any()   # towards label 1: none
    relabelled = run_edt(np.where(lab == 2, 0, lab).astype(np.uint8), [(0, 1)], 4)
    assert (relabelled["planes"][0, 3:9, 6] == 0).all()                         # the same edge towards background is seeded


def test_field_refusals_leave_their_planes_alone():
    labels, _, G = edt_cases()["48 x 64"]
    good = host_edt("48 x 64")
    big = 2 ** 31 - 1
    got = run_edt(labels, [(0, 1), (1, 1), (-1, 1), (0, 0), (0, 256), (0, -1), (big, big), (0, 3)], G)
    assert got["status"].tolist() == [0, 3, 3, 3, 3, 3, 3, 0]
    assert got["planes"][0].tobytes() == good["planes"][0].tobytes() and got["planes"][7].tobytes() == good["planes"][2].tobytes()
    assert (got["planes"][1:7] == PLANE_FILL).all() and (got["rows"][1:7].view(np.uint8) == 0xA5).all()


@pytest.mark.parametrize("name", ["37 x 50", "W = 65"])
def test_field_does_not_depend_on_the_workspace(name):
    first = host_edt(name)
    for fill in (0x00, 0xFF):
        again = run_edt(*edt_cases()[name], fill=fill)
        assert again["planes"].tobytes() == first["planes"].tobytes() and again["status"].tobytes() == first["status"].tobytes()


# ---- one step through the entry point ---------------------------------------------------------------------------------------------------
def step_arrays(case, gate=GATE):
    """the host arrays of one step over a case: every estimate rendered by the renderer's host twin into frames of up to 256 slots, one
    field per (image, label) from the field's host twin, one job per estimate -> dict(planes, records, fields, cams, jobs, poses, H, W, labels)"""
    from casapose_amd.data_handler.bop_converter import MAX_INSTANCES, MaskRenderer

    images, H, W = case["labels"].shape
    by_image = {}
    for i, m in enumerate(case["img"]):
        by_image.setdefault(int(m), []).append(i)
    imax = min(MAX_INSTANCES, max(len(r) for r in by_image.values()))
    frames, jobs, order, field_of = [], [], [], {}
    for m, rows in by_image.items():
        for lo in range(0, len(rows), imax):
            part = rows[lo:lo + imax]
            for k, i in enumerate(part):
                f = field_of.setdefault((m, int(case["label_of"][i])), len(field_of))
                jobs.append((m, len(frames) * imax + k, f, gate))
            order += part
            frames.append(dict(cam=case["cam"], instances=[(int(case["obj"][i]), 1, case["poses"][i]) for i in part]))
    renderer = MaskRenderer(None, {i: m for i, m in enumerate(case["meshes"])})
    planes, records = VR.render_planes(renderer, frames, H, W, CC.NEAR, CC.FAR, CC.SAMPLE_OFFSET)
    poses = np.zeros((len(frames) * imax, 12))
    poses[[j[1] for j in jobs]] = case["poses"][order].reshape(-1, 12)
    fields = run_edt(case["labels"], list(field_of), gate)["planes"]
    return dict(planes=planes.reshape(-1, H, W), records=np.ascontiguousarray(records.reshape(-1, 11)), fields=fields,
                cams=np.tile(np.asarray(case["cam"], np.float64), (images, 1)), jobs=np.asarray(jobs, np.int32), poses=poses, H=H, W=W,
                order=np.asarray(order), offset=CC.SAMPLE_OFFSET)


def crafted(tile):
    """Hand-made planes for the entry point itself: a box that ends inside the first tile, one that spans three tiles (the last one half
    full), one across the border, an empty record and a box in column 0, which the clipping empties; each plane is hit everywhere inside its
    box at a smooth, tilted depth and EMPTY outside, as the renderer leaves it.  The fields are those of label rectangles one or two pixels
    off the boxes, so that the straight parts of the contours have e = 0 in one coordinate and some contour pixels sit on their seed."""
    bw = 64
    rows_a, rows_b = tile // bw - 6, (5 * tile // 2) // bw
    H, W = rows_b + 10, bw + 6
    boxes = [(3, 3, bw - 1, rows_a - 1), (3, 3, bw - 1, rows_b - 1), (-5, -4, 30, 20), (-1, -1, -1, -1), (0, 5, 0, 10)]
    rng = np.random.default_rng(3)
    n = len(boxes)
    planes = np.full((n, H, W), VR.EMPTY, np.uint32)
    records = np.full((n, 11), -1, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for p, (x, y, w, h) in enumerate(boxes):
        records[p, 2:6] = (x, y, w, h)
        if w < 0 or h < 0:
            continue
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W - 1), min(y + h, H - 1)
        a, b = rng.uniform(-0.6, 0.6, 2)
        z = (1000.0 + a * (xx - x) + b * (yy - y) + 4.0 * np.sin(0.35 * xx + p) * np.cos(0.3 * yy)).astype(np.float32)
        planes[p, y0:y1 + 1, x0:x1 + 1] = z.view(np.uint32)[y0:y1 + 1, x0:x1 + 1]
    labels = np.zeros((3, H, W), np.uint8)
    labels[0, 3:rows_a + 4, 4:bw + 2] = 1          # the upper edge on box 0's, the others one or two pixels off
    labels[1, 4:rows_b + 4, 2:bw + 1] = 2
    labels[2, 0:18, 0:27] = 3                      # at the border: seeds on its right and lower edge only
    fields = run_edt(labels, [(0, 1), (1, 2), (2, 3)], 3)["planes"]
    poses = np.tile(np.hstack([np.eye(3), [[0.0], [0.0], [1000.0]]]).reshape(12), (n, 1))
    jobs = np.array([(0, 0, 0, 3), (1, 1, 1, 3), (2, 2, 2, 3), (0, 3, 0, 3), (0, 4, 0, 3)], np.int32)
    return dict(planes=planes, records=records, fields=fields, cams=np.tile([[400.0, 410.0, W / 2 - 0.3, H / 2 + 0.2]], (3, 1)), poses=poses,
                jobs=jobs, H=H, W=W, offset=0.25)


def run_step(a, device=None, split=1, fill=0xA5, update=1, damping=DAMPING, min_pixels=MIN_PIXELS, calls=1):
    """cp_contour_step_f64 on `device`, or its host twin (device None), over `step_arrays`' dict; the workspace pre-filled with the byte
    `fill` -> dict(poses [nplanes, 12], stats [njobs, 4], status [njobs], partials [njobs, max tiles, 30]) as NumPy arrays"""
    from casapose_amd import _lib, twin

    lib = _lib.load()
    njobs, nplanes, H, W = len(a["jobs"]), len(a["planes"]), a["H"], a["W"]
    size = int(lib.cp_contour_step_workspace_bytes(njobs, H, W))
    assert size > 0 and size % (30 * 8 * njobs) == 0
    stream = None
    if device is not None:
        import torch

        stream = torch.cuda.current_stream(device).cuda_stream
    arg = {k: twin.array(a[k], a[k].dtype, device) for k in ("planes", "records", "fields", "cams", "jobs")}
    arg["poses"] = twin.array(a["poses"].copy(), np.float64, device)           # rewritten in place: the caller's stay as they are
    out = twin.alloc(dict(stats=((njobs, 4), np.float64), status=((njobs,), np.int32)), device)
    work = twin.array(np.full(size, fill, np.uint8), np.uint8, device)
    for _ in range(calls):
        twin.call("cp_contour_step_f64", arg["planes"], arg["records"], nplanes, H, W, arg["fields"], len(a["fields"]), arg["cams"], len(a["cams"]),
                  arg["jobs"], njobs, float(a["offset"]), float(damping), int(min_pixels), int(update), int(split), arg["poses"], out["stats"], out["status"], work, size,
                  host=device is None, stream=stream)
    back = lambda t: t if device is None else t.cpu().numpy()   # noqa: E731
    return dict(poses=back(arg["poses"]), stats=back(out["stats"]), status=back(out["status"]),
                partials=back(work).view(np.float64).reshape(njobs, -1, 30))


def tiles_of(a, tile):
    """the tiles each job's clipped box has (0 for an empty one, -1 for a refused job)"""
    out = []
    for m, p, f, g in a["jobs"].tolist():
        if not (0 <= m < len(a["cams"]) and 0 <= p < len(a["planes"]) and 0 <= f < len(a["fields"]) and 1 <= g <= 255):
            out.append(-1)
            continue
        x, y, w, h = a["records"][p, 2:6].tolist()
        x0, y0, x1, y1 = max(x, 1), max(y, 1), min(x + w, a["W"] - 2), min(y + h, a["H"] - 2)
        out.append(0 if w < 0 or h < 0 or x0 > x1 or y0 > y1 else -(-(x1 - x0 + 1) * (y1 - y0 + 1) // tile))
    return out


def job_sums(got, n, tiles):
    """job n's 28 sums and two counts from its tile records, added in index order"""
    s = np.zeros(30)
    for t in range(tiles):
        s = s + got["partials"][n, t]
    return s[:28], int(s[28]), int(s[29])


def same_bytes(a, b, tiles, what=""):
    """the results of two runs of one step are the same bytes: poses, stats, status and every job's tile records"""
    for k in ("poses", "stats", "status"):
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differ" % (what, k)
    for n, t in enumerate(tiles):
        if t > 0:
            assert a["partials"][n, :t].tobytes() == b["partials"][n, :t].tobytes(), "%s: the tile records of job %d differ" % (what, n)


def check_against_reference(a, got, tile):
    """counts equal; every sum within N 2^-52 sum |term| (the bound of adding N fp64 terms in any order, N = the used pixels); the updated
    pose within 64 eps cond(A_damped) |xi| of the
    reference's solve of the twin's own sums, every entry of R and t alike.  -> (worst sum error / bound, pixels with e = 0)"""
    tiles = tiles_of(a, tile)
    worst, zeros = 0.0, 0
    for n, (m, p, f, g) in enumerate(a["jobs"].tolist()):
        if tiles[n] < 0:
            continue
        gg, ee, contour = CR.terms(a["planes"][p], a["fields"][f], a["cams"][m], g, a["offset"])
        want = CR.sums(gg, ee, contour)
        zeros += int((ee == 0).sum())
        s, used, cont = job_sums(got, n, tiles[n])
        assert used == want["count"] == got["stats"][n, 0] and cont == want["contour"] == got["stats"][n, 2], (n, used, want["count"], cont, want["contour"])
        iu = np.triu_indices(6)
        value = np.concatenate([want["A"][iu], want["b"], [want["rr"]]])
        bound = max(used, 1) * EPS * np.concatenate([want["absA"][iu], want["absb"], [want["rr"]]])
        assert (np.abs(s - value) <= bound).all(), (n, used, np.abs(s - value) / np.maximum(bound, 1e-300))
        assert got["stats"][n, 3] == s[27]
        if used:
            worst = max(worst, float((np.abs(s - value) / np.maximum(bound, 1e-300)).max()))
        status, _ = IR.solve(want, DAMPING, MIN_PIXELS)
        assert got["status"][n] == status, (n, got["status"][n], status)
        before = a["poses"][p].reshape(3, 4)
        if status != IR.OK:
            assert np.array_equal(got["poses"][p], a["poses"][p])
            continue
        A = np.zeros((6, 6))
        A[iu] = s[:21]
        A = A + np.triu(A, 1).T
        M = IR.damped(A, DAMPING)
        xi = np.linalg.solve(M, s[21:27])
        tol = 64 * EPS * np.linalg.cond(M) * np.linalg.norm(xi)
        diff = np.abs(got["poses"][p].reshape(3, 4) - IR.update(before, xi))
        assert diff.max() <= tol, (n, diff.max(), tol)
        assert abs(got["stats"][n, 1] - np.sqrt(s[27] / used)) <= 4 * EPS * got["stats"][n, 1]
    return worst, zeros


CASES = {"block": lambda: CC.block(), "block 37 x 50": lambda: CC.block(37, 50), "others": CC.others, "two images": CC.two_images,
         "300 jobs": CC.many_jobs, "unchanged": CC.unchanged}
_arrays = {}


def arrays_of(name, tile):
    if name not in _arrays:
        _arrays[name] = crafted(tile) if name == "crafted" else step_arrays(CASES[name]())
    return _arrays[name]


@pytest.mark.parametrize("name", list(CASES) + ["crafted"])
def test_twin_step_against_reference(hip_lib, name):
    tile = hip_lib.cp_contour_tile()
    a = arrays_of(name, tile)
    got = run_step(a)
    worst, zeros = check_against_reference(a, got, tile)
    print("%s: %d jobs, tiles %s, worst sum error / bound %.3f, %d used pixels with e = 0" % (name, len(a["jobs"]), sorted(set(tiles_of(a, tile))), worst, zeros))
    solved = got["status"] == 0
    assert solved.any() and not np.array_equal(got["poses"][a["jobs"][solved, 1]], a["poses"][a["jobs"][solved, 1]])
    slots = np.ones(len(a["poses"]), bool)
    slots[a["jobs"][solved, 1]] = False
    assert np.array_equal(got["poses"][slots], a["poses"][slots])          # no other pose is written
    if name == "crafted":
        assert tiles_of(a, tile) == [1, 3, 1, 0, 0] and got["status"].tolist() == [0, 0, 0, 1, 1]
        assert zeros > 0                                                     # contour pixels on their seed: counted, and no sum changed (above)
    if name == "unchanged":
        assert got["status"].tolist() == CC.unchanged()["want"].tolist()


@pytest.mark.parametrize("name", ["block 37 x 50", "crafted"])
def test_twin_does_not_depend_on_the_workspace_or_the_split(hip_lib, name):
    tile = hip_lib.cp_contour_tile()
    a = arrays_of(name, tile)
    first = run_step(a, fill=0x00)
    for fill, split in ((0xFF, 1), (0xA5, 3), (0x00, 64)):
        same_bytes(run_step(a, fill=fill, split=split), first, tiles_of(a, tile), "fill %#x, split %d" % (fill, split))
    evaluated = run_step(a, update=0)
    assert np.array_equal(evaluated["poses"], a["poses"]) and evaluated["stats"].tobytes() == first["stats"].tobytes()
    assert evaluated["status"].tobytes() == first["status"].tobytes()


def test_twin_refuses_jobs_out_of_range_and_reads_nothing_for_them(hip_lib):
    tile = hip_lib.cp_contour_tile()
    a = dict(arrays_of("crafted", tile))
    good = run_step(a)
    n, big = len(a["planes"]), 2 ** 31 - 1
    a["jobs"] = np.concatenate([a["jobs"][:2], np.array([(3, 0, 0, 3), (-1, 0, 0, 3), (0, n, 0, 3), (0, -1, 0, 3), (0, 2, 3, 3), (0, 2, -1, 3), (big, big, big, 3),
                                                          (0, 2, 0, 0), (0, 2, 0, 256), (0, 2, 0, -1)], np.int32)])
    got = run_step(a)
    assert got["status"].tolist() == [0, 0] + [3] * 10 and not got["stats"][2:].any()
    assert got["stats"][:2].tobytes() == good["stats"][:2].tobytes() and got["poses"].tobytes()[:2 * 96] == good["poses"].tobytes()[:2 * 96]
    assert np.array_equal(got["poses"][2:], a["poses"][2:])
    assert (got["partials"][2:].view(np.uint8) == 0xA5).all()              # not a word of a refused job's records is written


# ---- the whole loop ----------------------------------------------------------------------------------------------------------------------
def refiner_of(case, device=None, **kw):
    from casapose_amd.pose_estimation.mask_refine import DeviceMaskRefiner

    return DeviceMaskRefiner([m[0] for m in case["meshes"]], [m[1] for m in case["meshes"]], device, CC.NEAR, CC.FAR, sample_offset=CC.SAMPLE_OFFSET, **kw)


def refine(case, device=None, **kw):
    r = refiner_of(case, device)
    labels = case["labels"]
    if device is not None:
        import torch

        labels = torch.from_numpy(np.array(labels)).to(device)
    return r.refine(case["poses"], case["K"], case["obj"], case["img"], labels, case["label_of"], host=device is None, **kw) + (r,)


@pytest.mark.parametrize("name", ["block", "block 37 x 50", "others", "two images", "unchanged"])
def test_host_loop_against_the_references_loop(name):
    case = CASES[name]()
    want_poses, want_status, want_stats, _ = CC.reference_loop(case)
    poses, info, refiner = refine(case)
    assert np.array_equal(info["status"], want_status), (info["status"], want_status)
    assert info["status_names"][1] == "few_pixels" and refiner.last_renders == 9 * len(poses)
    assert np.array_equal(info["pixels_first"], want_stats[:, 0, 0]) and np.array_equal(info["pixels_last"], want_stats[:, -1, 0])
    assert np.array_equal(info["step_stats"][:, :, 2].T, want_stats[:, :, 2])                  # the contour pixels of every pass
    np.testing.assert_allclose(info["rms_first"], want_stats[:, 0, 1], rtol=1e-9)
    kept = info["status"] != 0
    assert np.array_equal(poses[kept], case["poses"][kept])                # rejected: the input, bit for bit
    if name.startswith("block") or name == "two images":
        assert (~kept).sum() >= len(poses) - 1
        ok = CC.inside(case, want_poses) & ~kept
        assert ok.sum() == (~kept).sum() and CC.inside(case, poses)[~kept].all(), CC.errors(case, poses)


def test_host_loop_does_not_depend_on_the_chunks(hip_lib):
    """300 estimates of one image are two render frames of 256 slots: one chunk under the default cap, two under a cap of one frame"""
    case = CC.many_jobs()
    one_frame = (int(hip_lib.cp_render_masks_workspace_bytes(1, 256, 37, 50)) + int(hip_lib.cp_contour_step_workspace_bytes(256, 37, 50)) +
                 2 * int(hip_lib.cp_mask_edt_workspace_bytes(256, 37, 50)))
    whole, info_whole, one = refine(case, iterations=2)
    cut, info_cut, two = refine(case, iterations=2, workspace_cap=one_frame + 100)
    assert one.last_chunks == 1 and two.last_chunks == 2 and whole.tobytes() == cut.tobytes()
    assert one.last_fields == 1 and two.last_fields == 2 and one.last_renders == 3 * 300
    for k in ("status", "step_status", "step_stats"):
        assert info_whole[k].tobytes() == info_cut[k].tobytes(), k
    assert (info_whole["status"] == 0).sum() > 200
    with pytest.raises(ValueError, match="workspace cap"):
        refine(case, iterations=2, workspace_cap=one_frame - 1)


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from casapose_amd import _lib

    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    i, d, p, z = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    edt, step = [p, i, i, i, p, i, i, p, p, p, z], [p, p, i, i, i, p, i, p, i, p, i, d, d, i, i, i, p, p, p, p, z]
    assert table["cp_contour_tile"] == (C.c_int, []) and table["cp_mask_edt_workspace_bytes"] == (z, [i, i, i])
    assert table["cp_contour_step_workspace_bytes"] == (z, [i, i, i])
    assert table["cp_mask_edt_u16"] == (C.c_int, edt + [p]) and table["cp_mask_edt_host_u16"] == (C.c_int, edt)
    assert table["cp_contour_step_f64"] == (C.c_int, step + [p]) and table["cp_contour_step_host_f64"] == (C.c_int, step)
    assert _lib.POINTEES["cp_mask_edt_u16"] == ("uint8_t", None, None, None, "int32_t", None, None, "uint16_t", "int32_t", "void", None, "void")
    assert _lib.POINTEES["cp_contour_step_f64"][5] == "uint16_t"
    assert _lib.host_twin("cp_mask_edt_u16") == "cp_mask_edt_host_u16" and _lib.host_twin("cp_contour_step_f64") == "cp_contour_step_host_f64"
    assert set(_lib.TWIN_STEPS) == {"cp_depth_icp_step_f64", "cp_contour_step_f64", "cp_mask_edt_u16"} and _lib.ABI_VERSION == 302
    tile = hip_lib.cp_contour_tile()
    assert tile >= 64 and tile % 64 == 0
    assert hip_lib.cp_contour_step_workspace_bytes(3, 48, 64) == 3 * -(-46 * 62 // tile) * 30 * 8
    assert hip_lib.cp_contour_step_workspace_bytes(1, 2, 2) == 30 * 8 and hip_lib.cp_contour_step_workspace_bytes(0, 4, 4) == 0
    assert hip_lib.cp_mask_edt_workspace_bytes(3, 48, 64) == 3 * 48 * 64 * 2 and hip_lib.cp_mask_edt_workspace_bytes(1, 16385, 4) == 0
    assert hip_lib.cp_mask_edt_workspace_bytes(4096, 16384, 16384) == 0                       # more row blocks than a grid holds
    assert hip_lib.cp_mask_edt_workspace_bytes(8388607, 1, 16384) == 8388607 * 16384 * 2      # 2^31 - 256 column blocks
    assert hip_lib.cp_mask_edt_workspace_bytes(8388608, 1, 16384) == 0                        # 2^31 column blocks, a quarter as many row blocks


def test_entry_points_refuse_bad_arguments_by_name(hip_lib):
    """CP_REQUIRE runs before anything is launched or read: no GPU is needed to be refused"""
    a = np.zeros(256, np.float64)
    p = a.ctypes.data
    for symbol in ("cp_mask_edt_u16", "cp_mask_edt_host_u16"):
        ok = [p, 1, 4, 4, p, 1, 3, p, p, p, 32]
        tail = () if "host" in symbol else (None,)
        for at, bad, word in ((0, None, b"null"), (9, None, b"null"), (1, 0, b"images"), (5, 0, b"njobs"), (2, 16385, b"H and W"), (3, 0, b"H and W"),
                              (6, 0, b"gate"), (6, 256, b"gate"), (10, 31, b"workspace_bytes"), (8, p + 2, b"4-byte"), (7, p + 1, b"2-byte")):
            args = list(ok)
            args[at] = bad
            assert getattr(hip_lib, symbol)(*args, *tail) == -1, word
            message = hip_lib.cp_last_error()
            assert word in message and symbol.encode() in message, (word, message)
    for symbol in ("cp_contour_step_f64", "cp_contour_step_host_f64"):
        ok = [p, p, 1, 4, 4, p, 1, p, 1, p, 1, 0.5, 1e-6, 24, 1, 1, p, p, p, p, 30 * 8]
        tail = () if "host" in symbol else (None,)
        for at, bad, word in ((0, None, b"null"), (19, None, b"null"), (2, 0, b"nplanes"), (6, 0, b"nfields"), (8, 0, b"images"), (10, 0, b"njobs"),
                              (3, 16385, b"H and W"), (11, -0.1, b"sample_offset"), (11, float("nan"), b"sample_offset"), (12, -1e-9, b"damping"),
                              (12, float("inf"), b"damping"), (13, 0, b"min_pixels"), (14, 2, b"update"), (15, 0, b"split"), (15, 65, b"split"),
                              (20, 30 * 8 - 1, b"workspace_bytes"), (7, p + 4, b"8-byte"), (5, p + 1, b"2-byte"), (18, p + 2, b"4-byte")):
            args = list(ok)
            args[at] = bad
            assert getattr(hip_lib, symbol)(*args, *tail) == -1, word
            message = hip_lib.cp_last_error()
            assert word in message and symbol.encode() in message, (word, message)


def test_refiner_without_a_device_has_no_fall_back():
    from casapose_amd._lib import CasaposeHipError
    from casapose_amd.pose_estimation import depth_refine, mask_refine

    assert mask_refine.keep_rule is depth_refine.keep_rule and mask_refine.STATUS_NAMES is depth_refine.STATUS_NAMES
    case = CC.unchanged()
    r = refiner_of(case)
    call = lambda **kw: r.refine(case["poses"], case["K"], case["obj"], case["img"], case["labels"], case["label_of"], **kw)   # noqa: E731
    with pytest.raises(CasaposeHipError, match="no host fall-back"):
        call()
    for kw, word in ((dict(iterations=0), "iterations"), (dict(gate=0), "gate"), (dict(gate=2.5), "gate"), (dict(gate=256), "gate"),
                     (dict(damping=-1.0), "damping"), (dict(min_pixels=0), "min_pixels"), (dict(split=65), "split"), (dict(workspace_cap=1000), "workspace cap")):
        with pytest.raises(ValueError, match=word):
            call(host=True, **kw)
    with pytest.raises(ValueError, match="object_index"):
        r.refine(case["poses"], case["K"], case["obj"] + 3, case["img"], case["labels"], case["label_of"], host=True)
    with pytest.raises(ValueError, match="image_index"):
        r.refine(case["poses"], case["K"], case["obj"], case["img"] + 1, case["labels"], case["label_of"], host=True)
    with pytest.raises(ValueError, match="label_of"):
        r.refine(case["poses"], case["K"], case["obj"], case["img"], case["labels"], case["label_of"] * 0, host=True)
    with pytest.raises(ValueError, match="uint8"):
        r.refine(case["poses"], case["K"], case["obj"], case["img"], case["labels"].astype(np.int32), case["label_of"], host=True)
