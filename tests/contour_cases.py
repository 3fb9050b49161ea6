"""The scenes tests/test_gpu_mask_refine.py refines on the device and tests/test_contour_twin_host.py / tests/test_contour_reference.py check on
the CPU: for each, the estimates, the label map and the ground truth, computed once and shared, never modified.  A case is a dict of what
`DeviceMaskRefiner.refine` takes (meshes, poses [n, 3, 4], K, obj, img [n], labels [images, H, W], label_of [n]) plus gt [n, 3, 4] and cam.

The label maps are rendered from the ground truth by the renderer's host twin (sample offset 0.5, as the refiner renders): the block of
tests/icp_cases.py with label 1, an ellipsoid of label 2 in front of its right edge (an occlusion edge) and an ellipsoid of label 3 that
the right border cuts.  At 37 x 50 the lower border cuts the block as well."""
import functools

import numpy as np

import contour_reference as CR
import icp_cases as IC
import raster_reference as RR
import test_masks_twin_host as TM
import vsd_reference as VR

NEAR, FAR, CAM = IC.NEAR, IC.FAR, IC.CAM
BLOCK, OCCLUDER, CUT = 1, 2, 3          # label values
ITERATIONS = CR.ITERATIONS
SAMPLE_OFFSET = 0.5                     # the reader's masks' and DeviceMaskRefiner's

# How close the reference's loop (tests/contour_reference.py on the rasteriser's planes, 8 iterations, default gate and min_pixels) comes to the
# ground truth on the block scene, at 48 x 64 and at 37 x 50, over the kept ones of the 12 + 6 starts below: the measured worst case.  A
# silhouette says little about the distance to the camera, so the translation error is given in the image plane (x, y) and along the optical
# axis (z) separately: measured 3.1127 degrees (at 48 x 64), 2.5336 mm and 14.1108 mm (both at 37 x 50; the other size: 2.6994 degrees, 1.5099 mm,
# 8.0237 mm), from starts up to 9.87 degrees, 5.56 mm and 19.22 mm off.  The means over the 18 starts go from 4.84 degrees / 3.40 mm / 6.54 mm
# to 1.91 / 0.80 / 2.50 at 48 x 64 and to 1.65 / 1.19 / 7.34 at 37 x 50: at 25 pixels across, the silhouette fixes the position in the image
# plane and the rotation, and says little about the distance.  The thresholds are twice the worst case.
MEASURED_DEG, MEASURED_XY_MM, MEASURED_Z_MM = 3.1127, 2.5336, 14.1108
CONVERGED_DEG, CONVERGED_XY_MM, CONVERGED_Z_MM = 2.0 * MEASURED_DEG, 2.0 * MEASURED_XY_MM, 2.0 * MEASURED_Z_MM


# the starts follow tests/icp_cases.py (12 small, 6 large, the same generator), shrunk until the reference's loop keeps them (below)
SMALL_START, LARGE_START = ((2.0, 5.0), (4.0, 4.0, 12.0)), ((6.0, 10.0), (6.0, 6.0, 20.0))
OCCLUDER_AXES = (18, 15, 14)


@functools.lru_cache(maxsize=None)
def meshes():
    return [IC.block_mesh(), TM.ellipsoid(2, OCCLUDER_AXES), TM.ellipsoid(2, (30, 25, 28))]


@functools.lru_cache(maxsize=None)
def block_starts():
    rng = np.random.default_rng(2024)
    small = [IC.perturbed(IC.BLOCK_GT, rng, *SMALL_START) for _ in range(12)]
    large = [IC.perturbed(IC.BLOCK_GT, rng, *LARGE_START) for _ in range(6)]
    return small, large


def placements(W):
    """(occluder pose, cut object's pose) of an image width"""
    if W == 64:
        return RR.pose_at(CAM, 43.7, 21.3, 400.0, RR.rotation((0, 1, 1), 0.4)), RR.pose_at(CAM, 60.6, 8.7, 500.0, RR.rotation((1, 0, 1), 0.9))
    return RR.pose_at(CAM, 40.0, 22.0, 400.0, RR.rotation((0, 1, 1), 0.4)), RR.pose_at(CAM, 47.2, 30.1, 500.0, RR.rotation((1, 0, 1), 0.9))


@functools.lru_cache(maxsize=None)
def scene():
    return VR.Scene(meshes(), NEAR, FAR, SAMPLE_OFFSET)


@functools.lru_cache(maxsize=None)
def label_map(H, W, occluder_label=OCCLUDER):
    """uint8 [H, W]; occluder_label = 0 relabels the occluder to background: its boundary is then wrongly seeded"""
    occ, cut = placements(W)
    frame = dict(cam=CAM, instances=[(0, BLOCK, IC.BLOCK_GT), (1, OCCLUDER, occ), (2, CUT, cut)])
    labels, _ = scene().renderer.render_host([frame], H, W, NEAR, FAR, SAMPLE_OFFSET)
    out = labels[0].copy()
    out[out == OCCLUDER] = occluder_label
    out.setflags(write=False)
    return out


def case_of(poses, gt, obj, img, labels, label_of, **extra):
    n = len(poses)
    return IC.frozen(dict(meshes=meshes(), poses=np.stack(poses), gt=np.stack(gt), K=np.stack([IC.VC.K_of(CAM)] * n), obj=np.asarray(obj, np.int64),
                          img=np.asarray(img, np.int64), labels=np.ascontiguousarray(np.stack(labels)), label_of=np.asarray(label_of, np.int64), cam=CAM,
                          **extra))


@functools.lru_cache(maxsize=None)
def block(H=48, W=64, occluder_label=OCCLUDER):
    """the block's 12 small and 6 large starts of tests/icp_cases.py against the label map"""
    small, large = block_starts()
    n = len(small) + len(large)
    return case_of(small + large, [IC.BLOCK_GT] * n, [0] * n, [0] * n, [label_map(H, W, occluder_label)], [BLOCK] * n, small=len(small))


@functools.lru_cache(maxsize=None)
def others(H=48, W=64):
    """three starts each of the occluder (wholly visible) and of the object the border cuts, and one of the block, in one image"""
    occ, cut = placements(W)
    rng = np.random.default_rng(11)
    poses, gt, obj, lab = [], [], [], []
    for o, l, pose in ((1, OCCLUDER, occ), (2, CUT, cut)):
        for _ in range(3):
            poses.append(IC.perturbed(pose, rng, (2.0, 6.0), (4.0, 4.0, 12.0))), gt.append(pose), obj.append(o), lab.append(l)
    poses.append(block_starts()[0][0]), gt.append(IC.BLOCK_GT), obj.append(0), lab.append(BLOCK)
    return case_of(poses, gt, obj, [0] * len(poses), [label_map(H, W)], lab)


@functools.lru_cache(maxsize=None)
def two_images():
    """the first six small starts, alternating between two copies of the 37 x 50 label map (the second with the occluder relabelled)"""
    small, _ = block_starts()
    return case_of(small[:6], [IC.BLOCK_GT] * 6, [0] * 6, [0, 1] * 3, [label_map(37, 50), label_map(37, 50, 0)], [BLOCK] * 6)


@functools.lru_cache(maxsize=None)
def many_jobs():
    """37 x 50: 300 estimates of the block in one image, more than the 256 slots of a render frame"""
    rng = np.random.default_rng(5)
    poses = [IC.perturbed(IC.BLOCK_GT, rng, (1.0, 6.0), (4.0, 4.0, 12.0)) for _ in range(300)]
    return case_of(poses, [IC.BLOCK_GT] * 300, [0] * 300, [0] * 300, [label_map(37, 50)], [BLOCK] * 300)


UNCHANGED = ("off the image", "behind the camera", "far off the mask", "a label that is not in the map", "three pixels across")


@functools.lru_cache(maxsize=None)
def unchanged():
    """five estimates that must come back as they went in, each with too few pixels, after one good one (the first small start of the block)"""
    start = block_starts()[0][0]
    move = lambda dx, dy, dz: np.hstack([start[:, :3], start[:, 3:] + np.array([[dx], [dy], [dz]])])   # noqa: E731
    tiny = RR.pose_at(CAM, 12.3, 40.2, 3000.0)
    poses = [start, move(4000.0, 0.0, 0.0), move(0.0, 0.0, -2.0 * start[2, 3]), move(-110.0, 0.0, 0.0), start, tiny]
    return case_of(poses, [IC.BLOCK_GT] * 5 + [tiny], [0] * 5 + [1], [0] * 6, [label_map(48, 64)], [BLOCK] * 4 + [77, OCCLUDER],
                   want=np.array([CR.OK] + [CR.FEW] * 5))


def reference_loop(case, iterations=ITERATIONS, **kw):
    """tests/contour_reference.py's loop over a case -> (poses [n, 3, 4], status [n], stats [n, iterations + 1, 4], last poses [n, 3, 4]);
    cached per case"""
    key = (id(case), iterations, tuple(sorted(kw.items())))
    if key not in _loops:
        G = kw.get("G", CR.GATE)
        fields = {}
        got = []
        for i in range(len(case["poses"])):
            m, l = int(case["img"][i]), int(case["label_of"][i])
            if (m, l) not in fields:
                fields[m, l] = CR.field(case["labels"][m], l, G)
            got.append(CR.refine(scene(), int(case["obj"][i]), case["poses"][i], case["cam"], fields[m, l], iterations=iterations, **kw))
        _loops[key] = (np.stack([g[0] for g in got]), np.array([g[1] for g in got]), np.stack([g[2] for g in got]), np.stack([g[3] for g in got]), case)
    return _loops[key][:4]


_loops = {}


def errors(case, poses):
    """(rotation error in degrees [n], translation error in the image plane [n] and along the optical axis [n] in millimetres) against the
    case's ground truth"""
    rot = np.array([IC.IR.rotation_error_deg(p, g) for p, g in zip(poses, case["gt"])])
    dt = np.asarray(poses)[:, :, 3] - case["gt"][:, :, 3]
    return rot, np.linalg.norm(dt[:, :2], axis=1), np.abs(dt[:, 2])


# The occluder case: where the reference ends, as the mean distance of the block's vertices from their true places over the 18 starts, with the
# occluder's boundary excluded (its label kept) and wrongly seeded (its label set to 0): measured 3.335 against 8.048 mm at 48 x 64 and 7.708
# against 10.013 mm at 37 x 50 (the starts: 9.203 mm).  "Measurably worse" is taken as a quarter more.
OCCLUDER_MVD_MM = {(48, 64): (3.335, 8.048), (37, 50): (7.708, 10.013)}
OCCLUDER_WORSE = 1.25


def mean_vertex_distance(case, poses):
    return np.array([IC.IR.mean_vertex_distance(case["meshes"][int(o)][0], p, g) for o, p, g in zip(case["obj"], poses, case["gt"])])


def inside(case, poses):
    rot, xy, z = errors(case, poses)
    return (rot < CONVERGED_DEG) & (xy < CONVERGED_XY_MM) & (z < CONVERGED_Z_MM)
