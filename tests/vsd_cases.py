"""The scenes tests/test_gpu_vsd.py scores on the device and tests/test_bop_vsd_host.py checks on the CPU: for each, the pairs, the sensor depth and
the reference's integers (tests/vsd_reference.py), computed once and shared, never modified."""
import functools

import numpy as np

import raster_reference as RR
import test_masks_twin_host as TM
import vsd_reference as VR

NEAR, FAR = 100.0, 2000.0
BACKGROUND = 900.0


def K_of(cam):
    return np.array([[cam[0], 0.0, cam[2]], [0.0, cam[1], cam[3]], [0.0, 0.0, 1.0]])


def sensor_depth(scene, instances, cam, H, W, occluder, zeros):
    """The nearest ground-truth depth over a background plane, rounded to uint16 millimetres, then an occluder (x0, y0, x1, y1, depth) and a
    patch of zeros (x0, y0, x1, y1) -> float32 [H, W]"""
    nearest = np.full((H, W), BACKGROUND)
    for obj, _, pose in instances:
        hit, z = VR.plane_depth(scene.plane(obj, pose, cam, H, W))
        nearest = np.where(hit, np.minimum(nearest, z), nearest)
    depth = np.rint(nearest).astype(np.uint16).astype(np.float32)
    x0, y0, x1, y1, z = occluder
    depth[y0:y1 + 1, x0:x1 + 1] = z
    x0, y0, x1, y1 = zeros
    depth[y0:y1 + 1, x0:x1 + 1] = 0.0
    return depth


def estimates_of(pose, diameter, k):
    """five estimates of one ground-truth pose: exact, shifted in depth, shifted sideways and turned, off the image, behind the camera"""
    shift = lambda dx, dy, dz: np.hstack([pose[:, :3], pose[:, 3:] + np.array([[dx], [dy], [dz]])])   # noqa: E731
    turned = np.hstack([RR.rotation((1, k + 1, 2), 0.15) @ pose[:, :3], pose[:, 3:] + np.array([[9.0 + k], [-6.0], [4.0]])])
    return [pose.copy(), shift(0.0, 0.0, (0.11 + 0.07 * k) * diameter), turned, shift(4000.0, 0.0, 0.0), shift(0.0, 0.0, -2.0 * pose[2, 3])]


@functools.lru_cache(maxsize=None)
def ellipsoids():
    """The three subdivision-2 ellipsoids of test_masks_twin_host.py in one 48 x 64 and one 37 x 50 image (an odd width, whose border cuts
    most of the third object off), five estimates per object -> dict(meshes, est, gt [n, 3, 4], K [n, 3, 3], obj, img [n], depths, diameters [n], want [n, 12],
    undecided [n])"""
    meshes, frames, _, _, _, _ = TM.three_ellipsoids()
    cam, instances = frames[0]["cam"], frames[0]["instances"]
    scene = VR.Scene(meshes, NEAR, FAR)
    diam = [2.0 * float(np.abs(np.asarray(v, np.float64)).max()) for v, _ in meshes]
    depths = [sensor_depth(scene, instances, cam, 48, 64, (38, 20, 43, 32, 480.0), (14, 18, 20, 24)),
              sensor_depth(scene, instances, cam, 37, 50, (36, 22, 41, 30, 480.0), (12, 16, 19, 21))]
    est, gt, obj, img, dia, want, und = [], [], [], [], [], [], []
    for m, depth in enumerate(depths):
        for k, (o, _, pose) in enumerate(instances):
            for e in estimates_of(pose, diam[o], k):
                c, u = scene.counts(o, e, pose, cam, depth, diam[o])
                est.append(e), gt.append(pose), obj.append(o), img.append(m), dia.append(diam[o]), want.append(c), und.append(u)
    out = dict(meshes=meshes, est=np.stack(est), gt=np.stack(gt), K=np.stack([K_of(cam)] * len(est)), obj=np.array(obj), img=np.array(img),
               depths=depths, diameters=np.array(dia), want=np.stack(want), undecided=np.array(und), renders=2 * (3 + 4 * 3),
               dropped=2 * 3 * len(meshes[0][1]))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


QUAD_N = 96      # columns 4-15 x rows 4-11: u = 2 X + 9.5 in [3.5, 15.5], v = 2 Y + 7.5 in [3.5, 11.5]


def quad():
    """16 x 20, f = 2000: a fronto-parallel 6 x 4 mm quad at 1000 mm, the estimate 1 mm = 0.125 diameters deeper (the diameter handed over is
    8 mm); c < 1.00002, so the cost lies in [0.125, 0.1250025]: above tau = 0.05 and 0.10, below 0.15 -> counts N, N, N, N, 0, ..., 0"""
    mesh = (np.array([[-3, -2, 0], [3, -2, 0], [3, 2, 0], [-3, 2, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    cam = (2000.0, 2000.0, 9.5, 7.5)
    gt = np.hstack([np.eye(3), [[0.0], [0.0], [1000.0]]])
    est = np.hstack([np.eye(3), [[0.0], [0.0], [1001.0]]])
    return dict(meshes=[mesh], est=est[None], gt=gt[None], K=K_of(cam), obj=[0], img=[0], depths=[np.full((16, 20), 1000.0, np.float32)], diameters=[8.0],
                want=np.array([[QUAD_N] * 4 + [0] * 8]))


@functools.lru_cache(maxsize=None)
def many_slots():
    """24 x 32: one ground truth and 299 distinct estimates of a small ellipsoid -> 300 render slots, more than one frame holds"""
    mesh = TM.ellipsoid(2, (40, 30, 35))
    cam = (100.0, 100.0, 15.6, 12.2)
    scene = VR.Scene([mesh], NEAR, FAR)
    gt = RR.pose_at(cam, 15.1, 11.8, 500.0, RR.rotation((1, 2, 3), 0.7))
    rng = np.random.default_rng(11)
    depth = sensor_depth(scene, [(0, 1, gt)], cam, 24, 32, (18, 8, 21, 14, 430.0), (9, 9, 11, 12))
    est = [np.hstack([gt[:, :3], gt[:, 3:] + rng.uniform(-12.0, 12.0, (3, 1)) * np.array([[1.0], [1.0], [2.5]])]) for _ in range(299)]
    both = [scene.counts(0, e, gt, cam, depth, 80.0) for e in est]
    return dict(meshes=[mesh], est=np.stack(est), gt=np.stack([gt] * 299), K=K_of(cam), obj=np.zeros(299, int), img=np.zeros(299, int), depths=[depth],
                diameters=np.full(299, 80.0), want=np.stack([c for c, _ in both]), undecided=np.array([u for _, u in both]))


def crafted(H, W, boxes, seed, images=1):
    """Hand-made planes for the entry point itself: one plane per box (x, y, w, h as a record holds it, possibly across the border), hit at
    about 70 % of the box's pixels inside the image with depths in [900, 1100]; a sensor depth in [880, 1120] with 10 % zeros per image
    -> (planes uint32 [n, H, W], records int32 [n, 11], depth float32 [images, H, W])"""
    rng = np.random.default_rng(seed)
    planes = np.full((len(boxes), H, W), VR.EMPTY, np.uint32)
    records = np.full((len(boxes), 11), -1, np.int32)
    for p, (x, y, w, h) in enumerate(boxes):
        records[p, 2:6] = (x, y, w, h)
        if w < 0 or h < 0:
            continue
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W - 1), min(y + h, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        z = rng.uniform(900.0, 1100.0, (y1 - y0 + 1, x1 - x0 + 1)).astype(np.float32).view(np.uint32)
        planes[p, y0:y1 + 1, x0:x1 + 1] = np.where(rng.random(z.shape) < 0.7, z, VR.EMPTY)
    depth = rng.uniform(880.0, 1120.0, (images, H, W)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.1] = 0.0
    return planes, records, depth


def crafted_reference(planes, depth, cams, pairs, diameters, delta=VR.DELTA, taus=VR.TAUS):
    """the reference over whole images (the planes are empty outside their boxes) -> (want [n, 2 + ntau], undecided [n]); a pair with an index
    out of range leaves zeros"""
    want, und, cache = [], [], {}
    for (m, e, g, _), d in zip(np.asarray(pairs).tolist(), diameters):
        if not (0 <= m < len(depth) and 0 <= e < len(planes) and 0 <= g < len(planes)):
            want.append(np.zeros(2 + len(taus), np.int64)), und.append(0)
            continue
        key = (m, e, g, float(d))
        if key not in cache:
            cache[key] = VR.pair_counts(planes[e], planes[g], depth[m], cams[m], d, delta, taus)
        want.append(cache[key][0]), und.append(cache[key][1])
    return np.stack(want), np.array(und)
