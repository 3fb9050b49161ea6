"""The rendered scenes tests/test_pose_verify_host.py scores on the CPU and tests/test_gpu_pose_verify.py on the device: the block scene of
tests/contour_cases.py (a block, an ellipsoid in front of its right edge, an ellipsoid the right border cuts) at 48 x 64 and at 37 x 50, with
the label map and the directions rendered from the truth -- every labelled pixel holds, per keypoint, the unit direction to its object's
projected keypoint, turned by N(0, 0.05 rad) -- and a two-instance scene for the slot path.  Built once, never modified."""
import functools

import numpy as np

import contour_cases as CC
import raster_reference as RR

CAM, NEAR, FAR = CC.CAM, CC.NEAR, CC.FAR
KP = 9
LD, DIR_OFF = 2 * KP + 2, 1            # a record with a word in front of and a word behind the directions
TURN_SIGMA = 0.05                      # radians
SIZES = ((48, 64), (37, 50))


@functools.lru_cache(maxsize=None)
def keypoints3d():
    """float64 [3, 9, 3]: per mesh the centre and the eight corners of its box"""
    out = []
    for verts, _ in CC.meshes():
        lo, hi = np.min(verts, axis=0).astype(np.float64), np.max(verts, axis=0).astype(np.float64)
        corners = [[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)]
        out.append(np.array([(lo + hi) / 2] + corners))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def project(pose, points):
    """[kp, 2] as (y, x) pixels, fp64"""
    X = points @ pose[:, :3].T + pose[:, 3]
    fx, fy, cx, cy = CAM
    return np.stack([fy * X[:, 1] / X[:, 2] + cy, fx * X[:, 0] / X[:, 2] + cx], axis=-1)


def truth(W):
    """[(object, label, pose)] of an image width"""
    occ, cut = CC.placements(W)
    return [(0, CC.BLOCK, CC.IC.BLOCK_GT), (1, CC.OCCLUDER, occ), (2, CC.CUT, cut)]


def field_of(labels, kp_of_label, seed):
    """float32 [H, W, LD]: on a pixel of label l the unit directions to kp_of_label[l] [kp, 2], turned by N(0, TURN_SIGMA); N(0, 1) words elsewhere"""
    rng = np.random.default_rng(seed)
    H, W = labels.shape
    field = rng.normal(0, 1, (H, W, LD)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for l, kps in kp_of_label.items():
        on = labels == l
        for k in range(KP):
            ey, ex = kps[k, 0] - (yy + 0.5), kps[k, 1] - (xx + 0.5)
            angle = np.arctan2(ey, ex) + rng.normal(0, TURN_SIGMA, (H, W))
            field[..., DIR_OFF + 2 * k][on], field[..., DIR_OFF + 2 * k + 1][on] = np.sin(angle)[on], np.cos(angle)[on]
    return field


@functools.lru_cache(maxsize=None)
def scene(H, W):
    """dict(labels uint8 [1, H, W], field float32 [1, H, W, LD], truth) of the block scene"""
    labels = CC.label_map(H, W)
    t = truth(W)
    field = field_of(labels, {l: project(pose, keypoints3d()[o]) for o, l, pose in t}, 100 + W)
    return CC.IC.frozen(dict(labels=np.ascontiguousarray(labels[None]), field=field[None], truth=t))


def pixel_width(obj, pose):
    p = project(pose, np.asarray(CC.meshes()[obj][0], np.float64))
    return float(p[:, 1].max() - p[:, 1].min())


def shifted(obj, pose):
    """the pose moved to the right by a quarter of the object's width in pixels (to the left where that leaves the image sooner)"""
    fx = CAM[0]
    out = np.array(pose, np.float64)
    out[0, 3] += 0.25 * pixel_width(obj, pose) * pose[2, 3] / fx
    return out


def half_turn(pose):
    """the pose turned by 180 degrees about the viewing ray through the model's origin: the origin stays where it projects"""
    A = RR.rotation(pose[:, 3], np.pi)
    return np.concatenate([A @ pose[:, :3], pose[:, 3:]], axis=1)


def candidates(H, W):
    """[(name, object whose label is verified, object rendered, pose)] -- per object of the scene the truth and three wrong estimates"""
    t = truth(W)
    out = []
    for o, l, pose in t:
        other = t[(o + 1) % 3]
        out += [("truth", o, o, pose), ("shifted", o, o, shifted(o, pose)), ("half turn", o, o, half_turn(pose)), ("another object", o, other[0], other[2])]
    return out


def verify_candidate(verifier, H, W, cand, host=True, device=None, **kw):
    """the candidate beside the true poses of the scene's other two objects, as the estimates of one image -> its row of verify()'s result"""
    s = scene(H, W)
    _, o, rendered, pose = cand
    rest = [(ro, rl, rp) for ro, rl, rp in s["truth"] if ro != o]
    poses = np.stack([pose] + [rp for _, _, rp in rest])
    obj, lab = [rendered] + [ro for ro, _, _ in rest], [s["truth"][o][1]] + [rl for _, rl, _ in rest]
    labels, field = s["labels"], s["field"]
    if not host:
        import torch

        labels, field = torch.from_numpy(labels).to(device), torch.from_numpy(field).to(device)
    got = verifier.verify(poses, CC.IC.VC.K_of(CAM), obj, [0] * 3, labels, lab, field, keypoints3d(), DIR_OFF, host=host, **kw)
    return {k: v[0] for k, v in got.items()}


# ---- two instances of the block, four slots ---------------------------------------------------------------------------------------------------
R = 4
REAL, PLANTED = (1, 3), (0, 2)          # slots of object 0; file order alone would keep slot 0, a planted one, first


@functools.lru_cache(maxsize=None)
def instance_scene():
    """48 x 64, one object (the block), R = 4: slots 1 and 3 hold two real instances, slots 0 and 2 sit on blobs of the slot map -- rectangles
    with N(0, 1) directions -- with random poses there.  -> dict(slot_map uint8 [1, H, W], field, poses float64 [1, 1, R, 3, 4])"""
    H, W = 48, 64
    rng = np.random.default_rng(77)
    real = [RR.pose_at(CAM, 16.3, 14.2, 560.0, RR.rotation((1, 2, 0.5), 2.3)), RR.pose_at(CAM, 45.1, 30.7, 540.0, RR.rotation((0.3, 1, 1), 0.8))]
    frame = dict(cam=CAM, instances=[(0, REAL[0] + 1, real[0]), (0, REAL[1] + 1, real[1])])
    slot_map = CC.scene().renderer.render_host([frame], H, W, NEAR, FAR, CC.SAMPLE_OFFSET)[0][0].copy()
    blobs = {PLANTED[0]: (34, 2, 46, 12), PLANTED[1]: (4, 34, 18, 44)}           # x0, y0, x1, y1: free of the two renders
    poses = np.zeros((1, 1, R, 3, 4))
    for r, (x0, y0, x1, y1) in blobs.items():
        assert not slot_map[y0:y1 + 1, x0:x1 + 1].any()
        slot_map[y0:y1 + 1, x0:x1 + 1] = r + 1
        poses[0, 0, r] = RR.pose_at(CAM, (x0 + x1) / 2 + rng.uniform(-2, 2), (y0 + y1) / 2 + rng.uniform(-2, 2), rng.uniform(500, 600),
                                    RR.rotation(rng.normal(0, 1, 3), rng.uniform(0, np.pi)))
    for r, pose in zip(REAL, real):
        poses[0, 0, r] = pose
    field = field_of(slot_map, {r + 1: project(pose, keypoints3d()[0]) for r, pose in zip(REAL, real)}, 9)
    return CC.IC.frozen(dict(slot_map=np.ascontiguousarray(slot_map[None]), field=field[None], poses=poses))
