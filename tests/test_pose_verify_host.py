"""pose_estimation/pose_verify.py without a GPU: `DevicePoseVerifier.verify(host=True)` on the synthetic scenes of tests/verify_scenes.py (label
map and directions rendered from the truth, the directions turned by N(0, 0.05 rad)), its argument checks, the two batch wrappers and the
score's formula.

In every scene the true pose must outscore each of three wrong ones -- shifted by a quarter of the object's pixel width, turned by 180 degrees
about the viewing ray, and the true pose of a different object under this object's label.  The smallest margin found (true score minus the best
wrong one) is 0.8132, on the cut ellipsoid at 48 x 64 (0.9942 against 0.1810 shifted); the true poses score 0.9878 to 0.9959."""
import numpy as np
import pytest

import contour_cases as CC
import verify_reference as VR
import verify_scenes as VS

SMALLEST_MARGIN = 0.8132


def verifier(objects=3, **kw):
    from casapose_amd.pose_estimation.pose_verify import DevicePoseVerifier

    key = (objects, tuple(sorted(kw.items())))
    if key not in _verifiers:
        m = CC.meshes()[:objects]
        _verifiers[key] = DevicePoseVerifier([v for v, _ in m], [f for _, f in m], None, near=CC.NEAR, far=CC.FAR, **kw)
    return _verifiers[key]


_verifiers = {}


def scored(H, W):
    if (H, W) not in _scored:
        _scored[H, W] = [(c, VS.verify_candidate(verifier(), H, W, c)) for c in VS.candidates(H, W)]
    return _scored[H, W]


_scored = {}


@pytest.mark.parametrize("size", VS.SIZES)
def test_the_true_pose_outscores_every_wrong_one(size):
    margins = []
    for o in range(3):
        rows = {c[0]: got for c, got in scored(*size) if c[1] == o}
        assert set(rows) == {"truth", "shifted", "half turn", "another object"}
        true = rows.pop("truth")
        assert true["score"] > 0.95 and true["iou"] > 0.95 and true["agreement"] > 0.95
        for name, got in rows.items():
            print("%d x %d object %d: truth %.4f, %s %.4f, counts %s" % (*size, o, true["score"], name, got["score"], got["counts"].tolist()))
            assert got["score"] < true["score"], (size, o, name)
            margins.append(true["score"] - got["score"])
        assert rows["another object"]["score"] == 0.0 and rows["another object"]["counts"][VR.ON_OTHER] > 0      # it lies on its own label
        assert rows["half turn"]["iou"] > 0.75 > rows["half turn"]["agreement"]                                # the silhouette alone would keep it
    assert min(margins) >= SMALLEST_MARGIN - 5e-5


def test_the_occluder_is_not_held_against_the_block():
    """the block's true pose: the occluder's estimate hides a part of the render, and what remains lies on the block's label alone"""
    cand, got = scored(48, 64)[0]
    c = got["counts"]
    assert cand[:3] == ("truth", 0, 0)
    assert c[VR.HIDDEN] > 0 and c[VR.ON_OTHER] == 0 and c[VR.ON_BACKGROUND] == 0 and c[VR.ON_LABEL] == c[VR.LABEL_PIXELS] == c[VR.RENDERED] - c[VR.HIDDEN]
    assert got["iou"] == 1.0 and 0.9 < got["visible"] < 1.0
    # without the occluder's estimate beside it nothing hides the render: those pixels lie on the occluder's label, reported and neutral
    s = VS.scene(48, 64)
    o, l, pose = s["truth"][0]
    alone = verifier().verify(pose[None], CC.IC.VC.K_of(VS.CAM), [o], [0], s["labels"], [l], s["field"], VS.keypoints3d(), VS.DIR_OFF, host=True)
    assert alone["counts"][0, VR.HIDDEN] == 0 and alone["counts"][0, VR.ON_OTHER] == c[VR.HIDDEN] and alone["iou"][0] == 1.0 and alone["visible"][0] == 1.0


def test_results_match_the_reference_formula():
    from casapose_amd.pose_estimation.pose_verify import COUNT_NAMES, score_from_counts

    assert COUNT_NAMES == ("rendered", "hidden", "on_label", "on_background", "on_other", "label_pixels", "pairs", "inliers")
    counts = np.array([(12, 2, 8, 1, 1, 10, 4, 2), (12, 2, 10, 0, 0, 11, 10, 10), (0,) * 8, (5, 5, 0, 0, 0, 7, 0, 0)])
    got, want = score_from_counts(counts), VR.score_from_counts(counts)
    for k, w in zip(("iou", "agreement", "visible", "score"), want):
        assert got[k].dtype == np.float64 and got[k].tolist() == w.tolist()
    assert got["score"].tolist() == [8 / 11 * 0.5, 10 / 11, 0.0, 0.0] and got["visible"].tolist() == [10 / 12, 10 / 12, 0.0, 0.0]


def test_cos_min_is_the_ransac_voters():
    import inspect

    from casapose_amd.pose_estimation import pose_verify, ransac_voting

    assert pose_verify.DEFAULT_COS_MIN is ransac_voting.INLIER_THRESH
    assert inspect.signature(ransac_voting.ransac_voting_layer_all_masks).parameters["inlier_thresh"].default == ransac_voting.INLIER_THRESH == 0.99
    assert inspect.signature(pose_verify.DevicePoseVerifier.verify).parameters["cos_min"].default == ransac_voting.INLIER_THRESH


@pytest.mark.parametrize("size", VS.SIZES)
def test_chunks_change_nothing(size):
    """each block scene as two images (the second with its field turned upside down); a cap of one frame's planes forces two chunks, of which
    the second holds image 1 alone"""
    from casapose_amd import _lib

    s = VS.scene(*size)
    labels, field = np.concatenate([s["labels"]] * 2), np.concatenate([s["field"], s["field"][:, ::-1].copy()])
    poses = np.stack([p for _, _, p in s["truth"]] * 2)
    obj, lab, img = [o for o, _, _ in s["truth"]] * 2, [l for _, l, _ in s["truth"]] * 2, [0, 0, 0, 1, 1, 1]
    v = verifier()
    one = v.verify(poses, CC.IC.VC.K_of(VS.CAM), obj, img, labels, lab, field, VS.keypoints3d(), VS.DIR_OFF, host=True)
    assert v.last_chunks == 1 and v.last_renders == 6
    cap = int(_lib.load().cp_render_masks_workspace_bytes(1, 3, *size))
    two = v.verify(poses, CC.IC.VC.K_of(VS.CAM), obj, img, labels, lab, field, VS.keypoints3d(), VS.DIR_OFF, host=True, workspace_cap=cap, split=7)
    assert v.last_chunks == 2 and two["counts"].tobytes() == one["counts"].tobytes()
    assert (one["counts"][:3, :6] == one["counts"][3:, :6]).all() and (one["counts"][3:, VR.INLIERS] < one["counts"][:3, VR.INLIERS]).all()
    with pytest.raises(ValueError, match="the workspace cap is"):
        v.verify(poses, CC.IC.VC.K_of(VS.CAM), obj, img, labels, lab, field, VS.keypoints3d(), VS.DIR_OFF, host=True, workspace_cap=cap - 1)


def test_argument_checks():
    from casapose_amd import _lib

    s = VS.scene(37, 50)
    o, l, pose = s["truth"][0]
    K, kps = CC.IC.VC.K_of(VS.CAM), VS.keypoints3d()
    v = verifier()
    call = lambda **kw: v.verify(**{**dict(poses=pose[None], K=K, object_index=[o], image_index=[0], labels=s["labels"], label_of=[l],   # noqa: E731
                                           field=s["field"], keypoints3d=kps, dir_off=VS.DIR_OFF, host=True), **kw})
    assert call()["counts"].shape == (1, 8)
    empty = call(poses=np.zeros((0, 3, 4)), object_index=[], image_index=[], label_of=[])
    assert empty["counts"].shape == (0, 8) and empty["score"].shape == (0,)
    for kw, word in ((dict(host=False), "built without a device"), (dict(image_index=[0, 0]), "one entry per estimate"), (dict(cos_min=1.5), "cos_min must lie in"),
                     (dict(cos_min=float("nan")), "cos_min must lie in"), (dict(split=0), "split must lie in"), (dict(split=65), "split must lie in"),
                     (dict(labels=s["labels"].astype(np.int32)), "labels is a uint8"), (dict(labels=s["labels"][0]), "labels is a uint8"),
                     (dict(field=s["field"][:, :-1]), "field is a float32"), (dict(field=s["field"].astype(np.float64)), "field is a float32"),
                     (dict(keypoints3d=kps[:2]), "keypoints3d is"), (dict(keypoints3d=np.zeros((3, 33, 3))), "keypoints3d is"),
                     (dict(dir_off=3), "do not fit"), (dict(dir_off=-1), "do not fit"), (dict(object_index=[3]), "object_index must lie in"),
                     (dict(image_index=[1]), "image_index must lie in"), (dict(label_of=[0]), "label_of must lie in"), (dict(label_of=[256]), "label_of must lie in")):
        with pytest.raises((ValueError, _lib.CasaposeHipError), match=word):
            call(**kw)
    n = 257
    with pytest.raises(ValueError, match="257 estimates; they hide each other"):
        call(poses=np.tile(pose[None], (n, 1, 1)), object_index=[o] * n, image_index=[0] * n, label_of=[l] * n)


def test_verify_estimates_of_a_batch():
    """[b, oc, 1, 3, 4] with a zero pose: score 0 for it, label o + 1 for object o, the batch's keypoints3d layout"""
    from casapose_amd.pose_estimation.pose_verify import verify_estimates

    s = VS.scene(48, 64)
    poses = np.zeros((2, 3, 1, 3, 4), np.float32)
    for o, _, pose in s["truth"]:
        poses[0, o, 0] = pose
    poses[1, 0, 0] = VS.shifted(0, s["truth"][0][2])
    labels, field = np.concatenate([s["labels"]] * 2), np.concatenate([s["field"]] * 2)
    kps = np.broadcast_to(VS.keypoints3d()[None, :, None], (2, 3, 1, VS.KP, 3))
    v = verifier()
    got = verify_estimates(v, poses, labels, field, kps, CC.IC.VC.K_of(VS.CAM), dir_off=VS.DIR_OFF, host=True)
    assert got.shape == (2, 3) and got.dtype == np.float64 and v.last_scores is got and v.last_counts.shape == (2, 3, 8)
    assert (got[0] > 0.95).all() and 0.0 < got[1, 0] < 0.3 and got[1, 1] == got[1, 2] == 0.0 and not v.last_counts[1, 1:].any()
    none = verify_estimates(v, np.zeros((2, 3, 3, 4)), labels, field, kps, CC.IC.VC.K_of(VS.CAM), dir_off=VS.DIR_OFF, host=True)
    assert none.shape == (2, 3) and not none.any() and not v.last_counts.any()


def test_real_instances_take_the_highest_scores():
    """R = 4: slots 1 and 3 hold real instances, slots 0 and 2 sit on blobs with random poses.  By file order with a constant score, slot 0 -- a
    planted one -- would be kept first; by the verified score the two real ones are"""
    from casapose_amd.pose_estimation.pose_verify import verify_instance_estimates

    s = VS.instance_scene()
    v = verifier(objects=1)
    got = verify_instance_estimates(v, s["poses"], s["slot_map"], s["field"], VS.keypoints3d()[:1], CC.IC.VC.K_of(VS.CAM), dir_off=VS.DIR_OFF, host=True)
    assert got.shape == (1, 1, VS.R) and v.last_counts.shape == (1, 1, VS.R, 8)
    order = np.argsort(-got[0, 0], kind="stable")
    print("instance scores", got[0, 0].tolist())
    assert sorted(order[:2].tolist()) == list(VS.REAL) and min(VS.PLANTED) < min(VS.REAL)
    assert got[0, 0, list(VS.REAL)].min() > 0.9 and got[0, 0, list(VS.PLANTED)].max() < 0.1
    assert (v.last_counts[0, 0, list(VS.PLANTED), VR.LABEL_PIXELS] > 100).all()       # the blobs are there; the poses do not explain them
    with pytest.raises(ValueError, match=r"poses is \[b, oc, R, 3, 4\]"):
        verify_instance_estimates(v, s["poses"][:, :, 0], s["slot_map"], s["field"], VS.keypoints3d()[:1], CC.IC.VC.K_of(VS.CAM), host=True)
