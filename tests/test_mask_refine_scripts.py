"""CASAPOSE_MASK_REFINE=1 in test_casapose.py and util_scripts/test_minimal.py: what is refused before any device work, and the switch itself.
Neither script has a line for the switch: test_casapose.py's step (training.test_step) and test_minimal.py's poses_pnp read it.  No GPU is
needed: test_step refuses a batch before its forward pass, and poses_pnp's host path runs here."""
import numpy as np
import pytest

import contour_cases as CC

IDENTITY = [0.0, 0.0, 480.0, 640.0, 0.0, 0.0, 0.0, 1.0, 640.0, 480.0]


def test_switch_is_read_like_the_uncertainty_switch(monkeypatch, capsys):
    from casapose_amd.pose_estimation import mask_refine as M

    monkeypatch.setattr(M.mask_refine_enabled, "said", False)
    monkeypatch.delenv("CASAPOSE_MASK_REFINE", raising=False)
    assert not M.mask_refine_enabled()
    monkeypatch.setenv("CASAPOSE_MASK_REFINE", "0")
    assert not M.mask_refine_enabled() and capsys.readouterr().out == ""
    monkeypatch.setenv("CASAPOSE_MASK_REFINE", "1")
    assert M.mask_refine_enabled() and M.mask_refine_enabled()
    assert capsys.readouterr().out.count("refine: mask contours") == 1              # said once


@pytest.mark.parametrize("at, value", [(0, 16.0), (1, 96.0), (4, 3.0), (5, -2.0), (6, 5.0), (7, 0.5)])
def test_offsets_that_are_not_the_identity_are_refused_by_name(at, value):
    from casapose_amd.pose_estimation.mask_refine import require_image_frame

    require_image_frame(np.array([IDENTITY, IDENTITY]))
    require_image_frame(np.array(IDENTITY, np.float32))
    bad = np.array([IDENTITY, IDENTITY])
    bad[1, at] = value
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1"):
        require_image_frame(bad)


def test_test_step_refuses_the_batch_before_the_forward_pass(monkeypatch):
    from casapose_amd.training import test_step

    class Net:      # any use of the network, the options or the loss factors would raise: the offsets are looked at first
        @property
        def device(self):
            return "cpu"

    bad = np.array([[16.0, 96.0, 448.0, 448.0, 0.0, 0.0, 0.0, 1.0, 640.0, 480.0]])
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1"):
        test_step(Net(), {"offsets": bad}, None, None, refiner=object())
    monkeypatch.setenv("CASAPOSE_MASK_REFINE", "1")                 # what test_casapose.py runs: no refiner is handed over
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1"):
        test_step(Net(), {"offsets": bad}, None, None)
    opt = type("Opt", (), {"estimate_coords": False})()
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1 needs estimate_coords"):
        test_step(Net(), {"offsets": np.array([IDENTITY])}, opt, None, refiner=object())


class Dataset:
    def __init__(self, meshes):
        self.meshes = meshes

    def generate_object_vertex_array(self):
        arr = np.zeros((len(self.meshes), max(len(m[0]) for m in self.meshes), 3), np.float32)
        for i, (v, _) in enumerate(self.meshes):
            arr[i, :len(v)] = v
        return arr, np.array([[len(m[0])] for m in self.meshes], np.int32)


def write_obj(path, verts, faces):
    with open(path, "w") as out:
        out.write("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in verts) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in faces))


def test_meshes_without_faces_are_refused_by_name(tmp_path, monkeypatch):
    from casapose_amd.pose_estimation import mask_refine as M

    def no_device(*a, **k):
        raise AssertionError("a refiner was built before the meshes were checked")

    meshes = CC.meshes()[:2]
    names = ["block", "ball"]
    for name, (v, f) in zip(names, meshes):
        (tmp_path / name).mkdir()
        write_obj(tmp_path / name / (name + ".obj"), v, f if name == "block" else [])
    monkeypatch.setattr(M, "DeviceMaskRefiner", no_device)
    with pytest.raises(ValueError, match=r"CASAPOSE_MASK_REFINE=1 needs meshes with faces.*ball\.obj"):
        M.refiner_for_dataset(Dataset(meshes), str(tmp_path), names, "cuda:0")
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1 needs a mesh for every object: lamp"):
        M.refiner_for_dataset(Dataset(meshes), str(tmp_path), ["block", "lamp"], "cuda:0")
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1 needs the objects' mesh files"):
        M.refiner_for_dataset(Dataset(meshes), "", names, "cuda:0")
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1 needs the objects' mesh files"):
        M.refiner_for_dataset(object(), str(tmp_path), names, "cuda:0")              # the built-in synthetic scenes have no mesh files


def test_refiner_for_dataset_and_refine_estimates_on_the_host(tmp_path):
    """the refiner the scripts build, driven through the host loop: the found objects are refined, the zero pose passes through"""
    from casapose_amd.pose_estimation import mask_refine as M

    meshes = CC.meshes()
    names = ["block", "occluder", "cut"]
    for name, (v, f) in zip(names, meshes):
        (tmp_path / name).mkdir()
        write_obj(tmp_path / name / (name + ".obj"), v, f)
    r = M.refiner_for_dataset(Dataset(meshes), str(tmp_path), names, None)
    assert r.objects == 3 and r.sample_offset == 0.5 and r.near < 400.0 < r.far and r.device is None
    assert np.array_equal(r.renderer.faces[0, :len(meshes[0][1])], meshes[0][1])
    case = CC.block()
    poses = np.zeros((1, 3, 1, 3, 4), np.float32)
    poses[0, 0, 0] = case["poses"][1]

    class HostRefiner:      # refine_estimates with host=True
        def __init__(self, inner):
            self.inner = inner

        def refine(self, *a, **k):
            return self.inner.refine(*a, host=True, **k)

    h = HostRefiner(r)
    got = M.refine_estimates(h, poses, case["labels"], CC.IC.VC.K_of(CC.CAM)[None])
    assert got.shape == poses.shape and got.dtype == np.float32 and not got[0, 1:].any() and h.last_info["status"].tolist() == [0]
    want, _ = r.refine(poses[0, 0].astype(np.float64), case["K"][:1], [0], [0], case["labels"], [1], host=True)
    assert got[0, 0, 0].tobytes() == want[0].astype(np.float32).tobytes() and not np.array_equal(got[0, 0, 0], poses[0, 0, 0])
    none = M.refine_estimates(h, np.zeros_like(poses), case["labels"], CC.IC.VC.K_of(CC.CAM))
    assert not none.any() and h.last_info is None


def test_environment_refiner_and_poses_pnp_refusals(tmp_path, monkeypatch):
    from casapose_amd.data_handler.vectorfield_dataset import VectorfieldDataset
    from casapose_amd.pose_estimation import mask_refine as M
    from casapose_amd.pose_estimation.pose_evaluation import poses_pnp

    meshes = CC.meshes()[:1]
    (tmp_path / "block").mkdir()
    write_obj(tmp_path / "block" / "block.obj", *meshes[0])
    verts, counts = Dataset(meshes).generate_object_vertex_array()
    opt = type("Opt", (), {"datameshes": str(tmp_path), "object": "block", "estimate_coords": True})()
    monkeypatch.setattr(M, "_refiners", {})
    monkeypatch.delenv("CASAPOSE_MASK_REFINE", raising=False)
    assert M.refiner_from_environment(opt, verts, counts, None) is None and not M._refiners
    monkeypatch.setenv("CASAPOSE_MASK_REFINE", "1")
    r = M.refiner_from_environment(opt, verts, counts, None)
    assert r is M.refiner_from_environment(opt, verts, counts, None) and r.objects == 1 and len(M._refiners) == 1
    with pytest.raises(ValueError, match="CASAPOSE_MASK_REFINE=1 needs the objects' mesh files"):          # the built-in synthetic scenes
        M.refiner_from_environment(type("Opt", (), {"datameshes": "", "object": "block"})(), None, None, None)
    # poses_pnp on keypoints that no voter returned
    kp3 = np.concatenate([meshes[0][0].mean(0, keepdims=True), meshes[0][0][:8]]).astype(np.float32)
    P = CC.IC.BLOCK_GT
    camp = kp3.astype(np.float64) @ P[:, :3].T + P[:, 3]
    yx = np.stack([CC.CAM[1] * camp[:, 1] / camp[:, 2] + CC.CAM[3], CC.CAM[0] * camp[:, 0] / camp[:, 2] + CC.CAM[2]], -1)[None, None].astype(np.float32)
    seg = np.eye(2, dtype=np.float32)[(CC.label_map(48, 64) == 1).astype(int)][None]
    args = (yx, seg, kp3[None, None, None], CC.IC.VC.K_of(CC.CAM), 1)
    with pytest.raises(ValueError, match="poses_pnp: CASAPOSE_MASK_REFINE=1 needs the keypoints tensor"):
        poses_pnp(*args, rng=np.random.default_rng(0))
    monkeypatch.delenv("CASAPOSE_MASK_REFINE")
    plain = poses_pnp(*args, rng=np.random.default_rng(0))                                                  # unset: the PnP pose, as before
    assert plain.shape == (1, 1, 1, 3, 4) and CC.IC.IR.mean_vertex_distance(meshes[0][0], plain[0, 0, 0], P) < 0.5
    assert VectorfieldDataset.last_instance is None or callable(VectorfieldDataset.last_instance)

