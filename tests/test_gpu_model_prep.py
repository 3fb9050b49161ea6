"""Keypoints and models_info from the meshes on the GPU: `cp_model_prep_f32` (csrc/models.hip) against its host twin on the cases of
tests/test_model_prep_host.py, and the BOP converter's keypoints / models_info = "generate" with renderer = "device" on top of it.

Kernel and twin run the same header (csrc/model_math.h) on the same inputs -- fp64 differences, products and sums without FMA contraction, maxima
and lowest-index arg-maxima, which do not depend on the order they are taken in -- so squared diameter, box, keypoints, indices and status are
compared bit for bit, and two launches give the same bits.

Besides the cases of the host test: three objects of 20011, 513 and 1 vertices in one call.  20011 vertices are 79 tiles and 3160 tile pairs, more
than the 1024 blocks of the diameter kernel's grid, so blocks take several pairs at the grid stride, and 20 vertices per thread of the keypoint
kernel's block; 513 vertices end in a tile of one vertex; the single vertex is refused by status (no distinct pick), with its box and a zero diameter."""
import json
import os

import numpy as np
import pytest

import test_masks_twin_host as T
import test_model_prep_host as H
from casapose_amd.data_handler import bop_converter as BC
from casapose_amd.data_handler import model_prep as MP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_kernel_matches_its_host_twin(device, name):
    meshes, K = H.CASES[name]
    want = H.host_outputs(name)
    prep = MP.ModelPrep(device)
    got = prep.outputs(meshes, K)
    H.assert_same_bits(got, want, name)
    again = prep.outputs(meshes, K)   # fresh buffers, the same bits
    H.assert_same_bits(again, got, name)


def test_refusals_come_through_the_status(device):
    """the host cases that end in a status: the kernel writes the same words and zeros, and nothing is launched for bad arguments"""
    prep, host = MP.ModelPrep(device), MP.ModelPrep(None)
    same = np.full((40, 3), 1000.0, np.float32)
    five = np.concatenate([H.cloud(5, 2), H.cloud(5, 2)])
    meshes = {"ok": H.cloud(20, 1), "flat": same, "none": np.zeros((0, 3), np.float32), "five": five, "after": H.cloud(9, 3)}
    got, want = prep.outputs(meshes, 7), host.outputs(meshes, 7, host=True)
    assert want["status"].tolist() == [MP.ST_OK, MP.ST_TOO_FEW, MP.ST_BAD_COUNT, MP.ST_TOO_FEW, MP.ST_OK]
    H.assert_same_bits(got, want, "refusals")
    with pytest.raises(ValueError, match="flat.*too few distinct vertices"):
        prep.prepare(meshes, 7)
    with pytest.raises(ValueError, match="no_points"):
        prep.prepare({"ok": H.cloud(20, 1)}, 33)


def test_many_blocks_and_pairs_match_the_twin(device):
    meshes = {"large": H.cloud(20011, 11), "odd": H.cloud(513, 12), "one": H.cloud(1, 13)}
    assert 79 * 80 // 2 > 1024   # tile pairs of the large object against the diameter kernel's grid
    prep = MP.ModelPrep(device)
    want = MP.ModelPrep(None).outputs(meshes, 9, host=True)
    assert want["status"].tolist() == [MP.ST_OK, MP.ST_OK, MP.ST_TOO_FEW] and want["diameter_sq"][2] == 0.0 and want["diameter_sq"][0] > want["diameter_sq"][1] > 0
    got = prep.outputs(meshes, 9)
    H.assert_same_bits(got, want, "many blocks")
    H.assert_same_bits(prep.outputs(meshes, 9), got, "many blocks, again")
    results = prep.prepare({k: meshes[k] for k in ("large", "odd")}, 9)
    assert results["large"]["diameter"] == float(np.sqrt(want["diameter_sq"][0])) and results["odd"]["keypoint_indices"].tolist() == want["indices"][1].tolist()


def test_converter_on_the_device_writes_what_the_host_writes(device, tmp_path):
    meshes, _ = H.write_bare_tree(tmp_path / "bop")
    for which in ("host", "device"):
        BC.generate_data(str(tmp_path / "bop"), str(tmp_path / which), H.generate_settings(renderer=which), model_folder="models",
                         model_folder_out="models", image_folder="test")
    H.check_generated_tree(tmp_path / "device", meshes, "device")
    for sub in [os.path.join("test", "000002", "rgb")] + [os.path.join("models", n) for n in T.NAMES] + ["models"]:
        names = sorted(n for n in os.listdir(tmp_path / "host" / sub) if os.path.isfile(tmp_path / "host" / sub / n))
        assert names == sorted(n for n in os.listdir(tmp_path / "device" / sub) if os.path.isfile(tmp_path / "device" / sub / n)) and names
        for n in names:
            assert open(tmp_path / "host" / sub / n, "rb").read() == open(tmp_path / "device" / sub / n, "rb").read(), (sub, n)
    assert json.load(open(tmp_path / "device" / "models" / "models_info.json"))["obj_000005"]["diameter"] > 60
