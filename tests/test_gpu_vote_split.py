"""cp_vote_split_labels (csrc/vote_split.hip) against the NumPy restatement of its rule (tests/vote_split_reference.py) for EQUALITY: the
accumulator, the candidate keys, the table and the slot map word for word, the peaks' positions bit for bit, whatever bytes (0x00 / 0xFF / 0xA5)
the workspace and the outputs held before.  The maps are those of tests/vote_split_cases.py: the planted scenes (48 x 64 and 60 x 80 at cell 4,
stride 1 and 2, whose conditions test_vote_split_reference.py asserts on the reference), 37 x 50 at cell 2, 4 and 8 in a batch of two different
images, R in {1, 4, 16}, the production record (ld 36, dir_off 9) and a narrow one (ld 20, dir_off 1, kp_index 3), 254 objects on 32 x 64, and one
480 x 640 image whose grid is the production one.  Every image but the 32 x 64 one has more rows than one block's band of 32, so several
blocks add to one grid in all of them."""
import ctypes as C

import numpy as np
import pytest
import torch

import vote_split_cases as Cs

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)


def run(lib, device, labels, field, dir_off, objects, max_instances, fill, kp_index=0, cell=4, vote_stride=2, min_votes=12, rel_percent=25,
        nms_radius=2, gate=4.0, min_size=50):
    """One call on a workspace and outputs pre-filled with the byte `fill` -> (slots, inst, peaks, acc, keys) as NumPy arrays."""
    from casapose_amd import _lib

    b, h, w = labels.shape
    ld = field.shape[3]
    nbytes = lib.cp_vote_split_workspace_bytes(b, h, w, objects, max_instances, cell)
    assert nbytes > 0
    off = (C.c_size_t * 3)()
    _lib.check(lib.cp_vote_split_workspace_layout(b, h, w, objects, max_instances, cell, off), "cp_vote_split_workspace_layout")
    gh, gw = -(-h // cell), -(-w // cell)
    cells = b * objects * gh * gw
    assert off[0] + 4 * cells <= off[2] and off[2] + 4 * b * objects * max_instances <= off[1] and off[1] + 8 * cells <= nbytes and off[1] % 8 == 0
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    lab_d = torch.from_numpy(np.array(labels, dtype=np.uint8, order="C")).to(device)
    field_d = torch.from_numpy(np.array(field, dtype=np.float32, order="C")).to(device)
    slots = torch.full_like(lab_d, fill)
    inst = torch.full((b, objects, max_instances, 4 * 4), fill, dtype=torch.uint8, device=device)
    peaks = torch.full((b, objects, max_instances, 2 * 4), fill, dtype=torch.uint8, device=device)
    _lib.check(lib.cp_vote_split_labels(lab_d.data_ptr(), field_d.data_ptr(), ld, dir_off, kp_index, b, h, w, objects, max_instances, cell, vote_stride,
                                        min_votes, rel_percent, nms_radius, gate, min_size, ws.data_ptr(), slots.data_ptr(), inst.data_ptr(),
                                        peaks.data_ptr(), torch.cuda.current_stream(device).cuda_stream), "cp_vote_split_labels")
    torch.cuda.synchronize(device)
    raw = ws.cpu().numpy()
    acc = raw[off[0]:off[0] + 4 * cells].view("<i4").reshape(b, objects, gh, gw)
    keys = raw[off[1]:off[1] + 8 * cells].view("<u8").reshape(b, objects, gh, gw)
    return (slots.cpu().numpy(), inst.cpu().numpy().view("<i4").reshape(b, objects, max_instances, 4),
            peaks.cpu().numpy().view("<f4").reshape(b, objects, max_instances, 2), acc, keys)


def assert_equal(got, want, what):
    slots, inst, peaks, acc, keys = got
    w_slots, w_inst, w_peaks, w_acc, w_keys = want
    assert np.array_equal(acc, w_acc), (what, "acc")
    assert np.array_equal(keys, w_keys), (what, "candidate keys")
    assert np.array_equal(inst, w_inst), (what, "inst_out")
    assert np.array_equal(peaks.view(np.uint32), w_peaks.view(np.uint32)), (what, "peaks_out")
    assert np.array_equal(slots, w_slots), (what, "slots_out")


@pytest.mark.parametrize("name", sorted(Cs.SCENES))
@pytest.mark.parametrize("sigma", Cs.SIGMAS)
@pytest.mark.parametrize("stride", (1, 2))
def test_planted_scenes_equal_the_reference(hip_lib, device, name, sigma, stride):
    s = Cs.scene(name, sigma)
    want = Cs.reference(name, sigma, stride)
    for fill in FILLS:
        got = run(hip_lib, device, s.labels, s.field, s.dir_off, s.objects, Cs.R, fill, **Cs.params(stride))
        assert_equal(got, want, (name, sigma, stride, fill))


@pytest.mark.parametrize("name", Cs.CONFIG_NAMES)
def test_maps_equal_the_reference(hip_lib, device, name):
    labels, field, dir_off, objects, r, p, want = Cs.config(name)
    for fill in FILLS if name != "production" else (0xA5,):
        assert_equal(run(hip_lib, device, labels, field, dir_off, objects, r, fill, **p), want, (name, fill))
    if name == "production":
        slots, inst = want[0], want[1]
        assert (inst[0, 0, :, 0] > 0).sum() == 3 and want[3].shape == (1, 1, 120, 160)      # the touching pair is split; the LDS grid is 76 800 bytes


@pytest.mark.parametrize("r", (1, 4, 16))
def test_every_rank_count_on_one_map(hip_lib, device, r):
    """the same map at R = 1, 4 and 16: the first ranks agree between them, and each equals the reference"""
    import vote_split_reference as VR

    labels, field, dir_off, objects, _, p, _ = Cs.config("ragged_c4")
    want = VR.split_labels(labels, field, dir_off, objects, r, stages=True, **p)
    assert_equal(run(hip_lib, device, labels, field, dir_off, objects, r, 0xA5, **p), want, r)


def test_two_calls_give_equal_bytes(hip_lib, device):
    labels, field, dir_off, objects, r, p, _ = Cs.config("narrow_r4")
    a = run(hip_lib, device, labels, field, dir_off, objects, r, 0x00, **p)
    b = run(hip_lib, device, labels, field, dir_off, objects, r, 0xFF, **p)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_an_object_without_a_peak(hip_lib, device):
    """min_votes above every cell's votes: no peak, every slot 0, every row (0, 0, -1, -1), every position (0, 0); the accumulator is still there"""
    s = Cs.scene("two_obj", 0.05)
    p = dict(Cs.params(1), min_votes=100000)
    slots, inst, peaks, acc, keys = run(hip_lib, device, s.labels, s.field, s.dir_off, s.objects, Cs.R, 0xA5, **p)
    assert not slots.any() and not keys.any() and not peaks.view(np.uint32).any()
    assert np.array_equal(inst, np.tile(np.array([0, 0, -1, -1], np.int32), (1, 2, Cs.R, 1)))
    assert np.array_equal(acc, Cs.reference("two_obj", 0.05, 1)[3])
    # an image without any labelled pixel: the blocks of the accumulate kernel end before they write, and the accumulator is zero
    empty = np.zeros_like(s.labels)
    slots, inst, peaks, acc, keys = run(hip_lib, device, empty, s.field, s.dir_off, s.objects, Cs.R, 0xFF, **Cs.params(1))
    assert not slots.any() and not acc.any() and not keys.any() and np.array_equal(inst[..., 2:], np.full((1, 2, Cs.R, 2), -1))


def test_ops_wrapper_and_defaults(hip_lib, device):
    from casapose_amd import ops

    s = Cs.scene("touch2", 0.05)
    want = Cs.reference("touch2", 0.05, 2)
    slots, inst, peaks = ops.vote_split_labels(torch.from_numpy(np.array(s.labels)).to(device), torch.from_numpy(np.array(s.field)).to(device), s.dir_off,
                                               s.objects, Cs.R, **Cs.params(2))
    assert np.array_equal(slots.cpu().numpy(), want[0]) and np.array_equal(inst.cpu().numpy(), want[1])
    assert np.array_equal(peaks.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
    with pytest.raises(TypeError, match="unknown parameter"):
        ops.vote_split_labels(slots, torch.from_numpy(np.array(s.field)).to(device), s.dir_off, s.objects, Cs.R, cells=4)


def test_bad_sizes_are_refused_by_name(hip_lib, device):
    from casapose_amd import _lib

    lab = torch.zeros(1, 16, 64, dtype=torch.uint8, device=device)
    field = torch.zeros(1, 16, 64, 36, dtype=torch.float32, device=device)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    slots = torch.full_like(lab, 0xEE)
    inst = torch.full((254 * 16 * 4,), -7, dtype=torch.int32, device=device)
    peaks = torch.full((254 * 16 * 2,), -7.0, dtype=torch.float32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    good = dict(ld=36, dir_off=9, kp_index=0, batch=1, h=16, w=64, objects=8, max_instances=4, cell=4, vote_stride=2, min_votes=12, rel_percent=25,
                nms_radius=2, gate=4.0, min_size=50)

    def call(**change):
        a = dict(good, **change)
        return hip_lib.cp_vote_split_labels(lab.data_ptr(), field.data_ptr(), a["ld"], a["dir_off"], a["kp_index"], a["batch"], a["h"], a["w"], a["objects"],
                                            a["max_instances"], a["cell"], a["vote_stride"], a["min_votes"], a["rel_percent"], a["nms_radius"], a["gate"],
                                            a["min_size"], ws.data_ptr(), slots.data_ptr(), inst.data_ptr(), peaks.data_ptr(), st)

    sizes = (dict(max_instances=0), dict(max_instances=17), dict(objects=128, max_instances=2), dict(objects=255, max_instances=1), dict(objects=0),
             dict(cell=3), dict(cell=16), dict(cell=0), dict(h=16385), dict(h=480, w=640, cell=2))
    words = ("max_instances", "max_instances", "objects \\* max_instances", "objects \\* max_instances", "must be positive", "cell", "cell", "cell",
             "at most 16384", "36864")
    for change, word in zip(sizes, words):
        a = dict(good, **change)
        assert hip_lib.cp_vote_split_workspace_bytes(a["batch"], a["h"], a["w"], a["objects"], a["max_instances"], a["cell"]) == 0, change
        with pytest.raises(_lib.CasaposeHipError, match="cp_vote_split_labels: .*" + word):
            _lib.check(call(**change), "cp_vote_split_labels")
    for change, word in ((dict(vote_stride=0), "vote_stride"), (dict(vote_stride=5), "vote_stride"), (dict(min_votes=0), "min_votes"),
                         (dict(rel_percent=-1), "rel_percent"), (dict(rel_percent=101), "rel_percent"), (dict(nms_radius=0), "nms_radius"),
                         (dict(nms_radius=5), "nms_radius"), (dict(gate=0.0), "gate"), (dict(gate=float("nan")), "gate"), (dict(gate=float("inf")), "gate"),
                         (dict(min_size=0), "min_size"), (dict(kp_index=14), "outside the pixel record"), (dict(dir_off=-1), "outside the pixel record"),
                         (dict(kp_index=-1), "outside the pixel record")):
        with pytest.raises(_lib.CasaposeHipError, match="cp_vote_split_labels: .*" + word):
            _lib.check(call(**change), "cp_vote_split_labels")
    with pytest.raises(_lib.CasaposeHipError, match="null pointer"):
        _lib.check(hip_lib.cp_vote_split_labels(lab.data_ptr(), None, 36, 9, 0, 1, 16, 64, 8, 4, 4, 2, 12, 25, 2, 4.0, 50, ws.data_ptr(), slots.data_ptr(),
                                                inst.data_ptr(), peaks.data_ptr(), st), "cp_vote_split_labels")
    torch.cuda.synchronize(device)
    assert bool((slots == 0xEE).all()) and bool((inst == -7).all()) and bool((peaks == -7.0).all())       # nothing was launched
    assert hip_lib.cp_vote_split_workspace_bytes(1, 480, 640, 8, 4, 4) > 0 and hip_lib.cp_vote_split_workspace_bytes(1, 16, 64, 254, 1, 8) > 0
