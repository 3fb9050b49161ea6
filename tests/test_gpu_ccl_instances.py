"""cp_ccl_instance_labels (csrc/ccl.hip) against the SciPy restatement of its rule (tests/instance_reference.py): the slot map and the (size,
root) table are equal, word for word, on the maps of tests/ccl_cases.py and on the hand-written maps, for R in {1, 2, 4, 16}, whatever bytes the
workspace and the outputs held before.  With R = 1 the slot map is cp_ccl_filter_labels' map wherever the two rules agree and differs as
documented elsewhere.  Sizes outside the limits are refused by name before any launch."""
import functools

import numpy as np
import pytest
import torch

import ccl_cases as Cs
import ccl_reference as R
import instance_reference as IR

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
RS = (1, 2, 4, 16)


def run(lib, device, labels, objects, max_instances, min_size, fill):
    """One call on a workspace, a slot map and a table pre-filled with the byte `fill` -> (slots, inst) as NumPy arrays."""
    from casapose_amd import _lib

    b, h, w = labels.shape
    nbytes = lib.cp_ccl_instance_workspace_bytes(b, h, w, objects, max_instances)
    assert nbytes > 0
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    lab_d = torch.from_numpy(np.array(labels, dtype=np.uint8, order="C")).to(device)
    slots = torch.full_like(lab_d, fill)
    inst = torch.full((b, objects, max_instances, 2 * 4), fill, dtype=torch.uint8, device=device)
    _lib.check(lib.cp_ccl_instance_labels(lab_d.data_ptr(), b, h, w, objects, max_instances, int(min_size), ws.data_ptr(), slots.data_ptr(),
                                          inst.data_ptr(), torch.cuda.current_stream(device).cuda_stream), "cp_ccl_instance_labels")
    torch.cuda.synchronize(device)
    return slots.cpu().numpy(), inst.cpu().numpy().view("<i4").reshape(b, objects, max_instances, 2)


@functools.lru_cache(maxsize=None)
def expected(name, max_instances, min_size):
    ref = Cs.reference(name)          # the map's properties are asserted in here, on the reference
    return IR.instance_labels(ref.case.labels, ref.case.objects, max_instances, min_size, components=(ref.root, ref.sizes))


CONFIGS = [(name, m, r) for name in Cs.NAMES for m in Cs.MIN_SIZES.get(name, (50,)) for r in RS
           if not (name == "objects_254" and r > 1)]              # 254 objects: one instance each is the limit; every other map has at most 6


@pytest.mark.parametrize("name,min_size,max_instances", CONFIGS, ids=lambda v: str(v))
def test_slots_and_table_equal_the_restatement(hip_lib, device, name, min_size, max_instances):
    case = Cs.reference(name).case
    want_slots, want_inst = expected(name, max_instances, min_size)
    for fill in FILLS:
        slots, inst = run(hip_lib, device, case.labels, case.objects, max_instances, min_size, fill)
        assert np.array_equal(inst, want_inst), (name, fill)
        assert np.array_equal(slots, want_slots), (name, fill)


@pytest.mark.parametrize("name", sorted(IR.HAND))
def test_hand_written_maps(hip_lib, device, name):
    c = IR.HAND[name]()
    for fill in FILLS:
        slots, inst = run(hip_lib, device, c.labels, c.objects, c.max_instances, c.min_size, fill)
        assert np.array_equal(inst, c.inst) and np.array_equal(slots, c.slots), (name, fill)
    for r in RS:
        if c.objects * r <= 254:
            want = IR.instance_labels(c.labels, c.objects, r, c.min_size)
            got = run(hip_lib, device, c.labels, c.objects, r, c.min_size, 0xA5)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (name, r)


def filter_labels(lib, device, labels, objects, min_size):
    from casapose_amd import _lib

    b, h, w = labels.shape
    ws = torch.empty(lib.cp_ccl_workspace_bytes(b, h, w, objects), dtype=torch.uint8, device=device)
    lab_d = torch.from_numpy(np.array(labels, dtype=np.uint8, order="C")).to(device)
    out = torch.empty_like(lab_d)
    _lib.check(lib.cp_ccl_filter_labels(lab_d.data_ptr(), b, h, w, objects, int(min_size), 1, ws.data_ptr(), out.data_ptr(),
                                        torch.cuda.current_stream(device).cuda_stream), "cp_ccl_filter_labels")
    torch.cuda.synchronize(device)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", Cs.SMALL)
def test_one_instance_against_the_filter(hip_lib, device, name):
    """R = 1: the slot of object o is o.  Per (image, object), from the restatement: where the largest component has at least min_size pixels
    and is no larger than the rest of the image, both entry points keep that component.  Elsewhere they differ as the header says: an object
    larger than the rest of the image keeps its largest component here (the filter takes the histogram's second entry: nothing, or another
    component), and an object whose components are all below min_size keeps nothing here (the filter keeps the first in raster order)."""
    ref = Cs.reference(name)
    case = ref.case
    b, h, w = case.labels.shape
    min_size = 50
    slots, _ = run(hip_lib, device, case.labels, case.objects, 1, min_size, 0xA5)
    kept = filter_labels(hip_lib, device, case.labels, case.objects, min_size)
    assert np.array_equal(kept, R.filter(case.labels, case.objects, min_size, 1))
    for n in range(b):
        comps = IR.ranked(ref.root[n], ref.sizes, case.labels[n], case.objects)
        for o in range(1, case.objects + 1):
            mine, theirs = slots[n] == o, kept[n] == o
            if not comps[o]:
                assert not mine.any() and not theirs.any()
                continue
            (root, size), fg = comps[o][0], int((case.labels[n] == o).sum())
            largest = ref.root[n] == root
            if size >= min_size and size <= h * w - fg:
                assert np.array_equal(mine, largest) and np.array_equal(theirs, largest), (n, o)
            elif size >= min_size:            # larger than the rest of the image
                assert np.array_equal(mine, largest) and not (theirs & largest).any(), (n, o)
            else:                             # every component below min_size
                first = ref.root[n] == min(r for r, _ in comps[o])
                assert not mine.any() and np.array_equal(theirs, first), (n, o)


def test_bad_sizes_are_refused_by_name(hip_lib, device):
    from casapose_amd import _lib

    lab = torch.zeros(1, 16, 64, dtype=torch.uint8, device=device)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    slots = torch.full_like(lab, 0xEE)
    inst = torch.full((254 * 16 * 2,), -7, dtype=torch.int32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    for objects, r, words in ((8, 0, "max_instances"), (8, 17, "max_instances"), (8, -1, "max_instances"), (128, 2, "objects \\* max_instances"),
                              (16, 16, "objects \\* max_instances"), (255, 1, "objects \\* max_instances"), (0, 1, "bad sizes")):
        assert hip_lib.cp_ccl_instance_workspace_bytes(1, 16, 64, objects, r) == 0
        with pytest.raises(_lib.CasaposeHipError, match="cp_ccl_instance_labels: .*" + words):
            _lib.check(hip_lib.cp_ccl_instance_labels(lab.data_ptr(), 1, 16, 64, objects, r, 50, ws.data_ptr(), slots.data_ptr(), inst.data_ptr(), st),
                       "cp_ccl_instance_labels")
    with pytest.raises(_lib.CasaposeHipError, match="null pointer"):
        _lib.check(hip_lib.cp_ccl_instance_labels(lab.data_ptr(), 1, 16, 64, 8, 2, 50, None, slots.data_ptr(), inst.data_ptr(), st), "cp_ccl_instance_labels")
    torch.cuda.synchronize(device)
    assert bool((slots == 0xEE).all()) and bool((inst == -7).all())       # nothing was launched
    assert hip_lib.cp_ccl_instance_workspace_bytes(1, 16, 64, 127, 2) > 0 and hip_lib.cp_ccl_instance_workspace_bytes(1, 16, 64, 15, 16) > 0
