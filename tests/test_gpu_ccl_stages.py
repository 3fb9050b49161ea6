"""The connected-component filter (csrc/ccl.hip) checked stage by stage: the C ABI is called directly, what the five kernels left in the
caller's workspace is read through cp_ccl_workspace_layout and compared, exactly, with the scipy restatement of tests/ccl_reference.py --
a. labelling (`parent`), b. sizes (`count`), c. root lists (`nroots`, `roots`), d. selection (`stats`), e. the kept label map.  The maps and the
properties each is chosen for are in tests/ccl_cases.py; those properties are asserted on the reference before the kernel's result is looked at.
The workspace is pre-filled with a byte pattern: nothing may depend on what it held."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ccl_cases as Cs
import ccl_reference as R

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)


def run_filter(lib, device, labels, objects, min_size, rank, fill):
    """One call of cp_ccl_filter_labels on a workspace pre-filled with the byte `fill`; everything it left behind, as NumPy arrays."""
    from casapose_amd import _lib

    b, h, w = labels.shape
    hw = h * w
    offs = (C.c_size_t * 5)()
    _lib.check(lib.cp_ccl_workspace_layout(b, h, w, objects, offs), "cp_ccl_workspace_layout")
    nbytes = lib.cp_ccl_workspace_bytes(b, h, w, objects)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
    assert ws.data_ptr() % 64 == 0
    lab_d = torch.from_numpy(np.array(labels, dtype=np.uint8, order="C")).to(device)      # a copy: the cases' maps are read-only
    out = torch.full_like(lab_d, 0xEE)
    _lib.check(lib.cp_ccl_filter_labels(lab_d.data_ptr(), b, h, w, objects, int(min_size), int(rank), ws.data_ptr(), out.data_ptr(),
                                        torch.cuda.current_stream(device).cuda_stream), "cp_ccl_filter_labels")
    torch.cuda.synchronize(device)
    raw = ws.cpu().numpy()
    sizes = [4 * b * hw, 4 * b * hw, 4 * b * hw, 4 * b, 8 * b * objects * 3]
    align = [4, 4, 4, 64, 64]

    def part(i, dtype, shape):
        assert offs[i] % align[i] == 0 and offs[i] + sizes[i] <= (offs[i + 1] if i < 4 else nbytes)
        return raw[offs[i]:offs[i] + sizes[i]].view(dtype).reshape(shape).copy()

    return SimpleNamespace(parent=part(0, "<i4", (b, h, w)), count=part(1, "<i4", (b * hw,)), roots=part(2, "<i4", (b, hw)),
                           nroots=part(3, "<i4", (b,)), stats=part(4, "<u8", (b, objects, 3)), out=out.cpu().numpy())


def decode(entry, n, hw):
    """a stats entry -> (which, thresholded count) in the terms of ccl_reference.select"""
    entry = int(entry)
    if entry == 0:
        return None, 0
    tie = entry & 0xFFFFFFFF
    return ("bin0" if tie == 0xFFFFFFFF else n * hw + 0xFFFFFFFE - tie), entry >> 32


@functools.lru_cache(maxsize=None)
def expected(name, min_size, rank):
    """per (image, object) the reference's selection, and the kept map built from it"""
    ref = Cs.reference(name)
    case = ref.case
    b, h, w = case.labels.shape
    hw = h * w
    order = np.argsort(ref.root.ravel(), kind="stable")            # pixels grouped by root, -1 first
    flat_root, flat_lab = ref.root.ravel()[order], case.labels.ravel()[order]
    starts = np.flatnonzero(np.r_[True, flat_root[1:] != flat_root[:-1]] & (flat_root >= 0))
    by_object = {}
    for r, o in zip(flat_root[starts].tolist(), flat_lab[starts].tolist()):
        by_object.setdefault((r // hw, o), []).append((r, int(ref.sizes[r])))
    sel = {(n, o): R.select(by_object.get((n, o), []), hw, min_size, rank) for n in range(b) for o in range(1, case.objects + 1)}
    keep_roots = np.array([which for which, _ in sel.values() if which is not None and which != "bin0"], np.int64)
    out = np.where(np.isin(ref.root, keep_roots) & (ref.root >= 0), case.labels, 0).astype(np.uint8)
    return sel, out


CONFIGS = [(name, m) for name in Cs.NAMES for m in Cs.MIN_SIZES.get(name, (50,))]


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill%02X" % f)
@pytest.mark.parametrize("rank", (1, 2), ids=lambda r: "rank%d" % r)
@pytest.mark.parametrize("name,min_size", CONFIGS, ids=lambda v: str(v))
def test_stages(hip_lib, device, name, min_size, rank, fill):
    ref = Cs.reference(name)                  # the map's properties are asserted in here, on the reference
    case = ref.case
    assert min_size in case.min_sizes
    b, h, w = case.labels.shape
    hw = h * w
    if name == "second_trip":
        assert b * hw > Cs.GRID_CAP_PIXELS
    sel, want_out = expected(name, min_size, rank)
    if name != "second_trip":                 # expected() builds the kept map its own way: the two restatements agree
        assert np.array_equal(want_out, R.filter(case.labels, case.objects, min_size, rank))
    got = run_filter(hip_lib, device, case.labels, case.objects, min_size, rank, fill)
    failed = []

    # a. labelling: the root of every pixel, -1 on background and on labels above `objects`
    if not np.array_equal(got.parent, ref.root):
        bad = np.argwhere(got.parent != ref.root)
        failed.append("a. labelling: %d pixels, first (n, y, x) = %s: parent %d, reference %d"
                      % (len(bad), bad[0].tolist(), got.parent[tuple(bad[0])], ref.root[tuple(bad[0])]))
    # b. sizes, at the reference's roots
    roots = np.flatnonzero(ref.sizes)
    if not np.array_equal(got.count[roots], ref.sizes[roots]):
        bad = roots[got.count[roots] != ref.sizes[roots]]
        failed.append("b. sizes: %d roots, first %d: count %d, reference %d" % (len(bad), bad[0], got.count[bad[0]], ref.sizes[bad[0]]))
    # c. root lists per image
    for n in range(b):
        want = roots[(roots >= n * hw) & (roots < (n + 1) * hw)]
        k = int(got.nroots[n])
        if k != len(want) or not 0 <= k <= hw or not np.array_equal(np.sort(got.roots[n, :k]), want):
            failed.append("c. root list of image %d: nroots %d, reference %d" % (n, k, len(want)))
    # d. selection: which histogram entry, and its thresholded count (absent objects: the header documents 0 = no such entry)
    for (n, o), want in sel.items():
        have = decode(got.stats[n, o - 1, 2], n, hw)
        if have != want:
            failed.append("d. selection of image %d, object %d: %s, reference %s" % (n, o, have, want))
    # e. the kept label map
    if not np.array_equal(got.out, want_out):
        failed.append("e. output: %d pixels differ" % int((got.out != want_out).sum()))
    assert not failed, " | ".join(failed[:12])
    if name in ("labels_out_of_range", "objects_254_map_with_one_object"):
        bad = case.labels > case.objects
        assert bad.any() and (got.parent[bad] == -1).all() and not got.out[bad].any()
