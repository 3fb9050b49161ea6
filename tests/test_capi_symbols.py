"""CPU checks of the C-ABI library: it builds for gfx950 without a GPU, loads, exports every
symbol that include/casapose_hip.h declares, and its host-side helpers (K layout, weight
packing, argument validation) behave as documented.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from casapose_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def declared_functions():
    text = open(os.path.join(ROOT, "include", "casapose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cp_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from casapose_amd import _lib

    names = declared_functions()
    assert len(names) >= 18
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in names:
        assert hasattr(lib, n), "header declares %s but the library does not export it" % n
        assert n in bound, "%s is exported but casapose_amd/_lib.py does not bind it" % n
    assert bound <= set(names), "bound symbols missing from the header: %s" % (bound - set(names))


def header_struct_fields(name):
    """[(field, kind)] of `typedef struct <name> { ... } <name>;` in the header, in declaration order; kind = "ptr", "int", "u32" or
    "<struct> * n"."""
    text = open(os.path.join(ROOT, "include", "casapose_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const )?(\w+)\s*(.*)", decl)
        base, rest = m.group(2), m.group(3)
        for item in rest.split(","):
            item = item.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", item)
            if arr:
                out.append((arr.group(1), "%s * %s" % (base, arr.group(2))))
            elif item.startswith("*") or base.endswith("*"):
                out.append((item.lstrip("* "), "ptr"))
            else:
                out.append((item, {"int": "int", "uint32_t": "u32"}[base]))
    return out


def ctypes_struct_fields(cls):
    kinds = {C.c_void_p: "ptr", C.c_int: "int", C.c_uint32: "u32"}
    out = []
    for n, t in cls._fields_:
        if isinstance(t, type) and issubclass(t, C.Array):
            out.append((n, "%s * %d" % ({"ConvSource": "cp_conv_source"}[t._type_.__name__], t._length_)))
        else:
            out.append((n, kinds[t]))
    return out


def test_descriptor_structs_match_the_header_field_for_field(lib):
    """The round-2 defect: cp_conv_desc grew at its tail while a documented binding kept the shorter struct.  The ctypes declarations must
    list the header's fields in the header's order with the header's kinds, and the library must report the same sizes."""
    from casapose_amd import _lib

    assert ctypes_struct_fields(_lib.ConvSource) == header_struct_fields("cp_conv_source")
    assert ctypes_struct_fields(_lib.ConvDesc) == header_struct_fields("cp_conv_desc")
    assert _lib.ConvDesc._fields_[0][0] == "struct_size"
    assert lib.cp_conv_desc_size() == C.sizeof(_lib.ConvDesc) and lib.cp_conv_source_size() == C.sizeof(_lib.ConvSource)
    assert _lib.ConvDesc().struct_size == C.sizeof(_lib.ConvDesc)


def test_ransac_state_record_matches_the_header(lib):
    """cp_ransac_state (the voter's per-object record, read back by the stage tests) is mirrored by _lib.RansacState field for field, and the
    library was compiled with the same size."""
    from casapose_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "casapose_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct cp_ransac_state \{(.*?)\} cp_ransac_state;", text, flags=re.S).group(1)
    header = [re.fullmatch(r"(int|float) (\w+)((?:\[\d+\])*)", " ".join(d.split())).groups() for d in body.split(";") if d.strip()]
    assert header == [("int", "tn", ""), ("int", "done", ""), ("int", "rounds", ""), ("float", "hyp_num", ""), ("float", "win_ratio", "[9]"),
                      ("float", "win_pts", "[9][2]")]

    def spell(t, dims=""):
        if isinstance(t, type) and issubclass(t, C.Array):
            return spell(t._type_, dims + "[%d]" % t._length_)
        return {C.c_int: "int", C.c_float: "float"}[t], dims

    assert [(spell(t)[0], n, spell(t)[1]) for n, t in _lib.RansacState._fields_] == header
    size = C.c_size_t()
    assert lib.cp_ransac_workspace_layout(1, 8, 8, 1, 9, 16, (C.c_size_t * 7)(), C.byref(size)) == 0
    assert size.value == C.sizeof(_lib.RansacState) == 4 * (4 + 9 + 18)


def test_ransac_workspace_layout_is_the_voters_own_carving(lib):
    """cp_ransac_workspace_layout (host only): seven parts in the documented order, each 256-byte aligned and large enough for its array, and
    cp_ransac_workspace_bytes still what it was -- the end of the last part plus 256 bytes of alignment slack (known answers worked out by hand)."""
    up = lambda n: (n + 255) // 256 * 256   # noqa: E731
    known = {(2, 72, 100, 4, 9, 16): 251168, (2, 72, 100, 4, 9, 48): 278816, (2, 72, 100, 4, 9, 64): 292640, (1, 12, 16, 1, 9, 16): 4356,
             (1, 12, 16, 1, 9, 128): 16132, (1, 60, 80, 8, 9, 128): 270880}
    for (b, h, w, objects, kp, hyp), total in known.items():
        offs = (C.c_size_t * 7)()
        assert lib.cp_ransac_workspace_layout(b, h, w, objects, kp, hyp, offs, None) == 0
        no = b * objects
        sizes = [no * h * 4, no * h * w * 4, no * 124, no * hyp * 9 * 2 * 4, no * hyp * 9 * 4, no * 9 * 5 * 8, no * 4]    # rowcnt .. thr
        want, p = [], 0
        for i, n in enumerate(sizes):
            if i == 6:
                p = up(p) + 4           # the 4-byte `active objects` word sits between sums and thr
            p = up(p)
            want.append(p)
            p += n
        assert list(offs) == want, (list(offs), want)
        assert lib.cp_ransac_workspace_bytes(b, h, w, objects, kp, hyp) == p + 256 == total, (b, h, w, objects, hyp, p + 256)
    assert lib.cp_ransac_workspace_layout(2, 8, 8, 1, 9, 16, None, None) == -1
    assert lib.cp_ransac_workspace_layout(2, 8, 8, 1, 8, 16, (C.c_size_t * 7)(), None) == -1 and b"keypoints" in lib.cp_last_error()


def test_ccl_workspace_layout_is_the_filters_own_carving(lib):
    """cp_ccl_workspace_layout (host only): five parts in the documented order -- parent, count, roots packed int32 arrays, nroots and stats on
    64-byte boundaries --, none overlapping the next, the last ending inside cp_ccl_workspace_bytes with the 64 bytes of slack for a base that
    the filter has to round up; known totals worked out by hand; a null pointer or bad sizes give -1."""
    up = lambda n: (n + 63) // 64 * 64   # noqa: E731
    known = {(2, 70, 200, 4): 336320, (1, 1, 1, 1): 216, (3, 601, 599, 3): 12960344, (2, 32, 64, 254): 61472, (16, 480, 640, 8): 58985600}
    for (b, h, w, objects), total in known.items():
        offs = (C.c_size_t * 5)()
        assert lib.cp_ccl_workspace_layout(b, h, w, objects, offs) == 0
        px = b * h * w
        sizes = [4 * px, 4 * px, 4 * px, 4 * b, 8 * b * objects * 3]        # parent .. stats
        assert list(offs)[:3] == [0, 4 * px, 8 * px] and offs[3] == up(12 * px) and offs[4] == up(offs[3] + 4 * b)
        assert all(offs[i] + sizes[i] <= offs[i + 1] for i in range(4))
        assert lib.cp_ccl_workspace_bytes(b, h, w, objects) == offs[4] + sizes[4] + 64 == total, (b, h, w, objects, offs[4] + sizes[4] + 64)
        # never above what the size function returned before the carve was shared: the packed arrays, both roundings, 128 bytes of slack
        assert total <= 12 * px + up(4 * b) + sizes[4] + 128
    assert lib.cp_ccl_workspace_layout(2, 8, 8, 1, None) == -1 and b"null pointer" in lib.cp_last_error()
    for bad in ((0, 8, 8, 1), (2, 0, 8, 1), (2, 8, 0, 1), (2, 8, 8, 0), (2, 8, 8, 255)):
        assert lib.cp_ccl_workspace_layout(*bad, (C.c_size_t * 5)()) == -1 and b"bad sizes" in lib.cp_last_error(), bad


def test_pose_loss_workspace_layouts_are_the_losses_own_carving(lib):
    """cp_pose_loss_workspace_layout / cp_pose_loss_sep_workspace_layout (host only): the parts in the documented order, aligned for their types,
    none overlapping the next (the per-object arrays with room for 64 objects per image), the last ending inside *_workspace_bytes, whose totals are
    what they were before the carve was shared -- label map and counts rounded up to 256 bytes, 256 spare bytes (known answers worked out by hand)."""
    up = lambda n: (n + 255) // 256 * 256   # noqa: E731
    known = {(2, 24, 32): 3712, (1, 5, 7): 1600, (2, 260, 508): 266368, (16, 480, 640): 4929024, (65, 1, 1): 55104}
    for (b, h, w), total in known.items():
        offs = (C.c_size_t * 5)()
        assert lib.cp_pose_loss_workspace_layout(b, h, w, offs) == 0
        px = b * h * w
        sizes = [px, 4 * b, 8 * b * 64, 4 * b * 64, b * 64]                  # fg, count, objsum, objcnt, bad
        assert list(offs) == [0, up(px), up(px) + up(4 * b), up(px) + up(4 * b) + 512 * b, up(px) + up(4 * b) + 768 * b]
        assert all(offs[i] + sizes[i] <= offs[i + 1] for i in range(4)) and offs[1] % 4 == 0 and offs[2] % 8 == 0 and offs[3] % 4 == 0
        assert lib.cp_pose_loss_workspace_bytes(b, h, w) == offs[4] + sizes[4] + 256 == total, (b, h, w, offs[4] + sizes[4] + 256)
        assert total == up(px) + up(4 * b) + b * 64 * 13 + 256                # the expression the size function held before
    assert lib.cp_pose_loss_workspace_layout(2, 8, 8, None) == -1 and b"null pointer" in lib.cp_last_error()
    for bad in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (2, 32768, 32768)):
        assert lib.cp_pose_loss_workspace_layout(*bad, (C.c_size_t * 5)()) == -1 and b"bad shape" in lib.cp_last_error(), bad
    known = {(2, 24, 32, 4): 1824, (1, 5, 7, 2): 520, (2, 516, 512, 3): 528664, (16, 480, 640, 9): 4916032}
    for (b, h, w, k), total in known.items():
        offs = (C.c_size_t * 2)()
        assert lib.cp_pose_loss_sep_workspace_layout(b, h, w, k, offs) == 0
        px = b * h * w
        assert list(offs) == [0, up(px)]
        assert lib.cp_pose_loss_sep_workspace_bytes(b, h, w, k) == offs[1] + 4 * b * k + 256 == total, (b, h, w, k, offs[1] + 4 * b * k + 256)
    assert lib.cp_pose_loss_sep_workspace_layout(2, 8, 8, 3, None) == -1 and b"null pointer" in lib.cp_last_error()
    for bad in ((0, 8, 8, 3), (2, 8, 8, 1), (2, 8, 8, 65), (2, 32768, 32768, 3)):
        assert lib.cp_pose_loss_sep_workspace_layout(*bad, (C.c_size_t * 2)()) == -1 and b"bad shape" in lib.cp_last_error(), bad


def test_descriptor_of_another_abi_revision_is_refused(lib):
    """A caller built against a header with a shorter (or longer) cp_conv_desc is refused by size in every entry point that takes one."""
    from casapose_amd._lib import ConvDesc

    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.cout = 1, 8, 8, 8, 8, 32
    d.kh = d.kw = 3
    d.stride = d.dilation = d.pad = 1
    d.num_sources = 1
    d.src[0].channels = d.src[0].ld = 32
    d.src[0].data = d.weights = d.out_raw = 16
    d.out_raw_ld = 32
    for size in (0, C.sizeof(ConvDesc) - 16, C.sizeof(ConvDesc) + 8):
        d.struct_size = size
        assert lib.cp_conv2d_fwd_f32(C.byref(d), None) == -1 and b"struct_size" in lib.cp_last_error()
        assert lib.cp_conv2d_fwd_split(C.byref(d), 16, None, 3, None) == -1 and b"struct_size" in lib.cp_last_error()
        assert lib.cp_conv2d_wgrad_f32(C.byref(d), 16, 32, 16, 0, None) == -1 and b"struct_size" in lib.cp_last_error()
        assert lib.cp_conv2d_wgrad_split(C.byref(d), 16, 32, 16, 0, 3, None) == -1 and b"struct_size" in lib.cp_last_error()
        assert lib.cp_conv_selected_tile(C.byref(d)) == -1
        assert lib.cp_conv_split_applicable(C.byref(d)) == 0 and lib.cp_conv_wgrad_split_applicable(C.byref(d)) == 0
    d.struct_size = C.sizeof(ConvDesc)
    assert lib.cp_conv_split_applicable(C.byref(d)) == 1 and lib.cp_conv_wgrad_split_applicable(C.byref(d)) == 1


def test_integration_doc_binding_is_current():
    """INTEGRATION.md section 3 shows the binding a maintainer would write; it is generated from casapose_amd/_lib.py."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_integration_binding.py"), "--check"])
    assert r.returncode == 0, "INTEGRATION.md's ctypes block is stale: run python tools/gen_integration_binding.py"


def test_version_and_device_probe(lib):
    from casapose_amd import _lib

    assert lib.cp_version() == _lib.ABI_VERSION == 302
    text = open(os.path.join(ROOT, "include", "casapose_hip.h")).read()
    assert int(re.search(r"#define CP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION
    assert lib.cp_device_count() >= 0  # 0 on the CPU-only build container; never raises


def test_ktot_layout(lib):
    ch = (C.c_int * 2)
    assert lib.cp_conv_ktot(3, 3, 1, ch(64, 0)) == 9 * 64
    assert lib.cp_conv_ktot(7, 7, 1, ch(4, 0)) == 7 * 32          # 49 taps x 4 ch, 8 taps per 32-wide chunk
    assert lib.cp_conv_ktot(3, 3, 2, ch(32, 4)) == 9 * 32 + 2 * 32
    assert lib.cp_conv_ktot(1, 1, 1, ch(512, 0)) == 512


def test_weight_packing_orders_k_by_source_tap_channel(lib):
    kh = kw = 3
    c0, c1r, cout = 32, 3, 5
    w = np.arange(kh * kw * (c0 + c1r) * cout, dtype=np.float32).reshape(kh, kw, c0 + c1r, cout)
    chans, real = (C.c_int * 2)(c0, 4), (C.c_int * 2)(c0, c1r)
    ktot = lib.cp_conv_ktot(kh, kw, 2, chans)
    dst = np.full((cout, ktot), -1.0, np.float32)
    assert lib.cp_conv_pack_weights_host(w.ctypes.data, 0, kh, kw, cout, 2, chans, real, dst.ctypes.data) == 0
    for co in (0, 4):
        for t in range(9):
            ky, kx = divmod(t, 3)
            assert np.array_equal(dst[co, t * 32 : (t + 1) * 32], w[ky, kx, :32, co])      # source 0: tap-major
            base = 9 * 32 + t * 4
            assert np.array_equal(dst[co, base : base + 3], w[ky, kx, 32:35, co])           # source 1: 4 per tap
            assert dst[co, base + 3] == 0.0                                                   # padded channel
    assert (dst[:, 9 * 32 + 36 :] == 0).all()                                                # K padding
    # IHWO layout (PartialConvolution.conv_w) packs to the same rows
    dst2 = np.empty_like(dst)
    w_ihwo = np.ascontiguousarray(np.transpose(w, (2, 0, 1, 3)))
    assert lib.cp_conv_pack_weights_host(w_ihwo.ctypes.data, 1, kh, kw, cout, 2, chans, real, dst2.ctypes.data) == 0
    assert np.array_equal(dst, dst2)


def test_argument_validation_reports_errors_without_a_gpu(lib):
    from casapose_amd._lib import ConvDesc

    assert lib.cp_conv2d_fwd_f32(None, None) == -1
    assert b"descriptor is null" in lib.cp_last_error()
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.cout = 1, 8, 8, 8, 8, 4
    d.kh = d.kw = 3
    d.stride = d.dilation = 1
    d.pad = 1
    d.num_sources = 1
    d.src[0].channels = 24  # neither 4 nor a multiple of 32
    d.src[0].ld = 24
    d.src[0].data = 16
    d.weights = 16
    d.out_raw = 16
    d.out_raw_ld = 4
    assert lib.cp_conv2d_fwd_f32(C.byref(d), None) == -1
    assert b"channels must be 4 or a multiple of 32" in lib.cp_last_error()
    d.out_h = 7  # inconsistent geometry
    d.src[0].channels = d.src[0].ld = 32
    assert lib.cp_conv2d_fwd_f32(C.byref(d), None) == -1
    assert b"inconsistent" in lib.cp_last_error()
    assert lib.cp_ls_vote_f32(None, 36, 0, 9, 27, None, 1, 8, 8, 8, 9, None, None, None) == -1
    assert lib.cp_argmax_labels(16, 4, 9, 10, 16, None) == -1  # ld < classes
    # the masked Adam step needs its skip words (no silent fall-back to an unmasked step)
    assert lib.cp_adam_step_masked_f32(16, 16, 16, 16, 4, 1e-3, 0.9, 0.999, 1e-7, 1, 1.0, None, None) == -1
    assert b"cp_adam_step_masked_f32" in lib.cp_last_error()
    assert lib.cp_ls_vote_workspace_bytes(2, 8, 9) == 2 * 8 * 9 * 5 * 8


def test_f16x2_range_check_known_answers(lib):
    """cp_f16x2_range_check (round 6: the band check of the f16x2 range guard behind the C ABI): 0 inside [lo, hi] or for amax == 0, 1 with the power
    of two that brings amax into [2^10, 2^11), 2 where no power of two in [2^-24, 2^24] does or amax is not finite.  Host function: runs without a GPU."""
    lo, hi = 0.5, 65504.0 / 4.0
    r = C.c_float(7.0)
    for amax in (0.0, 0.5, 1.0, 1353.0, hi):
        assert lib.cp_f16x2_range_check(amax, lo, hi, C.byref(r)) == 0 and r.value == 1.0, amax
    for amax, want in ((0.49, 4096.0), (1e-2, 2.0 ** 17), (3e-5, 2.0 ** 26), (16377.0, 2.0 ** -3), (1e5, 2.0 ** -6), (3e3 * 100, 2.0 ** -8), (65504.0 * 4096, 2.0 ** -17)):
        st = lib.cp_f16x2_range_check(amax, lo, hi, C.byref(r))
        if want > 2.0 ** 24 or want < 2.0 ** -24:
            assert st == 2 and r.value == 1.0, (amax, st, r.value)
            continue
        assert st == 1 and r.value == want and 1024.0 <= amax * r.value < 2048.0, (amax, st, r.value)
    for bad in (float("inf"), float("nan"), -1.0, 1e-30, 3e38):
        assert lib.cp_f16x2_range_check(bad, lo, hi, C.byref(r)) == 2 and r.value == 1.0, bad
    assert lib.cp_f16x2_range_check(3.0, lo, hi, None) == 0   # the factor is optional


def test_f16x2_monitor_slot_is_per_thread_state(lib):
    import threading

    assert lib.cp_f16x2_monitor_get() is None
    assert lib.cp_f16x2_monitor_set(4096) == 0 and lib.cp_f16x2_monitor_get() == 4096
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.cp_f16x2_monitor_get()))
    t.start(); t.join()
    assert seen == [None]                      # another thread's launches are not armed
    assert lib.cp_f16x2_monitor_set(4100) == -1 and b"16-byte" in lib.cp_last_error()   # a slot is four words, 16-byte aligned
    assert lib.cp_f16x2_monitor_set(None) == 0 and lib.cp_f16x2_monitor_get() is None


def test_armed_sets_the_slot_and_always_clears_it(lib):
    """f16x2_range.armed: the one place that arms a monitor slot -- set inside the block, cleared on exit and on an exception; a falsy slot arms nothing"""
    from casapose_amd.f16x2_range import armed

    with armed(8192):
        assert lib.cp_f16x2_monitor_get() == 8192
    assert lib.cp_f16x2_monitor_get() is None
    with pytest.raises(RuntimeError):
        with armed(8192):
            raise RuntimeError("a failed launch")
    assert lib.cp_f16x2_monitor_get() is None
    for slot in (None, 0):
        with armed(slot):
            assert lib.cp_f16x2_monitor_get() is None


# ---- the binding table is derived from the header: known answers written by hand from include/casapose_hip.h as it stands ----
_I, _LL, _ULL, _F, _D, _Z = C.c_int, C.c_longlong, C.c_ulonglong, C.c_float, C.c_double, C.c_size_t


def _p(pointee):
    return (C.c_void_p, pointee)


def _known_signatures():
    from casapose_amd._lib import ConvDesc

    i, ll, f, d = (_I, None), (_LL, None), (_F, None), (_D, None)
    fl, u8, i32, vd = _p("float"), _p("uint8_t"), _p("int32_t"), _p("void")
    return {
        # name: (restype, pointee of the return, [(argtype, pointee)])
        "cp_conv2d_fwd_f32": (_I, None, [(C.POINTER(ConvDesc), "cp_conv_desc"), vd]),
        "cp_amax_f32": (_I, None, [fl, ll, ll, ll, _p("uint32_t"), vd]),
        "cp_ransac_vote_seeded_f32": (_I, None, [u8, fl, i, i, i, i, i, i, i, (_ULL, None), i, f, f, i, i, i, vd, fl, i32, vd]),
        "cp_render_masks_u8": (_I, None, [fl, i32, i, i32, i32, i, i, _p("double"), i32, i32, i32, _p("double"), i, i, i, i, d, d, d, u8, i32, vd,
                                          (_Z, None), vd]),
        "cp_bn_finalize_f32": (_I, None, [_p("double"), d, i, i, i, fl, fl, f, i, f] + [fl] * 8 + [vd]),
        "cp_conv_ktot": (_I, None, [i, i, i, _p("int")]),
        "cp_label_pyramid": (_I, None, [u8, i, i, i, _p("uint8_t*"), _p("float*"), _p("uint8_t*"), vd]),
        "cp_f16x2_weight_scale": (_F, None, [f]),
        "cp_f16x2_monitor_get": (C.c_void_p, "uint32_t", []),
        "cp_last_error": (C.c_char_p, "char", []),
        "cp_bpnp_loss_workspace_bytes": (_Z, None, [i, i, i]),
        "cp_conv_stem_split_weight_floats": (_I, None, []),
        "cp_ransac_workspace_layout": (_I, None, [i, i, i, i, i, i, _p("size_t"), _p("size_t")]),
        "cp_ccl_workspace_layout": (_I, None, [i, i, i, i, _p("size_t")]),
        "cp_pose_loss_workspace_layout": (_I, None, [i, i, i, _p("size_t")]),
        "cp_pose_loss_sep_workspace_layout": (_I, None, [i, i, i, i, _p("size_t")]),
    }


def test_derived_signatures_match_known_answers():
    from casapose_amd import _lib

    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, (restype, ret_pointee, args) in _known_signatures().items():
        assert table[name][0] is restype, name
        assert _lib.RETURN_POINTEES[name] == ret_pointee, name
        assert table[name][1] == [t for t, _ in args], name
        assert _lib.POINTEES[name] == tuple(p for _, p in args), name


def test_no_prototype_is_dropped():
    from casapose_amd import _lib

    names = [n for n, _, _ in _lib.SYMBOLS]
    assert len(names) == len(set(names)) == len(declared_functions())
    assert set(_lib.POINTEES) == set(_lib.RETURN_POINTEES) == set(names)


def test_unreadable_declarations_raise():
    from casapose_amd import _lib

    good = "int cp_a(const float* x, int n, void* stream);\n"
    assert [n for n, _, _ in _lib.parse_header(good)[0]] == ["cp_a"]
    for bad, what in ((good + "int cp_b(const float* x, int n;\nint cp_c(void);\n", "cp_b"),       # no closing parenthesis
                      (good + "int cp_b(int (*callback)(int), void* stream);\n", "cp_b"),           # a function pointer
                      (good + "int cp_b(const half_t* x, void* stream);\n", "cp_b, parameter 0"),   # an unknown type
                      (good + "cp_thing cp_b(void);\n", "cp_b, return type"),
                      (good + "int cp_b(float x[4]);\n", "cp_b, parameter 0")):
        with pytest.raises(_lib.CasaposeHipError, match=re.escape(what)):
            _lib.parse_header(bad)


def test_host_twins_are_found_in_the_header():
    from casapose_amd import _lib

    assert _lib.TWINS == {"cp_pnp_f64": "cp_pnp_host_f64", "cp_bpnp_loss_f64": "cp_bpnp_loss_host_f64",
                          "cp_render_scenes_f32": "cp_render_scenes_host_f32", "cp_render_masks_u8": "cp_render_masks_host_u8",
                          "cp_model_prep_f32": "cp_model_prep_host_f32"}
    table = {n: a for n, _, a in _lib.SYMBOLS}
    for device, host in _lib.TWINS.items():
        assert table[device] == table[host] + [C.c_void_p]
        assert _lib.POINTEES[device] == _lib.POINTEES[host] + ("void",)
    dev = "int cp_x_f32(const float* a, int n, float* out, void* stream);\n"
    assert _lib.parse_header(dev + "int cp_x_host_f32(const float* a, int n, float* out);\n")[3] == {"cp_x_f32": "cp_x_host_f32"}
    assert _lib.parse_header(dev + "int cp_x_pack_host(const float* a);\n")[3] == {}     # no type suffix, no device partner: not a twin
    for twin in ("int cp_x_host_f32(const float* a, int n, float* out, int extra);\n",        # one parameter more
                 "int cp_x_host_f32(const float* a, int n, double* out);\n",                  # another pointee
                 "int cp_x_host_f32(const float* a, int n, float* out, void* stream);\n"):    # the stream kept
        with pytest.raises(_lib.CasaposeHipError, match="cp_x_host_f32"):
            _lib.parse_header(dev + twin)
