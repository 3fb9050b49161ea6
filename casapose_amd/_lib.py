"""ctypes binding of libcasapose_hip.so (the C ABI declared in include/casapose_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails,
`CasaposeHipError` is raised.  Build the library with `python __graft_entry__.py` (or
`make -C casapose_amd/csrc`).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

# PyTorch-ROCm ships its own libamdhip64; import it FIRST so that our library's dependency on
# the same SONAME binds to the runtime that owns torch's device context and streams (two HIP
# runtimes in one process do not share devices: launches fail with "no ROCm-capable device").
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# CASAPOSE_HIP_LIB overrides the library path (kernel-variant experiments only)
LIB_PATH = os.environ.get("CASAPOSE_HIP_LIB") or os.path.join(_HERE, "libcasapose_hip.so")


class CasaposeHipError(RuntimeError):
    pass


class ConvSource(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("channels", C.c_int),
        ("ld", C.c_int),
        ("mode", C.c_int),
        ("sel", C.c_void_p),
        ("pre_scale", C.c_void_p),
        ("pre_shift", C.c_void_p),
    ]


class ConvDesc(C.Structure):
    """cp_conv_desc of include/casapose_hip.h, field for field (tests/test_capi_symbols.py parses the header and compares).  `struct_size` is
    filled by the constructor; load() refuses a library whose sizeof(cp_conv_desc) differs from this declaration."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(ConvDesc)

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("batch", C.c_int),
        ("in_h", C.c_int),
        ("in_w", C.c_int),
        ("out_h", C.c_int),
        ("out_w", C.c_int),
        ("cout", C.c_int),
        ("kh", C.c_int),
        ("kw", C.c_int),
        ("stride", C.c_int),
        ("dilation", C.c_int),
        ("pad", C.c_int),
        ("num_sources", C.c_int),
        ("src", ConvSource * 2),
        ("weights", C.c_void_p),
        ("weights_halo", C.c_void_p),
        ("tap_label", C.c_void_p),
        ("row_scale", C.c_void_p),
        ("residual", C.c_void_p),
        ("residual_ld", C.c_int),
        ("scale", C.c_void_p),
        ("shift", C.c_void_p),
        ("epi_label", C.c_void_p),
        ("act", C.c_int),
        ("out_raw", C.c_void_p),
        ("out_raw_ld", C.c_int),
        ("out_act", C.c_void_p),
        ("out_act_ld", C.c_int),
        ("tile_hint", C.c_int),
        ("head_weights", C.c_void_p),
        ("head_out", C.c_void_p),
        ("head_cout", C.c_int),
        ("head_out_ld", C.c_int),
        ("group_rows", C.c_int),
        ("group_weight_stride", C.c_int),
        ("head_label_out", C.c_void_p),
        ("head_label_classes", C.c_int),
        ("head_prefix", C.c_void_p),
        ("head_prefix_n", C.c_int),
        ("head_prefix_ld", C.c_int),
    ]


AUG_MAX_OPS, AUG_MAX_LUTS, AUG_MAX_TAPS, AUG_NOISE_MAX, AUG_NOISE_FIELDS, AUG_FINISH_SLOT = 12, 6, 49, 16, 3, 15
AUG_LUT, AUG_HUE_SAT, AUG_FREQ_BLEND, AUG_GAUSS_NOISE, AUG_LAPLACE_NOISE, AUG_POISSON_NOISE, AUG_DROPOUT, AUG_REPLACE = range(1, 9)
AUG_BLUR_LINEAR, AUG_BLUR_MEDIAN, AUG_BLUR_BILATERAL = 9, 10, 11


class AugOp(C.Structure):
    """cp_aug_op of include/casapose_hip.h."""
    _fields_ = [("kind", C.c_int32), ("per_channel", C.c_int32), ("slot", C.c_int32), ("k", C.c_int32), ("i0", C.c_int32), ("i1", C.c_int32),
                ("f0", C.c_float), ("f1", C.c_float)]


class AugImage(C.Structure):
    """cp_aug_image of include/casapose_hip.h: one image's program for the input-pipeline kernels (csrc/augment.hip)."""
    _fields_ = [
        ("seed", C.c_uint64),
        ("src_offset", C.c_int64),
        ("src_h", C.c_int32), ("src_w", C.c_int32),
        ("crop_x", C.c_int32), ("crop_y", C.c_int32),
        ("warp", C.c_int32),
        ("n_ops", C.c_int32),
        ("affine", C.c_double * 6),
        ("brightness", C.c_float), ("contrast", C.c_float), ("noise_sigma", C.c_float),
        ("noise_fields", C.c_int32),
        ("noise_h", C.c_int32 * AUG_NOISE_FIELDS), ("noise_w", C.c_int32 * AUG_NOISE_FIELDS), ("noise_up", C.c_int32 * AUG_NOISE_FIELDS),
        ("noise_aggregate", C.c_int32),
        ("noise_sigmoid", C.c_int32),
        ("noise_threshold", C.c_float),
        ("ops", AugOp * AUG_MAX_OPS),
        ("taps", (C.c_float * AUG_MAX_TAPS) * 2),
        ("noise", (C.c_float * (AUG_NOISE_MAX * AUG_NOISE_MAX)) * AUG_NOISE_FIELDS),
        ("label_map", C.c_uint8 * 256),
        ("lut", ((C.c_uint8 * 256) * 3) * AUG_MAX_LUTS),
    ]


class RansacState(C.Structure):
    """cp_ransac_state of include/casapose_hip.h, field for field (tests/test_capi_symbols.py parses the header and compares): the RANSAC voter's
    per-(image, object) record inside its workspace, found through cp_ransac_workspace_layout."""
    _fields_ = [("tn", C.c_int), ("done", C.c_int), ("rounds", C.c_int), ("hyp_num", C.c_float), ("win_ratio", C.c_float * 9),
                ("win_pts", (C.c_float * 2) * 9)]


PLANES_F16X2 = 0x12  # CP_PLANES_F16X2: the fp16 two-way split (three products, fp32-level accuracy)

SRC_DIRECT, SRC_NEAREST_SEL, SRC_BILINEAR_X2, SRC_ZERO_INSERT_X2 = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_LEAKY01 = 0, 1, 2
TILE_AUTO, TILE_128x128, TILE_64x128, TILE_128x64, TILE_128x32, TILE_64x64, TILE_256x32, TILE_HALO, TILE_STEM = range(9)
# host-side selectors (never passed to the library): the bf16-pipe kernel of csrc/conv_hsplit.hip with 3 planes (exact fp32 split) / 1 plane (bf16)
TILE_SPLIT3, TILE_BF16, TILE_F16X2 = 100, 101, 102


# ---- the binding table, read from include/casapose_hip.h (plain C, ours: a few regular expressions are the whole front end) ----
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "casapose_hip.h")
_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "int64_t": C.c_int64, "unsigned long long": C.c_ulonglong, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_POINTEE_ONLY = ("void", "char", "int32_t", "uint8_t", "uint16_t", "uint32_t", "cp_conv_desc", "cp_aug_image")


def _parse_type(decl: str, where: str, is_return: bool = False):
    """One return type or parameter of a prototype -> (ctypes type, pointee type or None).  Pointers are c_void_p whatever they point to, except
    cp_conv_desc* (POINTER(ConvDesc)) and a returned char* (c_char_p); `name[]` is a pointer."""
    depth = decl.count("*") + decl.count("[]")
    words = re.sub(r"\*|\[\]|\bconst\b", " ", decl).split()
    bases = [" ".join(words[:n]) for n in (len(words), len(words) - 1)]   # a parameter may or may not be named
    base = next((b for b in bases if b in _SCALARS or b in _POINTEE_ONLY), None)
    if base is None or not all(re.fullmatch(r"\w+", w) for w in words):
        raise CasaposeHipError("%s: cannot read the type of `%s`" % (where, " ".join(decl.split())))
    if depth == 0:
        if base in _SCALARS:
            return _SCALARS[base], None
        if base == "void" and is_return:
            return None, None
        raise CasaposeHipError("%s: `%s` is passed by value" % (where, " ".join(decl.split())))
    if (base, depth) == ("cp_conv_desc", 1):
        return C.POINTER(ConvDesc), base
    return (C.c_char_p if is_return and (base, depth) == ("char", 1) else C.c_void_p), base + "*" * (depth - 1)


def parse_header(text: str):
    """Every function prototype of a header in the style of include/casapose_hip.h -> (symbols, pointees, return_pointees, twins):
    symbols [(name, restype, argtypes)] in declaration order; pointees {name: per argument, what a pointer points to ("float", "void",
    "uint8_t*", ...) or None for a scalar}; return_pointees {name: the same for the return value}; twins {X_T: X_host_T} for T in f32 / f64 /
    u8 / u16 / i32 where both are declared -- X_host_T then must take X_T's parameters minus a trailing `void* stream`.  A statement that is no struct, enum
    or readable prototype raises CasaposeHipError: nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    text = re.sub(r"\b(typedef\s+)?(struct|enum)\b[^{};]*\{[^{}]*\}[^;]*;", " ", text)
    symbols, pointees, return_pointees = [], {}, {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(?P<ret>[\w\s*]+?)\b(?P<name>\w+) ?\((?P<params>[^()]*)\)", stmt)
        if m is None:
            raise CasaposeHipError("cannot read the declaration `%s`" % stmt)
        name, params = m.group("name"), m.group("params").strip()
        if name in pointees:
            raise CasaposeHipError("%s is declared twice" % name)
        restype, return_pointees[name] = _parse_type(m.group("ret"), name + ", return type", is_return=True)
        parsed = [] if params in ("", "void") else [_parse_type(p, "%s, parameter %d" % (name, i)) for i, p in enumerate(params.split(","))]
        symbols.append((name, restype, [t for t, _ in parsed]))
        pointees[name] = tuple(p for _, p in parsed)
    twins, argtypes = {}, {n: a for n, _, a in symbols}
    for host in pointees:
        m = re.fullmatch(r"(\w+)_host_(f32|f64|u8|u16|i32)", host)
        device = m and "%s_%s" % m.groups()
        if device in pointees:
            if argtypes[device] != argtypes[host] + [C.c_void_p] or pointees[device] != pointees[host] + ("void",):
                raise CasaposeHipError("%s must take the parameters of %s minus the trailing `void* stream`" % (host, device))
            twins[device] = host
    return symbols, pointees, return_pointees, twins


with open(HEADER_PATH) as _f:
    _header = _f.read()
_m = re.search(r"^#define CP_ABI_VERSION (\d+)", _header, flags=re.M)
if _m is None:
    raise CasaposeHipError("%s does not define CP_ABI_VERSION" % HEADER_PATH)
ABI_VERSION = int(_m.group(1))
# every symbol the header declares: (name, restype, argtypes); what each pointer points to; the kernels that have a host twin
SYMBOLS, POINTEES, RETURN_POINTEES, _PAIRS = parse_header(_header)
# cp_pnp_weighted_f64 takes cp_pnp_f64's arguments plus the weights: the pair is listed as that kernel's variant, and TWINS keeps one row per
# kernel.  host_twin() reads both.
TWIN_VARIANTS = {d: _PAIRS[d] for d in ("cp_pnp_weighted_f64",)}
# cp_depth_icp_step_f64 has no inputs of its own: it reads the planes and rewrites the poses of cp_render_masks_u8, whose row TWINS holds.  Its
# pair is listed as a step on that kernel's output.  cp_contour_step_f64 is the same kind of step, and cp_mask_edt_u16 is one on the label map
# cp_ccl_filter_labels leaves behind.
TWIN_STEPS = {d: _PAIRS[d] for d in ("cp_depth_icp_step_f64", "cp_contour_step_f64", "cp_mask_edt_u16")}
# cp_pose_verify_i32 reads another kernel's output (the renderer's planes and records) and rewrites nothing: a reader.
TWIN_READERS = {d: _PAIRS[d] for d in ("cp_pose_verify_i32",)}
# cp_render_shaded_f32 is cp_render_masks_u8's geometry with a colour output: the pair is listed as that kernel's output variant, beside the
# argument variants above, and TWINS keeps one row per kernel.
TWIN_OUTPUT_VARIANTS = {d: _PAIRS[d] for d in ("cp_render_shaded_f32",)}
TWINS = {d: h for d, h in _PAIRS.items()
         if d not in TWIN_VARIANTS and d not in TWIN_OUTPUT_VARIANTS and d not in TWIN_STEPS and d not in TWIN_READERS}


def host_twin(name: str) -> Optional[str]:
    """the host twin of the device entry point `name` (a kernel's, a variant's, a follow-up step's or a reader's), or None"""
    return TWINS.get(name) or TWIN_VARIANTS.get(name) or TWIN_OUTPUT_VARIANTS.get(name) or TWIN_STEPS.get(name) or TWIN_READERS.get(name)


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once) and bind every declared symbol.  Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CasaposeHipError(
            "libcasapose_hip.so not found at %s -- build it with `python __graft_entry__.py` "
            "(there is no CPU fallback for the product path)" % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    # ABI check: the descriptor grew between rounds; a library built from another revision of the header must not be handed this struct
    if lib.cp_version() != ABI_VERSION or lib.cp_conv_desc_size() != C.sizeof(ConvDesc) or lib.cp_conv_source_size() != C.sizeof(ConvSource):
        raise CasaposeHipError("%s has ABI %d with sizeof(cp_conv_desc) = %d, sizeof(cp_conv_source) = %d; this binding is ABI %d with %d / %d -- "
                               "rebuild the library (python __graft_entry__.py)" % (LIB_PATH, lib.cp_version(), lib.cp_conv_desc_size(),
                                                                                  lib.cp_conv_source_size(), ABI_VERSION, C.sizeof(ConvDesc), C.sizeof(ConvSource)))
    if lib.cp_aug_image_size() != C.sizeof(AugImage):
        raise CasaposeHipError("%s has sizeof(cp_aug_image) = %d; this binding declares %d -- rebuild the library (python __graft_entry__.py)"
                               % (LIB_PATH, lib.cp_aug_image_size(), C.sizeof(AugImage)))
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().cp_last_error()
        raise CasaposeHipError("%s failed (%d): %s" % (what or "casapose_hip call", status, (msg or b"").decode()))
