"""The three Winograd transform entry points (cp_wino_input_transform_pre_f32, cp_wino_output_transform_stats_f32,
cp_wino_output_input_transform_f32) called directly, against fp64 restatements of B^T d B and A^T M A + epilogue.

The kernels reach pixels outside the image -- the zero padding of the input transform, the ragged last tiles of the output transform, the
threads of a fused block that own no tile -- through predicated (range-checked) accesses.  So every tensor here is a slice of a larger
buffer filled with NaN: strides wider than the channel count, NaN in the padding tiles of M and V, NaN guards in front of and behind each
tensor.  A predicated load that leaks shows up as a NaN in a result, a predicated store that leaks as an overwritten guard.

Bound: the forward error of the sums, element by element -- |error| <= 16 * 2^-24 * (|A^T| |M| |A| + |residual|), times |scale| for the
activated output, and 16 * 2^-24 * |B^T| |d| |B| for V (at most ten roundings stand between an operand and a result, and the factor leaves
room for the activation's).  For the fused transform's V' the error of the activated map it is computed from is carried through |B^T| . |B|.
The fp64 references are computed once per geometry and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 16.0 * 2.0 ** -24
GUARD = 64   # floats of NaN in front of and behind every tensor (256 bytes: the 16-byte alignment of the float4 accesses is kept)
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
NONE, RELU, LEAKY = 0, 1, 2

# (batch, h, w, dilation, channels, ld of the pixel tensors, channel offset in V, ld of V)
GEOMS = {
    "subgrid_smaller_than_a_tile": (2, 9, 7, 4, 4, 8, 0, 4),
    "ragged_last_row_and_column": (2, 13, 18, 1, 8, 12, 0, 8),
    "strided_channel_slice": (1, 15, 20, 2, 36, 40, 4, 48),
}


def _lib():
    from casapose_amd import _lib as L

    return L, L.load()


@functools.lru_cache(maxsize=None)
def _tiles(b, h, w, d):
    """(T, Tp, [(t, n, sy, sx, tu, tv)]) -- the tile numbering of wino.hip"""
    L, lib = _lib()
    t, tp = C.c_int(0), C.c_int(0)
    L.check(lib.cp_wino_tiles(b, h, w, d, C.byref(t), C.byref(tp)))
    tu_n, tv_n = ((h + d - 1) // d + 3) // 4, ((w + d - 1) // d + 3) // 4
    assert t.value == b * d * d * tu_n * tv_n and tp.value >= t.value
    out = []
    for n in range(b):
        for sy in range(d):
            for sx in range(d):
                for tu in range(tu_n):
                    for tv in range(tv_n):
                        out.append(((((n * d + sy) * d + sx) * tu_n + tu) * tv_n + tv, n, sy, sx, tu, tv))
    return t.value, tp.value, out


def _act64(x, act):
    if act == RELU:
        return np.maximum(x, 0.0)
    if act == LEAKY:
        return np.maximum(x, 0.0) - np.maximum(np.float64(np.float32(-0.1)) * x, 0.0)
    return x


def _ref_input(x, b, h, w, d):
    """x [b, h, w, c] fp64 -> V [36, T, c] = B^T d B of every tile's zero-padded patch, and |B^T| |d| |B|"""
    T, _, tiles = _tiles(b, h, w, d)
    c = x.shape[-1]
    V, Vabs = np.zeros((36, T, c)), np.zeros((36, T, c))
    for t, n, sy, sx, tu, tv in tiles:
        patch = np.zeros((6, 6, c))
        for r in range(6):
            y = sy + d * (4 * tu + r - 1)
            for j in range(6):
                xx = sx + d * (4 * tv + j - 1)
                if 0 <= y < h and 0 <= xx < w:
                    patch[r, j] = x[n, y, xx]
        V[:, t] = np.einsum("ar,rjc,bj->abc", BT, patch, BT).reshape(36, c)
        Vabs[:, t] = np.einsum("ar,rjc,bj->abc", np.abs(BT), np.abs(patch), np.abs(BT)).reshape(36, c)
    return V, Vabs


def _ref_output(M, b, h, w, d):
    """M [36, T, c] fp64 -> Y [b, h, w, c] = A^T M A of every tile, cropped to the image, and |A^T| |M| |A|"""
    _, _, tiles = _tiles(b, h, w, d)
    c = M.shape[-1]
    Y, Yabs = np.zeros((b, h, w, c)), np.zeros((b, h, w, c))
    for t, n, sy, sx, tu, tv in tiles:
        m = M[:, t].reshape(6, 6, c)
        y4 = np.einsum("ar,rjc,bj->abc", AT, m, AT)
        a4 = np.einsum("ar,rjc,bj->abc", np.abs(AT), np.abs(m), np.abs(AT))
        for r in range(4):
            y = sy + d * (4 * tu + r)
            for j in range(4):
                xx = sx + d * (4 * tv + j)
                if y < h and xx < w:
                    Y[n, y, xx], Yabs[n, y, xx] = y4[r, j], a4[r, j]
    return Y, Yabs


class Guarded:
    """A device tensor of `shape` whose last dimension is the first `c` (from `c_off`) of `ld` elements, inside a NaN-filled buffer with guards."""

    def __init__(self, device, shape, ld, c_off=0, values=None, lead_valid=None):
        self.shape, self.ld, self.c_off = tuple(shape), ld, c_off
        rows = int(np.prod(shape[:-1]))
        self.buf = torch.full((2 * GUARD + rows * ld,), float("nan"), device=device)
        self.wide = self.buf[GUARD:GUARD + rows * ld].view(*shape[:-1], ld)
        self.view = self.wide[..., c_off:c_off + shape[-1]]
        self.written = torch.zeros_like(self.buf, dtype=torch.bool)   # where a kernel may write (or the test has put values)
        wv = self.written[GUARD:GUARD + rows * ld].view(*shape[:-1], ld)[..., c_off:c_off + shape[-1]]
        if lead_valid is None:
            wv[:] = True
        else:   # [36, Tp, c]: only the first T tiles of every plane
            wv[:, :lead_valid] = True
        if values is not None:
            self.view.copy_(values)

    @property
    def ptr(self):
        return self.wide.data_ptr()

    def check_untouched(self, what):
        outside = self.buf[~self.written]
        assert bool(torch.isnan(outside).all()), "%s: %d elements outside the tensor were written" % (what, int((~torch.isnan(outside)).sum()))


@functools.lru_cache(maxsize=None)
def _input_case(name):
    b, h, w, d, c, ld, c_off, ldv = GEOMS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((b, h, w, c)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    shift = (100.0 + rng.standard_normal(c)).astype(np.float32)   # a padding pixel passed through the affine would read ~100, not 0
    return x, scale, shift


@functools.lru_cache(maxsize=None)
def _input_ref(name, pre):
    b, h, w, d = GEOMS[name][:4]
    x, scale, shift = _input_case(name)
    x64 = x.astype(np.float64)
    if pre == "factor":
        x64 = x64 * scale
    elif pre is not None:
        x64 = _act64(x64 * scale + shift, pre)
    return _ref_input(x64, b, h, w, d)


PRE_FORMS = [None, "factor", NONE, RELU, LEAKY]


@pytest.mark.parametrize("name,pre", [(n, None) for n in GEOMS] + [("strided_channel_slice", p) for p in PRE_FORMS[1:]] + [("subgrid_smaller_than_a_tile", LEAKY)])
def test_input_transform_against_fp64(device, name, pre):
    """V = B^T d B of the zero-padded (and, for the PRE forms, normalised + activated) input; padding stays exactly zero -- the shift of ~100
    would show otherwise --, V outside [c_off, c_off + C) and the padding tiles T..Tp stay untouched."""
    L, lib = _lib()
    b, h, w, d, c, ld, c_off, ldv = GEOMS[name]
    T, Tp, _ = _tiles(b, h, w, d)
    x, scale, shift = _input_case(name)
    src = Guarded(device, (b, h, w, c), ld, values=torch.from_numpy(x))
    V = Guarded(device, (36, Tp, c), ldv, c_off, lead_valid=T)
    sc, sh = Guarded(device, (c,), c, values=torch.from_numpy(scale)), Guarded(device, (c,), c, values=torch.from_numpy(shift))
    st = torch.cuda.current_stream().cuda_stream
    args = {None: (None, None, 0), "factor": (sc.ptr, None, 0)}.get(pre, (sc.ptr, sh.ptr, pre))
    L.check(lib.cp_wino_input_transform_pre_f32(src.ptr, ld, c, b, h, w, d, V.ptr, ldv, c_off, args[0], args[1], args[2], st))
    torch.cuda.synchronize()
    ref, bound = _input_ref(name, pre)
    got = V.view[:, :T].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "%d non-finite elements of V" % int((~np.isfinite(got)).sum())
    excess = np.abs(got - ref) - EPS * bound
    print("input transform %s pre %s: max |err| %.3g, max err / bound %.3g" % (name, pre, np.abs(got - ref).max(), (np.abs(got - ref) / np.maximum(EPS * bound, 1e-300)).max()))
    assert (excess <= 0).all(), "V off by up to %.3g beyond the bound" % excess.max()
    V.check_untouched("V")


@functools.lru_cache(maxsize=None)
def _output_case(name, cout=None):
    b, h, w, d, c = GEOMS[name][:5]
    c = cout or c
    T, Tp, _ = _tiles(b, h, w, d)
    rng = np.random.default_rng(sum(map(ord, name)) + 7 * c)
    M = rng.standard_normal((36, T, c)).astype(np.float32)
    res = rng.standard_normal((b, h, w, c)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    shift = rng.standard_normal(c).astype(np.float32)
    labels = rng.integers(0, 5, (b, h, w)).astype(np.uint8)
    tab_scale = (rng.uniform(0.5, 1.5, (5, c)) * rng.choice([-1.0, 1.0], (5, c))).astype(np.float32)
    tab_shift = rng.standard_normal((5, c)).astype(np.float32)
    Y, Yabs = _ref_output(M.astype(np.float64), b, h, w, d)
    return M, res, scale, shift, labels, tab_scale, tab_shift, Y, Yabs


def _check_outputs(what, raw, act, Y, Yabs, res, scale, shift, act_kind):
    """raw / act: Guarded outputs or None; scale / shift broadcast against [b, h, w, c].  Returns (fp64 activated map, its error bound)."""
    raw_ref = Y + (res.astype(np.float64) if res is not None else 0.0)
    raw_bound = EPS * (Yabs + (np.abs(res) if res is not None else 0.0))
    act_ref = _act64(raw_ref * scale + shift, act_kind)
    act_bound = raw_bound * np.abs(scale)
    for name, g, ref, bound in (("raw", raw, raw_ref, raw_bound), ("act", act, act_ref, act_bound)):
        if g is None:
            continue
        got = g.view.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), "%s %s: %d non-finite elements" % (what, name, int((~np.isfinite(got)).sum()))
        err = np.abs(got - ref)
        print("%s %s: max |err| %.3g, max err / bound %.3g" % (what, name, err.max(), (err / bound).max()))
        assert (err <= bound).all(), "%s %s off by up to %.3g beyond the bound" % (what, name, (err - bound).max())
        g.check_untouched(what + " " + name)
    return act_ref, act_bound


@pytest.mark.parametrize("outputs", ["raw", "act", "both"])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("name", list(GEOMS))
def test_output_transform_against_fp64(device, name, with_residual, outputs):
    """Y = A^T M A (+ residual), act(Y * scale + shift): every combination of the optional tensors, strides wider than cout, NaN in M's padding tiles"""
    L, lib = _lib()
    b, h, w, d, c, ld = GEOMS[name][:6]
    T, Tp, _ = _tiles(b, h, w, d)
    M, res, scale, shift, _, _, _, Y, Yabs = _output_case(name)
    Mg = Guarded(device, (36, Tp, c), c, lead_valid=T)
    Mg.view[:, :T] = torch.from_numpy(M).to(device)
    resg = Guarded(device, (b, h, w, c), ld + 4, values=torch.from_numpy(res)) if with_residual else None
    raw = Guarded(device, (b, h, w, c), ld) if outputs in ("raw", "both") else None
    act = Guarded(device, (b, h, w, c), ld + 8) if outputs in ("act", "both") else None
    sc, sh = Guarded(device, (c,), c, values=torch.from_numpy(scale)), Guarded(device, (c,), c, values=torch.from_numpy(shift))
    act_kind = RELU if name != "ragged_last_row_and_column" else LEAKY
    L.check(lib.cp_wino_output_transform_stats_f32(Mg.ptr, c, b, h, w, d, resg.ptr if resg else None, ld + 4, sc.ptr, sh.ptr, None, act_kind,
                                                   raw.ptr if raw else None, ld, act.ptr if act else None, ld + 8, None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    _check_outputs("output transform " + name, raw, act, Y, Yabs, res if with_residual else None, scale, shift, act_kind)


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("name", list(GEOMS))
def test_output_transform_label_table_and_statistics(device, name, with_residual):
    """The label-indexed affine table (scale / shift rows chosen per pixel) together with the fp64 sum and sum of squares of the raw output over
    the real pixels: the sums inherit the raw output's bound (the accumulation itself is fp64), summed over the pixels."""
    L, lib = _lib()
    b, h, w, d, c, ld = GEOMS[name][:6]
    T, Tp, _ = _tiles(b, h, w, d)
    M, res, _, _, labels, tab_scale, tab_shift, Y, Yabs = _output_case(name)
    Mg = Guarded(device, (36, Tp, c), c, lead_valid=T)
    Mg.view[:, :T] = torch.from_numpy(M).to(device)
    resg = Guarded(device, (b, h, w, c), ld + 4, values=torch.from_numpy(res)) if with_residual else None
    raw, act = Guarded(device, (b, h, w, c), ld), Guarded(device, (b, h, w, c), ld + 8)
    ts, tb = Guarded(device, (5, c), c, values=torch.from_numpy(tab_scale)), Guarded(device, (5, c), c, values=torch.from_numpy(tab_shift))
    lab = torch.from_numpy(labels).to(device)
    stats = torch.full((2 * c,), float("nan"), dtype=torch.float64, device=device)
    L.check(lib.cp_wino_output_transform_stats_f32(Mg.ptr, c, b, h, w, d, resg.ptr if resg else None, ld + 4, ts.ptr, tb.ptr, lab.data_ptr(), LEAKY, raw.ptr, ld,
                                                   act.ptr, ld + 8, stats.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    r = res if with_residual else None
    _check_outputs("label table " + name, raw, act, Y, Yabs, r, tab_scale[labels], tab_shift[labels], LEAKY)
    raw_ref = Y + (r.astype(np.float64) if r is not None else 0.0)
    raw_bound = EPS * (Yabs + (np.abs(r) if r is not None else 0.0))
    got = stats.cpu().numpy()
    s_ref, q_ref = raw_ref.sum((0, 1, 2)), (raw_ref ** 2).sum((0, 1, 2))
    s_bound, q_bound = raw_bound.sum((0, 1, 2)), ((2 * np.abs(raw_ref) + raw_bound) * raw_bound).sum((0, 1, 2))
    print("statistics %s: sum err / bound %.3g, sum of squares err / bound %.3g" % (name, (np.abs(got[:c] - s_ref) / s_bound).max(), (np.abs(got[c:] - q_ref) / q_bound).max()))
    assert np.isfinite(got).all() and (np.abs(got[:c] - s_ref) <= s_bound).all() and (np.abs(got[c:] - q_ref) <= q_bound).all()


FUSED = {"one_tile_subgrids": (2, 9, 7, 4), "two_tile_subgrids": (2, 15, 20, 4)}


@functools.lru_cache(maxsize=None)
def _fused_case(name):
    b, h, w, d = FUSED[name]
    c = 36   # nine channel quads: the second slice of eight is partial
    T, Tp, _ = _tiles(b, h, w, d)
    rng = np.random.default_rng(sum(map(ord, name)))
    M = rng.standard_normal((36, T, c)).astype(np.float32)
    res = rng.standard_normal((b, h, w, c)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    shift = rng.standard_normal(c).astype(np.float32)
    Y, Yabs = _ref_output(M.astype(np.float64), b, h, w, d)
    return M, res, scale, shift, Y, Yabs


@pytest.mark.parametrize("outputs", ["raw", "act", "both", "neither"])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("name", list(FUSED))
def test_fused_output_input_transform_against_fp64(device, name, with_residual, outputs):
    """cout 36 (a partial last slice of eight quads), a residual with res_ld > cout, either optional output absent; V' = B^T act B with the
    zero ring of the next convolution's padding, into a channel slice of a wider V whose padding tiles stay untouched."""
    L, lib = _lib()
    b, h, w, d = FUSED[name]
    c, ld, c_off, ldv = 36, 40, 8, 48
    assert lib.cp_wino_output_input_applicable(b, h, w, d, c) == 1
    T, Tp, _ = _tiles(b, h, w, d)
    M, res, scale, shift, Y, Yabs = _fused_case(name)
    Mg = Guarded(device, (36, Tp, c), c, lead_valid=T)
    Mg.view[:, :T] = torch.from_numpy(M).to(device)
    resg = Guarded(device, (b, h, w, c), ld + 4, values=torch.from_numpy(res)) if with_residual else None
    raw = Guarded(device, (b, h, w, c), ld) if outputs in ("raw", "both") else None
    act = Guarded(device, (b, h, w, c), ld + 8) if outputs in ("act", "both") else None
    V = Guarded(device, (36, Tp, c), ldv, c_off, lead_valid=T)
    sc, sh = Guarded(device, (c,), c, values=torch.from_numpy(scale)), Guarded(device, (c,), c, values=torch.from_numpy(shift))
    L.check(lib.cp_wino_output_input_transform_f32(Mg.ptr, c, b, h, w, d, resg.ptr if resg else None, ld + 4, sc.ptr, sh.ptr, RELU, raw.ptr if raw else None, ld,
                                                   act.ptr if act else None, ld + 8, V.ptr, ldv, c_off, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    act_ref, act_bound = _check_outputs("fused transform " + name, raw, act, Y, Yabs, res if with_residual else None, scale, shift, RELU)
    v_ref, v_abs = _ref_input(act_ref, b, h, w, d)
    _, carried = _ref_input(act_bound, b, h, w, d)   # |B^T| (bound of the activated map) |B|
    got = V.view[:, :T].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "%d non-finite elements of V'" % int((~np.isfinite(got)).sum())
    err, bound = np.abs(got - v_ref), EPS * v_abs + carried
    print("fused transform %s V': max |err| %.3g, max err / bound %.3g" % (name, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), "V' off by up to %.3g beyond the bound" % (err - bound).max()
    V.check_untouched("V'")
