"""The streaming kernels between the convolutions (csrc/aux_kernels.hip, csrc/guided_bilinear.hip, the resampling and utility part of
csrc/train_kernels.hip) checked one by one: the C ABI is called directly and every output is compared with the float64 restatement of
tests/resample_reference.py, which tests/test_resample_reference.py checks first on the CPU.  The inputs and the properties each is chosen
for are in tests/resample_cases.py; those properties are asserted there, on the reference, before a kernel's result is looked at.

Every call: the output buffer is pre-filled with a byte pattern (nothing may depend on what it held, and every element must be written), a
guard band behind it must come back untouched, and the read-only inputs are compared with their originals afterwards.

Copies, selections, arg-max and the integer-valued adjoints are compared bit for bit.  The blends are rounding-bounded, per output element:
|got - ref| <= (n + 4) 2^-24 S, with n the number of products in the reference's sum for that element (at most 4 forward, 16 in an adjoint)
and S the sum of their absolute values.  A sum of n float32 products accumulated in any order is off by at most n roundings of at most S
each; the + 4 covers the roundings inside one coefficient (miss / n, w + share, the product) and of the nested form of the plain bilinear
blend.  FMA contraction removes roundings, it adds none.  An element whose reference sum has no term must be exactly 0."""
import functools

import numpy as np
import pytest
import torch

import resample_cases as Cs
import resample_reference as R

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0xA5)
GUARD, GUARD_BYTE = 512, 0x3C
U = 2.0 ** -24
fills = pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill%02X" % f)


class Call:
    """the buffers of one call: inputs that must come back unchanged, outputs with a guard band behind them"""

    def __init__(self, lib, device):
        self.lib, self.device, self.inputs, self.outputs = lib, device, [], []

    def inp(self, array):
        a = np.ascontiguousarray(array)
        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.device)
        assert t.data_ptr() % 16 == 0
        self.inputs.append((t, a))
        return t.data_ptr()

    def out(self, shape, dtype, fill, initial=None):
        """a buffer of `shape` filled with the byte `fill`, or holding `initial`; returns its address"""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = torch.full((nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        if initial is None:
            raw[:nbytes] = fill
        else:
            raw[:nbytes] = torch.from_numpy(np.ascontiguousarray(initial, dtype=dtype).view(np.uint8).reshape(-1).copy()).to(self.device)
        assert raw.data_ptr() % 16 == 0
        self.outputs.append((raw, nbytes, shape, dtype))
        return raw.data_ptr()

    def run(self, name, *args):
        from casapose_amd import _lib

        _lib.check(getattr(self.lib, name)(*args, torch.cuda.current_stream(self.device).cuda_stream), name)
        torch.cuda.synchronize(self.device)

    def result(self, k=0):
        """output k, after the checks that hold for every call"""
        for t, a in self.inputs:
            assert t.cpu().numpy().tobytes() == a.tobytes(), "a read-only input was written"
        raw, nbytes, shape, dtype = self.outputs[k]
        host = raw.cpu().numpy()
        assert (host[nbytes:] == GUARD_BYTE).all(), "the guard band behind the output was written"
        return host[:nbytes].view(dtype).reshape(shape).copy()


def same_bits(got, want):
    want = np.ascontiguousarray(want, dtype=got.dtype)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def assert_same_bits(got, want, what):
    if not same_bits(got, want):
        want = np.ascontiguousarray(want, dtype=got.dtype)
        bad = np.argwhere(got.view(np.uint8 if got.itemsize == 1 else np.uint32) != want.view(np.uint8 if got.itemsize == 1 else np.uint32))
        raise AssertionError("%s: %d elements differ, first at %s: got %r, reference %r"
                             % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def assert_bounded(got, ref, what):
    assert got.dtype == np.float32 and got.shape == ref.out.shape
    err = np.abs(got.astype(np.float64) - ref.out)
    bound = (ref.n + 4) * U * ref.S
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d elements past the bound, first at %s: got %r, reference %r, error %.3g, bound %.3g (n = %d, S = %.6g)"
                             % (what, int(bad.sum()), list(i), got[i], ref.out[i], err[i], bound[i], ref.n[i], ref.S[i]))
    empty = ref.n == 0
    assert (got[empty] == 0).all(), "%s: an element without a term is not exactly 0" % what


def wide(dy, c):
    """dy as channels [8, 8 + c) of a buffer c + 20 floats wide, NaN everywhere else; the buffer and the byte offset of channel 8"""
    buf = np.full(dy.shape[:-1] + (c + 20,), np.nan, np.float32)
    buf[..., 8:8 + c] = dy
    return buf, 32


# ---- the references, computed once and shared by the fills ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_guided_bilinear(name):
    case = Cs.guided(name)
    return R.guided_bilinear(case.x, case.mask)


@functools.lru_cache(maxsize=None)
def ref_guided_bilinear_bwd(name):
    case = Cs.guided(name)
    return R.guided_bilinear_bwd(case.dy, case.mask)


@functools.lru_cache(maxsize=None)
def ref_bilinear(name):
    return R.bilinear_x2(Cs.guided(name).x)


@functools.lru_cache(maxsize=None)
def ref_bilinear_bwd(name):
    return R.bilinear_x2_bwd(Cs.guided(name).dy)


@functools.lru_cache(maxsize=None)
def ref_nearest_bwd(name):
    case = Cs.guided(name)
    return R.guided_nearest_bwd(case.dy_int, case.sel)


@functools.lru_cache(maxsize=None)
def ref_pool(shape, kind):
    return R.maxpool(Cs.pool(shape, kind).x)


FWD_NAMES = Cs.GUIDED_NAMES + ("big_fwd",)
BWD_NAMES = Cs.GUIDED_NAMES + ("big_bwd",)
POOL_CASES = [(s, k) for s in Cs.POOL_SHAPES for k in Cs.POOL_KINDS] + [(Cs.POOL_BIG, "relu")]


def check_items(name, formula, big):
    shape = dict(Cs.GUIDED_SHAPES)[name]
    assert Cs.past_cap(formula(*shape)) == (name == big), (name, formula(*shape))
    return shape


# ---- guided bilinear: mask, forward, adjoint ----------------------------------------------------------------------------------------------------------
@fills
@pytest.mark.parametrize("name", Cs.GUIDED_NAMES + ("big",))
def test_match_mask(hip_lib, device, name, fill):
    if name == "big":
        pair = Cs.mask_big()
        assert Cs.past_cap(Cs.items_match_mask(*Cs.MASK_BIG))
    else:
        pair = Cs.guided(name)
    want = R.match_mask(pair.hi, pair.lo)
    b, hh, ww = pair.hi.shape
    call = Call(hip_lib, device)
    out = call.out(want.shape, np.uint8, fill)
    call.run("cp_guided_match_mask", call.inp(pair.hi), call.inp(pair.lo), b, hh, ww, out)
    assert_same_bits(call.result(), want, "cp_guided_match_mask")


@fills
@pytest.mark.parametrize("name", FWD_NAMES)
def test_guided_bilinear_forward(hip_lib, device, name, fill):
    b, h, w, c = check_items(name, Cs.items_up_fwd, "big_fwd")
    case, ref = Cs.guided(name), ref_guided_bilinear(name)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_guided_bilinear_upsample_x2_f32", call.inp(case.x), call.inp(case.mask), b, h, w, c, out)
    got = call.result()
    assert_bounded(got, ref, "cp_guided_bilinear_upsample_x2_f32")
    assert not got[case.mask == 0].any()                       # no tap matches: exactly 0


@fills
@pytest.mark.parametrize("name", BWD_NAMES)
def test_guided_bilinear_backward(hip_lib, device, name, fill):
    b, h, w, c = check_items(name, Cs.items_up_bwd, "big_bwd")
    case, ref = Cs.guided(name), ref_guided_bilinear_bwd(name)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_guided_bilinear_upsample_x2_bwd_f32", call.inp(case.dy), c, call.inp(case.mask), b, h, w, c, out)
    dense = call.result()
    assert_bounded(dense, ref, "cp_guided_bilinear_upsample_x2_bwd_f32")
    buf, off = wide(case.dy, c)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_guided_bilinear_upsample_x2_bwd_f32", call.inp(buf) + off, c + 20, call.inp(case.mask), b, h, w, c, out)
    assert_same_bits(call.result(), dense, "cp_guided_bilinear_upsample_x2_bwd_f32 with ld_dy = channels + 20")


# ---- plain bilinear x2 -----------------------------------------------------------------------------------------------------------------------------
@fills
@pytest.mark.parametrize("name", FWD_NAMES)
def test_bilinear_forward(hip_lib, device, name, fill):
    b, h, w, c = check_items(name, Cs.items_up_fwd, "big_fwd")
    case, ref = Cs.guided(name), ref_bilinear(name)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_upsample_bilinear_x2_f32", call.inp(case.x), b, h, w, c, out)
    assert_bounded(call.result(), ref, "cp_upsample_bilinear_x2_f32")


@fills
@pytest.mark.parametrize("name", BWD_NAMES)
def test_bilinear_backward(hip_lib, device, name, fill):
    b, h, w, c = check_items(name, Cs.items_up_bwd, "big_bwd")
    case, ref = Cs.guided(name), ref_bilinear_bwd(name)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_upsample_bilinear_x2_bwd_f32", call.inp(case.dy), c, b, h, w, c, out)
    dense = call.result()
    assert_bounded(dense, ref, "cp_upsample_bilinear_x2_bwd_f32")
    buf, off = wide(case.dy, c)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_upsample_bilinear_x2_bwd_f32", call.inp(buf) + off, c + 20, b, h, w, c, out)
    assert_same_bits(call.result(), dense, "cp_upsample_bilinear_x2_bwd_f32 with ld_dy = channels + 20")


# ---- guided nearest x2 -----------------------------------------------------------------------------------------------------------------------------------
@fills
@pytest.mark.parametrize("name", FWD_NAMES)
def test_guided_nearest_forward(hip_lib, device, name, fill):
    b, h, w, c = check_items(name, Cs.items_up_fwd, "big_fwd")
    case = Cs.guided(name)
    want = R.guided_nearest(case.x, case.sel)
    call = Call(hip_lib, device)
    out = call.out(want.shape, np.float32, fill)
    call.run("cp_guided_upsample_x2_f32", call.inp(case.x), call.inp(case.sel), b, h, w, c, out)
    assert_same_bits(call.result(), want, "cp_guided_upsample_x2_f32")


@fills
@pytest.mark.parametrize("name", BWD_NAMES)
def test_guided_nearest_backward(hip_lib, device, name, fill):
    b, h, w, c = check_items(name, Cs.items_up_bwd, "big_bwd")
    case, want = Cs.guided(name), ref_nearest_bwd(name)
    assert np.abs(want).max() <= 64                            # sums of at most 16 integers of at most 4: exact in float32 in any order
    call = Call(hip_lib, device)
    out = call.out(want.shape, np.float32, fill)
    call.run("cp_guided_upsample_x2_bwd_f32", call.inp(case.dy_int), c, call.inp(case.sel), b, h, w, c, out)
    dense = call.result()
    assert_same_bits(dense, want + 0.0, "cp_guided_upsample_x2_bwd_f32")
    buf, off = wide(case.dy_int, c)
    call = Call(hip_lib, device)
    out = call.out(want.shape, np.float32, fill)
    call.run("cp_guided_upsample_x2_bwd_f32", call.inp(buf) + off, c + 20, call.inp(case.sel), b, h, w, c, out)
    assert_same_bits(call.result(), dense, "cp_guided_upsample_x2_bwd_f32 with ld_dy = channels + 20")


# ---- max-pool ------------------------------------------------------------------------------------------------------------------------------------------------
def pool_ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@fills
@pytest.mark.parametrize("shape,kind", POOL_CASES, ids=pool_ids)
def test_maxpool_forward(hip_lib, device, shape, kind, fill):
    b, h, w, c = shape
    assert Cs.past_cap(Cs.items_pool_fwd(*shape)) == (shape == Cs.POOL_BIG)
    case, ref = Cs.pool(shape, kind), ref_pool(shape, kind)
    call = Call(hip_lib, device)
    out = call.out(ref.val.shape, np.float32, fill)
    call.run("cp_maxpool3x3s2_f32", call.inp(case.x), b, h, w, c, None, None, 0, out)
    plain = call.result()
    assert_same_bits(plain, ref.val, "cp_maxpool3x3s2_f32")
    call = Call(hip_lib, device)
    out, idx = call.out(ref.val.shape, np.float32, fill), call.out(ref.idx.shape, np.uint8, fill)
    call.run("cp_maxpool3x3s2_idx_f32", call.inp(case.x), b, h, w, c, out, idx)
    assert_same_bits(call.result(0), ref.val, "cp_maxpool3x3s2_idx_f32, values")
    assert_same_bits(call.result(1), ref.idx, "cp_maxpool3x3s2_idx_f32, first-maximum taps")
    assert_same_bits(call.result(0), plain, "cp_maxpool3x3s2_idx_f32 against cp_maxpool3x3s2_f32")


@fills
@pytest.mark.parametrize("relu", (0, 1), ids=("affine", "affine_relu"))
@pytest.mark.parametrize("shape,kind", POOL_CASES, ids=pool_ids)
def test_maxpool_scale_shift(hip_lib, device, shape, kind, relu, fill):
    """|got - ref| <= 3 * 2^-24 * (|m s| + |b|): the product, the sum, and one more for a product that is not fused; a window of -inf alone gives
    -inf * s + b = -+inf on both sides (no scale is 0), compared as equal"""
    b, h, w, c = shape
    case = Cs.pool(shape, kind)
    rng = np.random.default_rng(c)
    scale = (rng.uniform(0.5, 1.5, c) * rng.choice((-1.0, 1.0), c)).astype(np.float32)
    shift = rng.standard_normal(c).astype(np.float32)
    ref = R.scale_shift(ref_pool(shape, kind).val, scale.astype(np.float64), shift.astype(np.float64), relu)
    call = Call(hip_lib, device)
    out = call.out(ref.out.shape, np.float32, fill)
    call.run("cp_maxpool3x3s2_f32", call.inp(case.x), b, h, w, c, call.inp(scale), call.inp(shift), relu, out)
    got = call.result().astype(np.float64)
    finite = np.isfinite(ref.mag)
    assert kind == "neg_inf" or finite.all()
    assert np.array_equal(got[~finite], ref.out[~finite])
    err = np.abs(got[finite] - ref.out[finite])
    assert (err <= 3 * U * ref.mag[finite]).all(), float((err / np.maximum(ref.mag[finite], 1e-300)).max() / U)
    if relu:
        assert (got >= 0).all()


@fills
@pytest.mark.parametrize("accumulate", (0, 1), ids=("overwrite", "accumulate"))
@pytest.mark.parametrize("shape,kind", POOL_CASES, ids=pool_ids)
def test_maxpool_backward(hip_lib, device, shape, kind, accumulate, fill):
    """both adjoints against the scatter of dy to the reference's first maximum: ties between in-image taps, ties with the padding, and windows
    the padding wins (whose gradient is dropped) included.  dy and the previous dx are small integers: every sum is exact."""
    b, h, w, c = shape
    assert Cs.past_cap(Cs.items_pool_bwd(*shape)) == (shape == Cs.POOL_BIG)
    case, ref = Cs.pool(shape, kind), ref_pool(shape, kind)
    want = R.maxpool_bwd(case.x, case.dy, case.dx_prev if accumulate else None, pooled=ref)
    assert np.abs(want).max() <= 64
    prev = case.dx_prev if accumulate else None
    call = Call(hip_lib, device)
    out = call.out(want.shape, np.float32, fill, prev)
    call.run("cp_maxpool3x3s2_bwd_f32", call.inp(case.x), call.inp(case.dy), b, h, w, c, out, accumulate)
    assert_same_bits(call.result(), want, "cp_maxpool3x3s2_bwd_f32")
    call = Call(hip_lib, device)
    out = call.out(want.shape, np.float32, fill, prev)
    call.run("cp_maxpool3x3s2_bwd_idx_f32", call.inp(ref.idx), call.inp(case.dy), b, h, w, c, out, accumulate)
    assert_same_bits(call.result(), want, "cp_maxpool3x3s2_bwd_idx_f32")


# ---- arg-max ----------------------------------------------------------------------------------------------------------------------------------------------------
def run_argmax(hip_lib, device, case, fill):
    call = Call(hip_lib, device)
    out = call.out((case.pixels,), np.uint8, fill)
    base = call.inp(case.buffer)
    assert Cs.argmax_route(case.classes, case.ld, case.offset, base & -base) == case.route
    call.run("cp_argmax_labels", base + 4 * case.offset, case.ld, case.classes, case.pixels, out)
    got = call.result()
    if not same_bits(got, case.want):
        rows = np.flatnonzero(got != case.want)
        names = {r: n for n, r in case.planted.items()}
        raise AssertionError("cp_argmax_labels (%s route): %d pixels differ: %s"
                             % (case.route, len(rows), [(int(r), names.get(int(r), "random"), int(got[r]), int(case.want[r])) for r in rows[:8]]))


@fills
@pytest.mark.parametrize("cfg", Cs.argmax_configs(), ids=lambda c: "k%d_ld%d_off%d" % c)
def test_argmax(hip_lib, device, cfg, fill):
    run_argmax(hip_lib, device, Cs.argmax_case(*cfg), fill)


@fills
@pytest.mark.parametrize("cfg", ((9, 12, 0), (5, 5, 0), (4, 4, 0), (8, 8, 0)), ids=lambda c: "k%d_ld%d_off%d" % c)
def test_argmax_past_the_cap(hip_lib, device, cfg, fill):
    """the three vector kernels (one, two, three float4 per pixel) and the scalar one"""
    case = Cs.argmax_case(*cfg, pixels=Cs.FLAT_BIG)
    assert Cs.past_cap(case.pixels) and case.route == ("scalar" if cfg[0] == 5 else "vector")
    run_argmax(hip_lib, device, case, fill)


# ---- pad, gather, scatter, axpby ------------------------------------------------------------------------------------------------------------------------------
@fills
@pytest.mark.parametrize("n", Cs.FLAT_SIZES)
def test_pad_channels(hip_lib, device, n, fill):
    f = Cs.flat(n)
    call = Call(hip_lib, device)
    out = call.out((n, 4), np.float32, fill)
    call.run("cp_pad_channels_3to4", call.inp(f.rgb), out, n)
    assert_same_bits(call.result(), R.pad3to4(f.rgb), "cp_pad_channels_3to4")


@fills
@pytest.mark.parametrize("n", Cs.FLAT_SIZES)
def test_gather(hip_lib, device, n, fill):
    f = Cs.flat(n)
    call = Call(hip_lib, device)
    out = call.out((n,), np.float32, fill)
    call.run("cp_gather_f32", call.inp(f.table), call.inp(f.idx), n, out)
    assert_same_bits(call.result(), R.gather(f.table, f.idx), "cp_gather_f32")


@fills
@pytest.mark.parametrize("accumulate", (0, 1), ids=("overwrite", "accumulate"))
@pytest.mark.parametrize("n", Cs.FLAT_SIZES)
def test_scatter(hip_lib, device, n, accumulate, fill):
    """targets that no index names keep the fill; with accumulate the named targets start from integers, so the sums are exact"""
    f = Cs.flat(n)
    used = f.idx[f.idx >= 0]
    before = np.frombuffer(bytes([fill]) * (8 * n), np.float32).copy()
    if accumulate and len(used):
        before[used] = f.table[used]
    call = Call(hip_lib, device)
    out = call.out((2 * n,), np.float32, fill, before)
    call.run("cp_scatter_f32", call.inp(f.src), call.inp(f.idx), n, out, accumulate)
    assert_same_bits(call.result(), R.scatter(f.src, f.idx, before, accumulate), "cp_scatter_f32")


@fills
@pytest.mark.parametrize("with_b", (1, 0), ids=("a_and_b", "a_alone"))
@pytest.mark.parametrize("n", Cs.FLAT_SIZES)
def test_axpby(hip_lib, device, n, with_b, fill):
    f = Cs.flat(n)
    alpha, beta = float(np.float32(0.3)), float(np.float32(-1.7))             # float32 values; neither product is exact
    ref = R.axpby(f.a, alpha, f.b if with_b else None, beta)
    call = Call(hip_lib, device)
    out = call.out((n,), np.float32, fill)
    call.run("cp_axpby_f32", call.inp(f.a), alpha, call.inp(f.b) if with_b else None, beta, n, out)
    assert_bounded(call.result(), ref, "cp_axpby_f32")


# ---- cross-checks between entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Cs.GUIDED_NAMES)
def test_zero_selection_is_nearest_neighbour(hip_lib, device, name):
    case = Cs.guided(name)
    b, h, w, c = case.shape
    call = Call(hip_lib, device)
    out = call.out((b, 2 * h, 2 * w, c), np.float32, FILLS[0])
    call.run("cp_guided_upsample_x2_f32", call.inp(case.x), call.inp(np.zeros((b, 2 * h, 2 * w), np.uint8)), b, h, w, c, out)
    assert_same_bits(call.result(), R.up2(case.x), "cp_guided_upsample_x2_f32 with sel = 0")


@pytest.mark.parametrize("name", Cs.GUIDED_NAMES)
def test_full_mask_is_the_fixed_weight_blend(hip_lib, device, name):
    """every tap matches in the interior; on the last row / column the padding cannot match, so the mask there is what one label everywhere gives"""
    case = Cs.guided(name)
    b, h, w, c = case.shape
    mask = R.match_mask(np.ones((b, 2 * h, 2 * w), np.uint8), np.ones((b, h, w), np.uint8))
    interior = np.broadcast_to(Cs.position_kind(h, w) == 0, mask.shape)
    assert (mask[interior] == 15).all() and (mask[~interior] != 15).all()
    call = Call(hip_lib, device)
    out = call.out((b, 2 * h, 2 * w, c), np.float32, FILLS[0])
    call.run("cp_guided_bilinear_upsample_x2_f32", call.inp(case.x), call.inp(mask), b, h, w, c, out)
    got = call.result()
    taps = R.up2(R.tap_values(case.x))                                                   # [B,2H,2W,4,C]
    p = R.SUB_WEIGHTS[R.sub_pixel(h, w)][None, :, :, :, None] * taps
    err = np.abs(got.astype(np.float64) - p.sum(3))
    assert (err[interior] <= ((4 + 4) * U * np.abs(p).sum(3))[interior]).all()


def test_label_pyramid_selection_and_match_mask_share_one_label_rule(hip_lib, device):
    from casapose_amd import ops

    rng = np.random.default_rng(11)
    lab0 = Cs.blobs(rng, 2, 24, 40, labels=4)
    labels, _, sel = ops.label_pyramid(torch.from_numpy(lab0).to(device))
    torch.cuda.synchronize(device)
    for lvl in range(3):
        hi, lo = labels[lvl].cpu().numpy(), labels[lvl + 1].cpu().numpy()
        assert np.array_equal(lo, hi[:, ::2, ::2])
        want_sel = R.sel_map(hi, lo)
        got_sel = sel[lvl].cpu().numpy()
        assert_same_bits(got_sel, want_sel, "sel[%d] of cp_label_pyramid" % lvl)
        b, hh, ww = hi.shape
        call = Call(hip_lib, device)
        out = call.out(hi.shape, np.uint8, FILLS[1])
        call.run("cp_guided_match_mask", call.inp(hi), call.inp(lo), b, hh, ww, out)
        mask = call.result()
        assert_same_bits(mask, R.match_mask(hi, lo), "cp_guided_match_mask on the pyramid's pair")
        some = mask != 0
        assert some.any() and (~some).any()
        assert (((mask[some] >> got_sel[some]) & 1) == 1).all() and not got_sel[~some].any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib, device):
    """each of these returns a nonzero status before anything is launched"""
    from casapose_amd._lib import CasaposeHipError

    call = Call(hip_lib, device)
    f = call.inp(np.zeros(4096, np.float32))
    u = call.inp(np.zeros(4096, np.uint8))
    o = call.out((4096,), np.float32, FILLS[1])
    bad = [("cp_guided_match_mask", (u, u, 1, 3, 4, o)), ("cp_guided_match_mask", (u, u, 1, 4, 3, o))]
    for ch in (6, 3):                                                  # channels % 4 != 0, every 4-channel-group kernel
        bad += [("cp_guided_bilinear_upsample_x2_f32", (f, u, 1, 2, 2, ch, o)),
                ("cp_guided_bilinear_upsample_x2_bwd_f32", (f, ch, u, 1, 2, 2, ch, o)),
                ("cp_upsample_bilinear_x2_f32", (f, 1, 2, 2, ch, o)),
                ("cp_upsample_bilinear_x2_bwd_f32", (f, ch, 1, 2, 2, ch, o)),
                ("cp_guided_upsample_x2_f32", (f, u, 1, 2, 2, ch, o)),
                ("cp_guided_upsample_x2_bwd_f32", (f, ch, u, 1, 2, 2, ch, o)),
                ("cp_maxpool3x3s2_f32", (f, 1, 4, 4, ch, None, None, 0, o)),
                ("cp_maxpool3x3s2_idx_f32", (f, 1, 4, 4, ch, o, o)),
                ("cp_maxpool3x3s2_bwd_f32", (f, f, 1, 4, 4, ch, o, 0)),
                ("cp_maxpool3x3s2_bwd_idx_f32", (u, f, 1, 4, 4, ch, o, 0))]
    bad += [("cp_guided_bilinear_upsample_x2_bwd_f32", (f, 4, u, 1, 2, 2, 8, o)),        # ld_dy < channels
            ("cp_upsample_bilinear_x2_bwd_f32", (f, 4, 1, 2, 2, 8, o)),
            ("cp_guided_upsample_x2_bwd_f32", (f, 4, u, 1, 2, 2, 8, o)),
            ("cp_argmax_labels", (f, 12, 0, 16, o)), ("cp_argmax_labels", (f, 256, 256, 16, o)), ("cp_argmax_labels", (f, 8, 9, 16, o)),
            ("cp_maxpool3x3s2_f32", (f, 1, 4, 4, 4, f, None, 0, o)), ("cp_maxpool3x3s2_f32", (f, 1, 4, 4, 4, None, f, 1, o))]
    for name, args in bad:
        with pytest.raises(CasaposeHipError):
            call.run(name, *args)
    assert call.result().tobytes() == bytes([FILLS[1]]) * (4096 * 4)          # nothing was launched
