"""Host-side policy of the fp16-pair backward (f16x2_range.BackwardRange): which power of two goes on the loss, which layers join, how the
Winograd GEMMs' own exponents move with it, the overflow guards; and the slot decoding both plans share.  Pure Python on stub ops: no GPU, no library."""
import types

import numpy as np

from casapose_amd.f16x2_range import BackwardRange, BwdSlot, decode, exponent_for


class _Op:
    def __init__(self, name, fwd_f16x2=True):
        self.layer = types.SimpleNamespace(name=name, fwd_f16x2=fwd_f16x2)
        self.bw16 = None
        self.calls = []

    def set_direct_dgrad_f16x2(self, on, stream):
        self.bw16.on = on
        self.calls.append(on)

    def set_dgrad_exponent(self, entry, e, stream):
        entry["f16"].e = e


def _policy(direct_names, wino_exps):
    ops = [_Op(n) for n in direct_names]
    slots = []
    for op in ops:
        op.bw16 = BwdSlot("direct", op, mon=1)
        slots.append(op.bw16)
    for i, e in enumerate(wino_exps):
        w = {}
        w["f16"] = BwdSlot("wino_dgrad", _Op("wino%d" % i), entry=w, e=e, mon=1)
        slots.append(w["f16"])
    return BackwardRange(slots), ops, slots


def test_loss_exponent_puts_the_largest_layer_at_2_pow_10_and_admits_what_fits_the_band():
    pol, ops, slots = _policy(["a", "b", "c", "d"], [5, -3])
    # unscaled maxima as a first backward would measure them: 2^-11 .. 2^-24 (a spread of 2^13)
    vals = {0: 2.0 ** -11 * 1.3, 1: 2.0 ** -15, 2: 2.0 ** -20.5, 3: 2.0 ** -24}
    pol.judge_direct(vals, 0)
    assert pol.loss_exp == 21                                   # 1.3 * 2^-11 * 2^21 = 1.3 * 2^10 in [2^10, 2^11)
    assert [op.bw16.on for op in ops] == [True, True, True, False]   # 2^-24 * 2^21 = 2^-3 < 1: stays on the exact split
    assert [r.e for r in slots if r.kind != "direct"] == [5 - 21, -3 - 21]   # the Winograd GEMMs' own factors give the loss factor back


def test_hysteresis_and_drift():
    pol, ops, _ = _policy(["a", "b"], [])
    pol.judge_direct({0: 2.0 ** -10, 1: 2.0 ** -12}, 0)
    e0 = pol.loss_exp
    assert e0 == 20 and all(op.bw16.on for op in ops)
    # readings now carry the factor.  Inside [2^7, 2^13): nothing moves; a layer at 0.3 (below 1 but above 0.25) stays where it is
    pol.judge_direct({0: 2.0 ** 12.5, 1: 0.3}, 0)
    assert pol.loss_exp == e0 and ops[1].bw16.on and ops[1].calls == [True]
    # ... below 0.25 it leaves
    pol.judge_direct({0: 2.0 ** 12.5, 1: 0.2}, 0)
    assert not ops[1].bw16.on
    # the largest maximum drifts to 2^14: the exponent follows (2^14 -> [2^10, 2^11): -4); the second layer, now at 2^9 * 2^-4 = 32, joins again
    pol.judge_direct({0: 2.0 ** 14, 1: 2.0 ** 9}, 0)
    assert pol.loss_exp == e0 - 4 and ops[0].bw16.on and ops[1].bw16.on   # 2^9 * 2^-4 = 32: inside [1, 2^13] -> joins again
    # a non-finite maximum ends a layer's fp16-pair run for good
    pol.judge_direct({0: float("inf"), 1: 2.0 ** 9}, 0)
    assert ops[0].bw16.dead and not ops[0].bw16.on
    pol.judge_direct({0: 2.0 ** 10, 1: 2.0 ** 9}, 0)
    assert not ops[0].bw16.on


def test_all_zero_gradients_change_nothing():
    pol, ops, _ = _policy(["a"], [3])
    pol.judge_direct({0: 0.0}, 0)
    assert pol.loss_exp == 0 and not ops[0].bw16.on


def _reading(vals):
    """uint32 [slots][4] as a reading of the backward slots: [0] float bits of max |operand|, [1] launches that reported"""
    w = np.zeros((len(vals), 4), np.uint32)
    w[:, 0] = np.asarray(vals, np.float32).view(np.uint32)
    w[:, 1] = [1 if v > 0 else 0 for v in vals]
    return w


class _Device:
    """the device slots' maxima as the backward kernels leave them; reset() is what the plan does when a judgement moved something"""

    def __init__(self, n):
        self.maxima = np.zeros(n, np.float32)
        self.resets = 0

    def judge(self, pol, words):
        out, moved = pol.judge(words, 0)
        if moved:
            self.maxima[:] = 0.0
            self.resets += 1
        return out


def test_a_move_is_not_repeated_by_the_stale_window_behind_its_reading():
    """The slots are copied at the end of a check step's forward and judged at the start of a later step; the backward in between still reports
    with the OLD factors.  Without a reset those maxima stay in the sticky slots, the next reading judges them as if measured with the NEW factors
    and moves a second time (loss exponent down by another 4, a Winograd exponent down again).  The plan resets the backward slots when anything
    moved, so the next reading holds only what the new factors produced."""
    pol, ops, slots = _policy(["a", "b"], [3])
    dev = _Device(len(slots))
    pol.loss_exp = 20
    for op in ops:
        op.bw16.on = True
    # the window of reading 1: the largest direct layer drifted to 2^14 (loss exponent 20), the Winograd data gradient to 2^14 (e = 3).  Without
    # the reset the second reading would see 2^14 again and take the loss exponent to 12 (checked below through the reset count)
    window = [2.0 ** 14, 2.0 ** 9, 2.0 ** 14]
    dev.maxima[:] = window
    copy = _reading(dev.maxima)
    dev.maxima[:] = 0.0                 # zeroed behind the copy
    dev.maxima[:] = window              # the backward between the copy and the judgement: old factors, same maxima
    dev.judge(pol, copy)
    # the Winograd slot: its own drift (-4), then the loss move gives the factor back (+4)
    assert pol.loss_exp == 16 and slots[2].e == 3 - 4 + 4 and pol.moves == [("wino0", 3, -1)], (pol.loss_exp, slots[2].e)
    assert dev.resets == 1
    # the steps after the judgement, with the new factors: everything back at 2^10 / 2^5 / 2^10
    dev.maxima[:] = np.maximum(dev.maxima, [2.0 ** 10, 2.0 ** 5, 2.0 ** 10])
    moves = len(pol.moves)
    dev.judge(pol, _reading(dev.maxima))
    assert pol.loss_exp == 16 and slots[2].e == 3 and len(pol.moves) == moves, (pol.loss_exp, slots[2].e)
    assert dev.resets == 1   # nothing moved: no reset


def test_an_unchanged_reading_does_not_reset_the_slots():
    pol, ops, slots = _policy(["a"], [0])
    dev = _Device(len(slots))
    pol.loss_exp = 10
    ops[0].bw16.on = True
    dev.judge(pol, _reading([2.0 ** 10, 2.0 ** 10]))
    assert dev.resets == 0 and pol.loss_exp == 10 and slots[1].e == 0


def test_keep_on_band_ends_at_hi():
    """the switch of a direct layer: joins inside [1, 2^13], stays inside [0.25, HI] with HI = 65504 / 4 = 16376, no longer
    2^14 = 16384.  (Inside judge_direct no layer reaches the upper edge after a move -- the top lands in [2^10, 2^11) -- so the rule is pinned on
    its own.)"""
    band = BackwardRange.direct_band
    assert band(False, 1.0) and band(False, 2.0 ** 13) and not band(False, 0.99) and not band(False, 2.0 ** 13 * 1.01)
    assert band(True, 0.25) and band(True, 16376.0) and not band(True, 0.24)
    for v in (16376.5, 16380.0, 16384.0):
        assert not band(True, v), v


def test_exponent_for_targets_2_pow_10_and_clips():
    assert exponent_for(1.3 * 2.0 ** -11) == 21 and exponent_for(2.0 ** 10) == 0 and exponent_for(2.0 ** 11 * 0.999) == 0 and exponent_for(2.0 ** 11) == -1
    assert exponent_for(2.0 ** 14, 3) == -1 and exponent_for(2.0 ** 5, -2) == 3   # measured under 2^e: the new e
    assert exponent_for(1e-45) == 100 and exponent_for(3e38) == -100          # 10 + 149 and 10 - 127, clipped


def test_decode_reads_the_float_bits_and_the_launch_count():
    w = np.zeros((3, 4), np.uint32)
    w[:, 0] = np.array([1.5, 0.0, 65504.0], np.float32).view(np.uint32)
    w[:, 1] = [2, 0, 7]
    w[:, 2] = np.array([0.0, 0.0, 3.25], np.float32).view(np.uint32)
    w[:, 3] = [0, 0x80000000, 0]   # a fired guard does not touch the maximum
    for words in (w, w.view(np.int32), w.view(np.int32).reshape(-1)):   # as the device buffer's int32 words, flat or [n][4]
        amax, n = decode(words)
        assert amax == [1.5, 0.0, 65504.0] and n == [2, 0, 7]
        assert all(type(a) is float for a in amax) and all(type(c) is int for c in n)
        assert decode(words, 2)[0] == [0.0, 0.0, 3.25]


def test_guard_thresholds():
    """word [3] of every backward slot: 65504 where the slot measures the converted operand itself (a direct layer on the fp16 pair, a Winograd
    data gradient's V x 2^e), 65504 2^-e on a Winograd weight gradient's dM, 0 for what runs on the exact split or has left the pair for good"""
    pol, ops, slots = _policy(["on", "off", "dead"], [5, None])
    ops[0].bw16.on = True
    ops[2].bw16.on, ops[2].bw16.dead = True, True
    wg = [BwdSlot("wino_wgrad", _Op("wg", fwd_f16x2=f), e=e) for f, e in ((True, 3), (False, 3), (True, None), (True, -2))]
    wg[3].dead = True
    pol = BackwardRange(slots + wg)
    g = pol.guard_thresholds()
    assert g.dtype == np.float32
    assert g.tolist() == [65504.0, 0.0, 0.0, 65504.0, 0.0, 65504.0 / 8, 0.0, 0.0, 0.0]


def test_skipped_steps_count_from_the_calibration_and_warn_once():
    pol = BackwardRange([])
    pol.skip_base = 2   # skip[1] when the plan calibrated: steps another plan on the same store skipped
    assert not pol.count_skips(2) and pol.skipped_steps == 0
    assert pol.count_skips(3) and pol.skipped_steps == 1
    assert not pol.count_skips(5) and pol.skipped_steps == 3
    assert not pol.count_skips(5) and pol.skipped_steps == 3
