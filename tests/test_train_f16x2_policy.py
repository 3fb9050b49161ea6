"""Host-side policy of the fp16-pair backward (train_engine.TrainPlan._judge_direct / _set_loss_exponent): which power of two goes on the loss, which
layers join, how the Winograd GEMMs' own exponents move with it.  Pure Python on stub objects: no GPU, no library."""
import types

import numpy as np

from casapose_amd import train_engine as TE


class _Op:
    def __init__(self, name):
        self.layer = types.SimpleNamespace(name=name)
        self.bw16 = dict(on=False, mon=1, dead=False, e=None)
        self.calls = []

    def set_direct_dgrad_f16x2(self, on, stream):
        self.bw16["on"] = on
        self.calls.append(on)

    def set_dgrad_exponent(self, entry, e, stream):
        entry["f16"]["e"] = e


def _plan(direct_names, wino_exps):
    plan = types.SimpleNamespace(loss_exp=0, f16x2_bwd_moves=[])
    ops = [_Op(n) for n in direct_names]
    slots = [(op, op.bw16, "direct") for op in ops]
    for i, e in enumerate(wino_exps):
        w = dict(f16=dict(e=e, mon=1, dead=False))
        slots.append((_Op("wino%d" % i), w["f16"], w))
    plan._bwd_slots = lambda: slots
    plan._set_bwd_exponent = TE.TrainPlan._set_bwd_exponent
    plan._set_loss_exponent = types.MethodType(TE.TrainPlan._set_loss_exponent, plan)
    plan._judge_direct = types.MethodType(TE.TrainPlan._judge_direct, plan)
    return plan, ops, slots


def test_loss_exponent_puts_the_largest_layer_at_2_pow_10_and_admits_what_fits_the_band():
    plan, ops, slots = _plan(["a", "b", "c", "d"], [5, -3])
    # unscaled maxima as a first backward would measure them: 2^-11 .. 2^-24 (a spread of 2^13)
    vals = {0: 2.0 ** -11 * 1.3, 1: 2.0 ** -15, 2: 2.0 ** -20.5, 3: 2.0 ** -24}
    plan._judge_direct(vals, 0)
    assert plan.loss_exp == 21                                   # 1.3 * 2^-11 * 2^21 = 1.3 * 2^10 in [2^10, 2^11)
    assert [op.bw16["on"] for op in ops] == [True, True, True, False]   # 2^-24 * 2^21 = 2^-3 < 1: stays on the exact split
    assert [f["e"] for _, f, e in slots if e != "direct"] == [5 - 21, -3 - 21]   # the Winograd GEMMs' own factors give the loss factor back


def test_hysteresis_and_drift():
    plan, ops, _ = _plan(["a", "b"], [])
    plan._judge_direct({0: 2.0 ** -10, 1: 2.0 ** -12}, 0)
    e0 = plan.loss_exp
    assert e0 == 20 and all(op.bw16["on"] for op in ops)
    # readings now carry the factor.  Inside [2^7, 2^13): nothing moves; a layer at 0.3 (below 1 but above 0.25) stays where it is
    plan._judge_direct({0: 2.0 ** 12.5, 1: 0.3}, 0)
    assert plan.loss_exp == e0 and ops[1].bw16["on"] and ops[1].calls == [True]
    # ... below 0.25 it leaves
    plan._judge_direct({0: 2.0 ** 12.5, 1: 0.2}, 0)
    assert not ops[1].bw16["on"]
    # the largest maximum drifts to 2^14: the exponent follows (2^14 -> [2^10, 2^11): -4); the second layer, now at 2^9 * 2^-4 = 32, joins again
    plan._judge_direct({0: 2.0 ** 14, 1: 2.0 ** 9}, 0)
    assert plan.loss_exp == e0 - 4 and ops[0].bw16["on"] and ops[1].bw16["on"]   # 2^9 * 2^-4 = 32: inside [1, 2^13] -> joins again
    # a non-finite maximum ends a layer's fp16-pair run for good
    plan._judge_direct({0: float("inf"), 1: 2.0 ** 9}, 0)
    assert ops[0].bw16["dead"] and not ops[0].bw16["on"]
    plan._judge_direct({0: 2.0 ** 10, 1: 2.0 ** 9}, 0)
    assert not ops[0].bw16["on"]


def test_all_zero_gradients_change_nothing():
    plan, ops, _ = _plan(["a"], [3])
    plan._judge_direct({0: 0.0}, 0)
    assert plan.loss_exp == 0 and not ops[0].bw16["on"]


def _reading(vals):
    """uint32 [slots][4] as a reading of the backward slots: [0] float bits of max |operand|, [1] launches that reported"""
    w = np.zeros((len(vals), 4), np.uint32)
    w[:, 0] = np.asarray(vals, np.float32).view(np.uint32)
    w[:, 1] = [1 if v > 0 else 0 for v in vals]
    return w


def _judging_plan(direct_names, wino_exps):
    plan, ops, slots = _plan(direct_names, wino_exps)
    plan.device = np.zeros(len(slots), np.float32)   # the device slots' maxima, as the backward kernels leave them
    plan.resets = 0

    def reset():
        plan.device[:] = 0.0
        plan.resets += 1

    plan._reset_bwd_slots = reset
    plan._judge_bwd = types.MethodType(TE.TrainPlan._judge_bwd, plan)
    return plan, ops, slots


def test_a_move_is_not_repeated_by_the_stale_window_behind_its_reading():
    """The slots are copied at the end of a check step's forward and judged at the start of a later step; the backward in between still reports
    with the OLD factors.  Without a reset those maxima stay in the sticky slots, the next reading judges them as if measured with the NEW factors
    and moves a second time (loss exponent down by another 4, a Winograd exponent down again).  The plan resets the backward slots when anything
    moved, so the next reading holds only what the new factors produced."""
    plan, ops, slots = _judging_plan(["a", "b"], [3])
    plan.loss_exp = 20
    for op in ops:
        op.bw16["on"] = True
    # the window of reading 1: the largest direct layer drifted to 2^14 (loss exponent 20), the Winograd data gradient to 2^14 (e = 3).  Without
    # the reset the second reading would see 2^14 again and take the loss exponent to 12 (checked below through the reset count)
    window = [2.0 ** 14, 2.0 ** 9, 2.0 ** 14]
    plan.device[:] = window
    copy = _reading(plan.device)
    plan.device[:] = 0.0                 # zeroed behind the copy
    plan.device[:] = window              # the backward between the copy and the judgement: old factors, same maxima
    plan._judge_bwd(copy, 0)
    # the Winograd slot: its own drift (-4), then the loss move gives the factor back (+4)
    assert plan.loss_exp == 16 and slots[2][1]["e"] == 3 - 4 + 4 and plan.f16x2_bwd_moves == [("wino0", 3, -1)], (plan.loss_exp, slots[2][1]["e"])
    assert plan.resets == 1
    # the steps after the judgement, with the new factors: everything back at 2^10 / 2^5 / 2^10
    plan.device[:] = np.maximum(plan.device, [2.0 ** 10, 2.0 ** 5, 2.0 ** 10])
    moves = len(plan.f16x2_bwd_moves)
    plan._judge_bwd(_reading(plan.device), 0)
    assert plan.loss_exp == 16 and slots[2][1]["e"] == 3 and len(plan.f16x2_bwd_moves) == moves, (plan.loss_exp, slots[2][1]["e"])
    assert plan.resets == 1   # nothing moved: no reset


def test_an_unchanged_reading_does_not_reset_the_slots():
    plan, ops, slots = _judging_plan(["a"], [0])
    plan.loss_exp = 10
    ops[0].bw16["on"] = True
    plan._judge_bwd(_reading([2.0 ** 10, 2.0 ** 10]), 0)
    assert plan.resets == 0 and plan.loss_exp == 10 and slots[1][1]["e"] == 0



def test_keep_on_band_ends_at_hi():
    """the switch of a direct layer: joins inside [1, 2^13], stays inside [0.25, HI] with HI = 65504 / 4 = 16376, no longer
    2^14 = 16384.  (Inside _judge_direct no layer reaches the upper edge after a move -- the top lands in [2^10, 2^11) -- so the rule is pinned on
    its own.)"""
    band = TE.TrainPlan._direct_band
    assert band(False, 1.0) and band(False, 2.0 ** 13) and not band(False, 0.99) and not band(False, 2.0 ** 13 * 1.01)
    assert band(True, 0.25) and band(True, 16376.0) and not band(True, 0.24)
    for v in (16376.5, 16380.0, 16384.0):
        assert not band(True, v), v
