"""The fp16-pair ("f16x2") range monitor of engine.ForwardPlan and train_engine.TrainPlan, and the training backward's policy (BackwardRange).  A slot
is four words (include/casapose_hip.h): [0] max |x| converted, [1] launches that reported, [2] a fused head's operand, [3] a backward overflow guard."""
from dataclasses import dataclass
from typing import TYPE_CHECKING, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

if TYPE_CHECKING:
    from .train_engine import WinoGemm


class armed:
    """context: the calling thread's launches inside report into the slot at device address `slot`, cleared on exit (a falsy slot: nothing)"""
    __slots__ = ("slot",)
    monitor_set = None   # cp_f16x2_monitor_set, bound on first use (every armed launch passes here: kept cheap)

    def __init__(self, slot: Optional[int]):
        self.slot = slot

    def __enter__(self):
        if self.slot:
            if armed.monitor_set is None:
                armed.monitor_set = _lib.load().cp_f16x2_monitor_set
            armed.monitor_set(self.slot)

    def __exit__(self, t, v, tb):
        if self.slot:
            armed.monitor_set(None)


def decode(words: np.ndarray, word: int = 0) -> Tuple[List[float], List[int]]:
    """slot words ([n][4], int32 or uint32) -> (max |x| of every slot, from word [0] or the head operand's word [2]; its launch count)"""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, 4)
    return np.ascontiguousarray(w[:, word]).view(np.float32).tolist(), w[:, 1].tolist()


def exponent_for(amax: float, e: int = 0) -> int:
    """the power of two that moves max |x| = amax, measured under 2^e, into [2^10, 2^11)"""
    return int(np.clip(e + 10 - int(np.floor(np.log2(amax))), -100, 100))


class SlotBuffer:
    """the monitor slots of one plan: the device int32 [n][4] buffer, its pinned host copy, the event of the reading in flight and the guards"""

    def __init__(self, n: int, device: torch.device):
        self.dev = torch.zeros(4 * n, dtype=torch.int32, device=device)
        self.host = torch.zeros(4 * n, dtype=torch.int32).pin_memory()
        self.event: Optional[torch.cuda.Event] = None
        self.guards: Optional[Tuple[torch.Tensor, torch.Tensor]] = None   # (word [3] of the guarded slots, the thresholds' bits): set_guards()

    def ptr(self, i: int) -> int:
        return self.dev.data_ptr() + 16 * i

    def zero(self, first: int = 0):
        self.dev[4 * first:].zero_()

    def set_guards(self, thresholds: np.ndarray, first: int):
        """word [3] of slots first.. = the float thresholds, now and behind every read_async() (clears the overflow bits)"""
        self.guards = (self.dev.view(-1, 4)[first:first + len(thresholds), 3], torch.from_numpy(thresholds.astype(np.float32).view(np.int32)).to(self.dev.device))
        self.guards[0].copy_(self.guards[1])

    def read(self, first: int = 0) -> np.ndarray:
        """the words of slots first.. as uint32 [n][4] (synchronises: calibration only)"""
        return self.dev[4 * first:].cpu().numpy().view(np.uint32).reshape(-1, 4)

    def read_async(self, stream: torch.cuda.Stream, extra: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """stream-ordered: the slots (and extra = (host, device)) to pinned memory, zeroed behind the copy, the guards rewritten, the event recorded"""
        self.host.copy_(self.dev, non_blocking=True)
        if extra is not None:
            extra[0].copy_(extra[1], non_blocking=True)
        self.dev.zero_()
        if self.guards is not None:
            self.guards[0].copy_(self.guards[1])
        self.event = torch.cuda.Event()
        self.event.record(stream)

    def poll(self) -> Optional[np.ndarray]:
        """the words of the last read_async() as uint32 [n][4] once they have landed, else None (never waits)"""
        if self.event is None or not self.event.query():
            return None
        self.event = None
        return self.host.numpy().copy().view(np.uint32).reshape(-1, 4)


@dataclass(eq=False)
class BwdSlot:
    """a backward GEMM on fp16 pairs and its slot: "direct" (a 3x3 layer under the loss factor, switched by `on`) or a Winograd GEMM with its e"""
    kind: str
    op: object
    entry: Optional["WinoGemm"] = None   # wino_dgrad: the op's wino_dgrad record (set_dgrad_exponent re-packs its weights)
    e: Optional[int] = None
    on: bool = False
    dead: bool = False             # a non-finite maximum ended its fp16-pair run for good
    slot: int = -1                 # index in the plan's SlotBuffer (behind the forward's slots)
    mon: Optional[int] = None      # that slot's device address once the plan has armed

    def __getitem__(self, field: str):   # read-only dict access: record["e"], record["on"] (TrainPlan._bwd_slots)
        return getattr(self, field)


class BackwardRange:
    """the host policy of the fp16-pair training backward (train_engine.train_bwd_f16x2), acting on ops through set_direct_dgrad_f16x2 and
    set_dgrad_exponent only.  The loss exponent E puts the largest max |dY| of the direct layers at [2^10, 2^11), a Winograd GEMM's e (None: the
    exact split, measuring) its own maximum; both follow a drift out of [2^7, 2^13), a non-finite maximum ends a GEMM's fp16-pair run."""

    def __init__(self, slots: List[BwdSlot], skip_host: Optional[torch.Tensor] = None):
        self.slots = list(slots)
        self.loss_exp = 0                             # power of two on the loss (the direct layers' dY carry it)
        self.moves: List[Tuple[str, int, int]] = []   # (layer, e before, e after): drift moves of the Winograd exponents
        self.skip_host = skip_host                    # pinned copy of ParamStore.skip, taken with every reading
        self.skip_base: Optional[int] = None          # skip[1] when the plan calibrated (None: not yet, or no monitor)
        self.skipped_steps = 0                        # optimizer steps this plan skipped, as of the last reading

    def _set_exponent(self, r: BwdSlot, e: Optional[int], stream: int):
        if r.kind == "wino_dgrad":
            r.op.set_dgrad_exponent(r.entry, e, stream)
        else:
            r.e = e

    def set_loss_exponent(self, e_new: int, stream: int):
        """move the power of two on the loss; the Winograd GEMMs' own exponents move the other way at the same moment (their operands carry it)"""
        d = e_new - self.loss_exp
        if d == 0:
            return
        self.loss_exp = e_new
        for r in self.slots:
            if r.kind != "direct" and r.e is not None and not r.dead:
                self._set_exponent(r, r.e - d, stream)

    def judge_direct(self, vals: Dict[int, float], stream: int):
        """vals: {slot index j: max |dY| as measured, loss factor included}: the loss exponent, then every direct layer's switch (direct_band)"""
        live = {j: v for j, v in vals.items() if np.isfinite(v) and v > 0.0}
        if not live:
            return
        top = max(live.values())
        shift = 0
        if not (2.0 ** 7 <= top < 2.0 ** 13):
            shift = 10 - int(np.floor(np.log2(top)))   # (unclipped: the band below judges the maxima with it)
            self.set_loss_exponent(exponent_for(top, self.loss_exp), stream)
        for j, v in vals.items():
            r = self.slots[j]
            if r.dead:
                continue
            if not np.isfinite(v):
                r.dead = True
                r.op.set_direct_dgrad_f16x2(False, stream)
                continue
            on = self.direct_band(r.on, v * 2.0 ** shift)
            if on != r.on:
                r.op.set_direct_dgrad_f16x2(on, stream)

    @staticmethod
    def direct_band(on: bool, v: float) -> bool:
        """a direct data gradient with max |dY| = v (loss factor included): joins the fp16 pair inside [1, 2^13], stays inside [0.25, HI]"""
        from . import engine

        return (0.25 <= v <= engine.F16X2_AMAX_HI) if on else (1.0 <= v <= 2.0 ** 13)

    def calibrate(self, words: np.ndarray, stream: int):
        """the plan's first backward (exact split, slots armed, words: uint32 [slots][4]): the Winograd exponents, then the loss exponent"""
        (amax, n), direct = decode(words), {}
        for j, r in enumerate(self.slots):
            if n[j] == 0 or r.e is not None:
                continue
            if r.kind == "direct":
                direct[j] = amax[j]
            elif np.isfinite(amax[j]) and amax[j] > 0.0:
                self._set_exponent(r, exponent_for(amax[j]), stream)
        self.judge_direct(direct, stream)

    def judge(self, words: np.ndarray, stream: int) -> Tuple[List[str], bool]:
        """one reading of the backward slots (uint32 [slots][4]) -> (the GEMMs that left the fp16 pair for good, whether anything moved: the plan
        then resets the slots, whose maxima since the copy were measured with the old factors and would move them a second time)"""
        before = self._state()
        (amax, n), out, direct = decode(words), [], {}
        for j, r in enumerate(self.slots):
            # a data gradient's slot holds max |V 2^e| (the transform applies the factor), a weight gradient's max |dM| (the GEMM applies it)
            if r.dead or n[j] == 0:
                continue
            a = amax[j]
            if r.kind == "direct":
                direct[j] = a
                continue
            scaled = a * (2.0 ** r.e if (r.kind == "wino_wgrad" and r.e is not None) else 1.0)
            if not np.isfinite(a):
                r.dead = True
                self._set_exponent(r, None, stream)
                out.append("%s %s gradient (max %.3g)" % (r.op.layer.name, "data" if r.kind == "wino_dgrad" else "weight", a))
            elif r.e is None:
                if a > 0.0:
                    self._set_exponent(r, exponent_for(a), stream)
            elif scaled > 0.0 and not (2.0 ** 7 <= scaled < 2.0 ** 13):
                e = exponent_for(scaled, r.e)
                self.moves.append((r.op.layer.name, r.e, e))
                self._set_exponent(r, e, stream)
        self.judge_direct(direct, stream)
        return out, self._state() != before

    def _state(self):
        return self.loss_exp, [r.e for r in self.slots], [r.on for r in self.slots]

    def guard_thresholds(self) -> np.ndarray:
        """every backward slot's overflow guard (word [3]): 65504 on what a slot measures as converted (direct dY with the loss factor, Winograd
        V x 2^e), 65504 2^-e on a weight gradient's dM (its GEMM applies 2^e); 0 (no guard) for a GEMM on the exact split"""
        out = np.zeros(len(self.slots), np.float32)
        for j, r in enumerate(self.slots):
            if r.dead:
                continue
            if r.kind == "direct":
                out[j] = 65504.0 if r.on else 0.0
            elif r.e is not None and (r.kind == "wino_dgrad" or r.op.layer.fwd_f16x2):
                out[j] = 65504.0 * 2.0 ** (-r.e if r.kind == "wino_wgrad" else 0)
        return out

    def count_skips(self, total: int) -> bool:
        """total = skip[1] as of a reading; True when this plan's first skipped step shows (the plan warns once)"""
        first = self.skipped_steps == 0
        self.skipped_steps = max(self.skipped_steps, total - (self.skip_base or 0))
        return first and self.skipped_steps > 0
