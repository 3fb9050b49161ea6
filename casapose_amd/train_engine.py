"""Training step of casapose_c_gcu5 on MI355X: forward with batch statistics, losses, hand-written
backward, Adam -- the path of train_casapose.py:494-611 (runnetwork/train_step) -- issued as a static
launch plan over libcasapose_hip.so.

Design
  * one flat fp32 MASTER parameter buffer (Keras layout per variable, names of SURVEY Appendix A) with a
    flat gradient and the two Adam moments beside it: one Adam launch and one all-reduce per step;
  * every kernel layout of a convolution (forward K order, halo fragment order, the flipped/transposed
    data-gradient packs) is a device GATHER of the master buffer through an index map built once by pushing
    an index ramp through the same host packers the inference engine uses; the packed weight gradient of
    cp_conv2d_wgrad_f32 goes back through the same map (scatter);
  * the plan is a tape: a list of ops with forward()/backward(); tensors with several consumers
    accumulate gradients in place (first writer overwrites, later writers add -- for convolution
    data-gradients through the kernel's fused residual input);
  * SyncBatchNormalization: the fp64 sum tables of cp_bn_stats_f32 / cp_bn_act_bwd_reduce_f32 are
    all-reduced across replicas when a process group is given (parallel.py), nothing else is exchanged in
    the forward/backward; the flat gradient is SUM-all-reduced before Adam (MirroredStrategy semantics,
    train_casapose.py:641-643).

The decoder-2 conditioning is the hard label map (arg-max of the logits or, with
train_vectors_with_ground_truth, the ground-truth segmentation: train_casapose.py:522-524) and is a constant
of the gradient, exactly like the saturated softmax of the reference (pose_models.py:547-552) whose
derivative vanishes in fp32.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, engine, parallel
from ._lib import ConvDesc, check
from .architecture import BILINEAR_DEFAULT, DECODER_DIMS_DEFAULT, GUIDED_DEFAULT, PARTIAL_DEFAULT, SHARED_DEFAULT, Arch, forward_order, graph  # noqa: F401
from .engine import BN_EPS
from .f16x2_range import BackwardRange, BwdSlot, SlotBuffer, armed, decode

BN_MOMENTUM = 0.99  # resnet.py:43 (Keras default elsewhere)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------
# parameters
# ------------------------------------------------------------------------------------------------
# gradient buckets = groups of consecutive layers whose all-reduce is launched as soon as the backward has passed them
BUCKET_STARTS = ("bn_data", "stage4_unit1_bn1", "pv_block_1_conv2d", "pv_block_6_prepare_conv2d")


# refreshes between two evaluations of max |w| for the f16x2 weight scale (a host synchronisation per layer).  16: an Adam step moves a weight by about
# the learning rate (<= 1e-3 here), so over 16 steps max |w| of an initialised layer (he_uniform: >= 0.036) cannot leave the 16x headroom; round 4's 256 could
F16X2_RESCALE_EVERY = int(os.environ.get("CASAPOSE_F16X2_RESCALE_EVERY", "16"))


def train_fwd_f16x2() -> bool:
    """The FORWARD convolutions of the training plan in the fp16 two-way split (csrc/split_f16.h: three products, fp32-level error) wherever the conv
    mode is "split"; CASAPOSE_TRAIN_FWD=split keeps the exact three-way bf16 split there too.  Only the forward: its operands are normalised
    activations and weights (scaled by a power of two); the backward's operands are gradients of arbitrary magnitude and stay on the exact bf16 split.
    Rounds 4 / 5 kept this an opt-in (57.2 against 53.4 ms per step) for two reasons.  (1) Accuracy: the exact split is BETTER than fp32 (operands
    exact) -- on the one ill-conditioned gradient comparison of the suite (config 13: the proxy-voting loss divides by |v|^2) the worst per-variable
    error is 6e-5 with the exact forward and 4.4e-3 with this one, which is what the fp32 MFMA gives as well
    (tests/test_gpu_train.py::test_config13_bpnp_step_at_448_matches_autograd): fp32-LEVEL, i.e. the reference's arithmetic.  (2) Nobody watched the
    fp16 range condition on activations that change with every step.  Round 6 removed (2): every f16x2 forward launch of the plan reports max |x| of what
    it converts into a device-side monitor slot (cp_f16x2_monitor_set, include/casapose_hip.h), the slots are judged every F16X2_TRAIN_CHECK_EVERY
    steps without a synchronisation, and an op whose operands have left the band moves its forward to the exact split for good (TrainPlan._poll_f16x2).
    With that the fp32-level forward is the DEFAULT."""
    return os.environ.get("CASAPOSE_TRAIN_FWD", "f16x2") == "f16x2"


def train_bwd_f16x2() -> bool:
    """The backward GEMMs of the training plan in the fp16 two-way split as well (round 6; CASAPOSE_TRAIN_BWD=split keeps the exact three-way bf16
    split).  A gradient has no natural magnitude, so the operand gets one, a power of two (exact): a Winograd GEMM's own 2^e (applied by the input
    transform of dY or the weight-gradient GEMM's loaders, taken back by the accumulators), and ONE 2^E on the loss for the DIRECT 3x3 layers
    (conv_hsplit converts its source as it is; TrainPlan.loss_exp: the flat gradient takes 2^-E before anything reads it).  The maxima come from
    monitor slots (max |dY| from cp_amax_f32 on the check steps): the FIRST backward of a plan runs on the exact split and ends with one synchronous
    reading, later ones are judged with the forward's without a synchronisation.  The rules: f16x2_range.BackwardRange (tools/debug/grad_ranges.py)."""
    return os.environ.get("CASAPOSE_TRAIN_BWD", "f16x2") == "f16x2"


# steps between two readings of the forward range monitor (asynchronous copy to pinned memory, judged at the start of a later step)
F16X2_TRAIN_CHECK_EVERY = max(1, int(os.environ.get("CASAPOSE_F16X2_TRAIN_CHECK_EVERY", "16")))


def f16x2_scale(cache: dict, weights: torch.Tensor) -> float:
    """the power of two the weights are multiplied by before their fp16 split (cp_f16x2_weight_scale: max |w| -> [2^11, 2^12), i.e. 16x headroom to
    the fp16 range).  It needs max |w| on the host, so it is re-evaluated every F16X2_RESCALE_EVERY refreshes, not every step."""
    n = cache.get("n", 0)
    cache["n"] = n + 1
    if "scale" not in cache or n % F16X2_RESCALE_EVERY == 0 or cache.get("max", 0.0) == 0.0:   # (an all-zero tensor has no scale yet: look again next time)
        cache["max"] = float(weights.abs().max())
        cache["scale"] = float(_lib.load().cp_f16x2_weight_scale(cache["max"]))
    return cache["scale"]


def conv_split_planes() -> int:
    """bf16-pipe mode of the shallow 3x3 convolutions of the TRAINING plan (csrc/conv_hsplit.hip), read from CASAPOSE_CONV_MODE:
    "split" (default) = 3 planes, exact three-way bf16 split, fp32-equivalent; "bf16" = 1 plane, operands rounded to bf16 (BASELINE configs[2]);
    "f32" = 0, the fp32-MFMA kernels."""
    mode = os.environ.get("CASAPOSE_CONV_MODE", "split")
    if mode not in ("split", "bf16", "f32"):
        raise ValueError("CASAPOSE_CONV_MODE must be split, bf16 or f32 (got %r)" % mode)
    return {"split": 3, "bf16": 1, "f32": 0}[mode]


class ParamStore:
    """Flat master parameters / gradients / Adam moments with named views."""

    def __init__(self, params: Dict[str, np.ndarray], device: torch.device):
        self.device = device
        self.offsets: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.state: Dict[str, torch.Tensor] = {}  # non-trainable: moving statistics
        chunks, off = [], 0
        rank = {n: i for i, n in enumerate(forward_order())}
        ordered = sorted(params.items(), key=lambda kv: rank.get(kv[0].split(".")[0], len(rank)))  # stable: unknown layers keep their order at the end
        for name, v in ordered:
            a = np.asarray(v, dtype=np.float32)
            if name.endswith(".moving_mean") or name.endswith(".moving_variance"):
                self.state[name] = torch.from_numpy(a.copy()).to(device)
                continue
            n = a.size
            self.offsets[name] = (off, tuple(a.shape))
            chunks.append(a.reshape(-1))
            pad = (-n) % 4  # keep every variable 16-byte aligned
            if pad:
                chunks.append(np.zeros(pad, np.float32))
            off += n + pad
        self.size = off
        self.theta = torch.from_numpy(np.concatenate(chunks)).to(device)
        self.grad = torch.zeros_like(self.theta)
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.step_count = 0
        # device-side skip of the fp16-pair backward (TrainPlan): int32 [skip flag (bit 31), steps skipped so far]; None = plain Adam.  skip[1] is
        # not part of export(): a store rebuilt from exported parameters counts its bias correction from step_count again.  step_count itself
        # (and with it training.Adam.iterations, the learning-rate schedule's clock) still advances on a skipped step: a skip is rare, one per
        # gradient spike, and the schedule stays tied to the batches seen
        self.skip: Optional[torch.Tensor] = None

    # ---- packed-weight arena: every kernel layout of every layer lives in ONE buffer refreshed by ONE gather of the master parameters
    def pack_reset(self):
        self._pack_parts: List[np.ndarray] = []
        self._pack_used = 0
        self._pack_cap = 8 * self.size
        self.pack_arena = torch.empty(self._pack_cap, dtype=torch.float32, device=self.device)
        self.pack_idx: Optional[torch.Tensor] = None

    def pack_alloc(self, idx_rel: np.ndarray, master_off: int) -> torch.Tensor:
        """A packed-layout buffer of len(idx_rel) floats whose element i is theta[master_off + idx_rel[i]] (0 where idx_rel[i] < 0)."""
        n = int(idx_rel.size)
        if getattr(self, "_pack_parts", None) is None or self.pack_idx is not None:
            self.pack_reset()
        npad = n + ((-n) % 4)
        if self._pack_used + npad > self._pack_cap:
            raise RuntimeError("packed-weight arena exhausted (%d + %d > %d floats)" % (self._pack_used, npad, self._pack_cap))
        part = np.full(npad, -1, np.int32)
        part[:n] = np.where(idx_rel >= 0, idx_rel.astype(np.int64) + master_off, -1).astype(np.int32)
        self._pack_parts.append(part)
        view = self.pack_arena[self._pack_used:self._pack_used + n]
        self._pack_used += npad
        return view

    def pack_finalize(self):
        self.pack_idx = torch.from_numpy(np.concatenate(self._pack_parts)).to(self.device) if self._pack_parts else None

    def pack_refresh(self, stream: int):
        """arena[i] = theta[pack_idx[i]]: all layers' kernel layouts in one launch"""
        if self.pack_idx is not None:
            check(_lib.load().cp_gather_f32(self.theta.data_ptr(), self.pack_idx.data_ptr(), self.pack_idx.numel(), self.pack_arena.data_ptr(), stream),
                  "cp_gather_f32(arena)")

    def view(self, name: str, of: Optional[torch.Tensor] = None) -> torch.Tensor:
        off, shape = self.offsets[name]
        n = int(np.prod(shape))
        return (self.theta if of is None else of)[off:off + n].view(shape)

    def grad_view(self, name: str) -> torch.Tensor:
        return self.view(name, self.grad)

    def export(self) -> Dict[str, np.ndarray]:
        out = {k: self.view(k).detach().cpu().numpy().copy() for k in self.offsets}
        out.update({k: v.detach().cpu().numpy().copy() for k, v in self.state.items()})
        return out

    def adam_step(self, lr: float, stream: int, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        self.step_count += 1
        if self.skip is None:
            check(_lib.load().cp_adam_step_f32(self.theta.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.size,
                                               lr, beta1, beta2, eps, self.step_count, grad_scale, stream), "cp_adam_step_f32")
            return
        # a step whose fp16-pair backward clamped an operand (TrainPlan.backward sets bit 31 of skip[0]) leaves theta, m and v as they are and
        # does not count: the kernel's bias correction uses step_count - skip[1], and skip[1] counts the skipped step behind it
        check(_lib.load().cp_adam_step_masked_f32(self.theta.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.size,
                                                  lr, beta1, beta2, eps, self.step_count, grad_scale, self.skip.data_ptr(), stream),
              "cp_adam_step_masked_f32")
        self.skip[1:].sub_(self.skip[:1] >> 31)   # (bit 31 set: the int32 is negative, >> 31 gives -1)


class TT:
    """Activation tensor [B,H,W,C] (contiguous) with an optional gradient buffer."""

    __slots__ = ("data", "grad", "has_grad", "needs_grad", "name")

    def __init__(self, data: torch.Tensor, needs_grad: bool = True, name: str = ""):
        self.data = data
        self.needs_grad = needs_grad
        self.grad = torch.empty_like(data) if needs_grad else None
        self.has_grad = False
        self.name = name

    @property
    def c(self):
        return self.data.shape[-1]

    @property
    def pixels(self):
        return self.data.numel() // self.data.shape[-1]


def _index_map(pack: Callable[[np.ndarray, np.ndarray], None], ramp_hwio: np.ndarray, n_out: int) -> np.ndarray:
    """Run a host packer over (index+1) stored as fp32 and recover the int32 gather map (-1 = zero fill)."""
    assert ramp_hwio.max() < (1 << 24)
    src = np.ascontiguousarray(ramp_hwio + 1, dtype=np.float32)
    dst = np.empty(n_out, dtype=np.float32)
    pack(src, dst)
    return (dst.astype(np.int64) - 1).astype(np.int32)


# bf16-pipe products per fp32 product of an arithmetic: exact three-way bf16 split, fp16 two-way split, hi + mid bf16 planes, operands rounded to bf16
PRODUCTS = {3: 6.0, _lib.PLANES_F16X2: 3.0, 2: 3.0, 1: 1.0}


class SplitWeights:
    """One weight set split into 2-byte operand planes.  `src` is its fp32 image, `arith` the arithmetic in force (a key of PRODUCTS), `planes` the
    buffer the consuming launch reads and `out_scale` the factor that launch multiplies its output by (1.0 unless arith is the fp16 pair: the weights
    are split as src * 2^k, f16x2_scale; a Winograd data gradient also takes the 2^e of its transformed dY back, `e`).  `shape` is None for the
    fragment stream of conv_hsplit / the stem (`idx`: its gather map from the master weights) and (groups, n, k) for a GEMM's [groups][n][k]."""

    def __init__(self, src: torch.Tensor, arith: int, shape: Optional[Tuple[int, int, int]] = None, idx: Optional[torch.Tensor] = None,
                 two_buffers: bool = False):
        self.src, self.arith, self.shape, self.idx = src, arith, shape, idx
        self.out_scale, self.e, self.cache = 1.0, None, {}   # (cache: f16x2_scale's counter, maximum and scale)
        # two_buffers (a Winograd GEMM): one buffer for the fp16 pair and one for the bf16 planes, each allocated by the first repack() that needs it
        self.two_buffers, self._other = two_buffers, None
        self.planes = None if two_buffers else self._alloc()

    products = property(lambda self: PRODUCTS[self.arith])

    def _alloc(self) -> torch.Tensor:   # (a fragment stream: 1 KiB per plane and 512 floats)
        n = self.src.numel() // 512 * (self.arith & 15) * 1024 if self.shape is None else _lib.load().cp_wino_split_weights_bytes(*self.shape)
        return torch.empty(n, dtype=torch.uint8, device=self.src.device)

    def set_arith(self, arith: int):
        """change the arithmetic; repack() makes the planes follow"""
        pair = _lib.PLANES_F16X2
        if self.two_buffers and (arith == pair) != (self.arith == pair):
            self.planes, self._other = self._other, self.planes
        self.arith = arith
        if self.shape is None and self.planes.numel() < self.src.numel() // 512 * (arith & 15) * 1024:   # (a demoted forward: two planes -> three)
            self.planes = self._alloc()

    def repack(self, stream: int):
        """src (just refreshed from the master weights) -> planes, in the arithmetic in force"""
        lib = _lib.load()
        pair = self.arith == _lib.PLANES_F16X2
        if self.planes is None:
            self.planes = self._alloc()
        scale = f16x2_scale(self.cache, self.src) if pair else 1.0
        self.out_scale = (1.0 if self.e is None else 2.0 ** (-self.e)) / scale
        if self.shape is None:
            check(lib.cp_conv_split_weights_scaled_f32(self.src.data_ptr(), self.src.numel(), self.arith, scale, self.planes.data_ptr(), stream),
                  "cp_conv_split_weights_scaled_f32")
        elif pair:
            check(lib.cp_wino_split_weights_scaled_f32(self.src.data_ptr(), *self.shape, self.arith, scale, self.planes.data_ptr(), stream),
                  "cp_wino_split_weights_scaled_f32")
        else:
            check(lib.cp_wino_split_weights_f32(self.src.data_ptr(), *self.shape, self.planes.data_ptr(), stream), "cp_wino_split_weights_f32")


@dataclass(eq=False)
class DgradPack:
    """the flipped / transposed kernel of one source's data gradient: gather maps and arena views (plain and halo order), descriptor, conv_hsplit planes"""
    idx: torch.Tensor
    w: torch.Tensor
    cout: int
    cin: int
    desc: ConvDesc
    idx_halo: Optional[torch.Tensor] = None
    w_halo: Optional[torch.Tensor] = None
    split: Optional[SplitWeights] = None
    deep: bool = False          # CASAPOSE_CONV_MODE=bf16: the direct bf16-operand kernel (csrc/conv_bf16d.hip) reads split.planes


@dataclass(eq=False)
class GemmRoute:
    """a 1x1 / stride-1 convolution as GEMMs rows x cin x cout on the bf16 matrix pipe (ConvOp.setup_gemm)"""
    rows: int
    cin: int
    idx_t: torch.Tensor               # [co][ci] -> master [ci][co]
    Uf: torch.Tensor                  # the transposed weights, fp32
    fwd: SplitWeights                 # planes of Uf
    dgrad: Optional[SplitWeights]     # planes of the master itself (None: no gradient wanted, or a later op of the tape reads the source too)
    dU: Optional[torch.Tensor] = None   # the weight gradient of the transposed GEMM (csrc/wino_wgrad_split.hip), where Routes.wgrad is gemm_split


@dataclass(eq=False)
class WinoGemm:
    """one Winograd GEMM of an op (ConvOp.setup_winograd): the forward (V kept for the weight gradient: dU, wdesc) or the data gradient of the source
    whose channels start at c0.  split: the planes of U (None: fp32 GEMM, CASAPOSE_WINO_GEMM=f32); slot: its backward GEMM on fp16 pairs -- the
    forward record's weight gradient, a data gradient's own GEMM (ps: the 2^e table its input transform applies)"""
    U: torch.Tensor
    ktot: int
    cout: int
    tp: int
    desc: ConvDesc
    split: Optional[SplitWeights] = None
    slot: Optional[BwdSlot] = None
    V: Optional[torch.Tensor] = None
    dU: Optional[torch.Tensor] = None
    wdesc: Optional[ConvDesc] = None
    c0: int = 0
    ps: Optional[torch.Tensor] = None


@dataclass(frozen=True)
class Routes:
    """The kernel family of every launch of a ConvOp, decided once (ConvOp.routes): constants of a finished plan -- shapes, pointers, leading
    dimensions, alignment, the tape order and the environment switches as they stood when the plan was built.  The ARITHMETIC of a family (fp16
    pair / exact split / exponents) moves at run time and stays in the SplitWeights / BwdSlot records.  dgrad has one entry per source; head_bn:
    pre_bn's backward recomputes the head's data gradient and the op launches nothing."""
    forward: str                        # gemm / wino / head_record / head_affine / head / stem_split / split / f32
    wgrad: str                          # head_affine / head / gemm_split / wino_split / wino_f32 / direct_split / f32
    dgrad: Tuple[Optional[str], ...]    # per source: None (no gradient wanted) / head_bn / head / gemm / deep / wino / split / f32


class TrainConv:
    """One convolution layer of the training plan: packs, descriptors, forward / wgrad / dgrad launches."""

    def __init__(self, store: ParamStore, key: str, layout: int, k: int, cout: int, sources: Sequence[Tuple[int, int]],
                 grad_sources: Sequence[bool]):
        lib = _lib.load()
        dev = store.device
        self.store, self.key, self.k, self.cout = store, key, k, cout
        self.sources = list(sources)
        self.name = key.rsplit(".", 1)[0]
        off, shape = store.offsets[key]
        n = int(np.prod(shape))
        self.master = store.theta[off:off + n]
        self.master_grad = store.grad[off:off + n]
        ramp = np.arange(n, dtype=np.int64).reshape(shape)
        hwio = ramp if layout == 0 else ramp.transpose(1, 2, 0, 3)  # [kh,kw,cin,cout] view of the master indices
        ns = len(sources)
        chans = (C.c_int * 2)(*([s[0] for s in sources] + [0] * (2 - ns)))
        real = (C.c_int * 2)(*([s[1] for s in sources] + [0] * (2 - ns)))
        self.ktot = lib.cp_conv_ktot(k, k, ns, chans)

        def packed(pack, view, n_out: int):
            """one kernel layout: the host packer `pack(src, dst)` pushed over the master indices `view` -> (device gather map, arena view)"""
            imap = _index_map(lambda src, dst: check(pack(src.ctypes.data, dst.ctypes.data), "pack " + key), view, n_out)
            return torch.from_numpy(imap).to(dev), store.pack_alloc(imap, off)

        self.idx_fwd, self.wp = packed(lambda s, d: lib.cp_conv_pack_weights_host(s, 0, k, k, cout, ns, chans, real, d), hwio, cout * self.ktot)
        self.dwp = torch.empty(cout * self.ktot, dtype=torch.float32, device=dev)
        self.idx_halo = self.wp_halo = None
        if k == 3 and cout <= 64 and sources[0][0] % 32 == 0 and (ns == 1 or sources[1][0] == 4 or sources[1][0] % 32 == 0):
            self.idx_halo, self.wp_halo = packed(lambda s, d: lib.cp_conv_pack_weights_halo_host(s, 0, cout, ns, chans, real, d), hwio,
                                                 lib.cp_conv_halo_weight_floats(cout, ns, chans))
        elif k == 7 and cout == 64 and ns == 1 and sources[0][0] == 4:  # the stem (csrc/conv_stem.hip): its packing travels in weights_halo
            self.idx_halo, self.wp_halo = packed(lambda s, d: lib.cp_conv_pack_weights_stem_host(s, 0, sources[0][1], d), hwio, 25 * 2 * 64 * 4)
        # bf16-pipe kernel (csrc/conv_hsplit.hip) for the shallow 3x3 layers: fp32 image of its fragment stream in the arena, bf16 planes beside it
        self.split: Optional[SplitWeights] = None
        planes = self.mode_planes = conv_split_planes()   # read ONCE per layer: the backward and the accounting reuse it (bench.py changes the variable between plans)
        self.fwd_f16x2 = planes == 3 and train_fwd_f16x2()   # forward launches of this layer in the fp16 two-way split
        fwd_np = _lib.PLANES_F16X2 if self.fwd_f16x2 else planes
        deep_dgrad = False
        if layout == 0 and sum(s_[0] for s_ in sources) >= 256 and cout >= 128:
            # bf16 conv mode: the DATA gradient of these layers runs on the direct bf16-operand kernel (csrc/conv_bf16d.hip; 1.2-1.6x the two-plane
            # Winograd path at bs 32) -- the forward stays Winograd: its transformed input V is what the weight gradient multiplies, its output
            # transform accumulates the batch statistics and its input transform applies the normalisation (CASAPOSE_BF16_DEEP=0: Winograd everywhere)
            deep_dgrad = planes == 1 and k == 3 and os.environ.get("CASAPOSE_BF16_DEEP", "1") != "0"
            planes = 0   # the deep ordinary 3x3 layers run as Winograd (engine.wino_eligible); partial convolutions (layout 1) of that size do not
        if planes and k == 3 and cout <= 512 and cout % 4 == 0 and sources[0][0] % 16 == 0 and sources[0][0] != 4 and (
                ns == 1 or (sources[1][0] == 4 and cout <= 32) or sources[1][0] % 16 == 0):
            idx, f32 = packed(lambda s, d: lib.cp_conv_pack_weights_split_host(s, 0, cout, ns, chans, real, d), hwio,
                              lib.cp_conv_split_weight_floats(cout, ns, chans))
            self.split = SplitWeights(f32, fwd_np, idx=idx)
        elif planes and k == 7 and cout == 64 and ns == 1 and sources[0][0] == 4 and os.environ.get("CASAPOSE_STEM_SPLIT", "1") != "0":
            # the stem on the bf16 matrix pipe (csrc/conv_stem_split.hip, round 4): same bookkeeping as the 3x3 layers -- fp32 image of the fragment
            # stream in the arena (re-gathered with every weight refresh), bf16 planes beside it; the weight gradient stays on the fp32 kernel
            idx, f32 = packed(lambda s, d: lib.cp_conv_pack_weights_stem_split_host(s, 0, sources[0][1], d), hwio, lib.cp_conv_stem_split_weight_floats())
            self.split = SplitWeights(f32, fwd_np, idx=idx)
        # data-gradient packs: per source that needs a gradient, the flipped / transposed kernel
        self.dgrad: List[Optional[DgradPack]] = []
        cpad = (cout + 31) // 32 * 32
        c0 = 0
        for s, (cs, cr) in enumerate(sources):
            if not grad_sources[s]:
                self.dgrad.append(None)
                c0 += cr
                continue
            sub = np.ascontiguousarray(hwio[::-1, ::-1, c0:c0 + cr, :].transpose(0, 1, 3, 2))  # [kh,kw,cout,cr]: taps flipped, in/out swapped
            dch = (C.c_int * 2)(cpad, 0)
            dre = (C.c_int * 2)(cout, 0)
            idx, w = packed(lambda s_, d, dch=dch, dre=dre, cr=cr: lib.cp_conv_pack_weights_host(s_, 0, k, k, cr, 1, dch, dre, d), sub,
                            cr * lib.cp_conv_ktot(k, k, 1, dch))
            ent = DgradPack(idx=idx, w=w, cout=cr, cin=cpad, desc=ConvDesc(), deep=deep_dgrad and cr % 128 == 0 and cr <= 512 and cpad % 16 == 0)
            if k == 3 and cr <= 64:
                ent.idx_halo, ent.w_halo = packed(lambda s_, d, dch=dch, dre=dre, cr=cr: lib.cp_conv_pack_weights_halo_host(s_, 0, cr, 1, dch, dre, d), sub,
                                                  lib.cp_conv_halo_weight_floats(cr, 1, dch))
            if (planes or ent.deep) and k == 3 and cr <= 512 and cr % 4 == 0:
                idx, f32 = packed(lambda s_, d, dch=dch, dre=dre, cr=cr: lib.cp_conv_pack_weights_split_host(s_, 0, cr, 1, dch, dre, d), sub,
                                  lib.cp_conv_split_weight_floats(cr, 1, dch))
                ent.split = SplitWeights(f32, planes or 1, idx=idx)
            self.dgrad.append(ent)
            c0 += cr
        self.desc = ConvDesc()
        self.layout = layout
        self.refresh_hooks: List[Callable[[int], None]] = []  # extra weight layouts owned by the ops (Winograd planes)
        if self._splits():
            self.refresh_hooks.append(self._refresh_split)

    def _splits(self) -> List[SplitWeights]:
        """the conv_hsplit / stem weight sets of this layer: the forward's, then every data gradient's"""
        return [sp for sp in [self.split] + [e.split for e in self.dgrad if e is not None] if sp is not None]

    def _refresh_split(self, stream: int):
        """fp32 fragment images (just re-gathered from the master weights) -> bf16 planes of the bf16-pipe kernel"""
        for sp in self._splits():
            sp.repack(stream)

    def refresh(self, stream: int, hooks_only: bool = False):
        """Re-pack the kernel layouts from the master weights (after an optimizer step / at start).  hooks_only: the plan refreshes the
        gather-type layouts of all layers with one launch over the packed-weight arena (ParamStore.pack_refresh)."""
        lib = _lib.load()
        m = self.master.data_ptr()
        if not hooks_only:
            for sp in self._splits():   # fp32 fragment images of the bf16-pipe kernel, then their planes
                check(lib.cp_gather_f32(m, sp.idx.data_ptr(), sp.idx.numel(), sp.src.data_ptr(), stream), "cp_gather_f32")
        for hook in self.refresh_hooks:
            hook(stream)
        if hooks_only:
            return
        packs = [(self.idx_fwd, self.wp), (self.idx_halo, self.wp_halo)]
        for ent in self.dgrad:
            if ent is not None:
                packs += [(ent.idx, ent.w), (ent.idx_halo, ent.w_halo)]
        for idx, w in packs:
            if idx is not None:
                check(lib.cp_gather_f32(m, idx.data_ptr(), idx.numel(), w.data_ptr(), stream), "cp_gather_f32")


class ConvOp:
    """raw = conv(sources) [* row_scale] [+ residual]; backward: wgrad + per-source dgrad."""

    def __init__(self, layer: TrainConv, srcs: Sequence[Tuple[TT, int]], out_ptr_ld: Tuple[torch.Tensor, int, int], batch: int, in_h: int,
                 in_w: int, stride=1, dilation=1, pad=0, tap_label=None, row_scale=None, residual: Optional[TT] = None,
                 out: Optional[TT] = None, dy_ptr_ld: Optional[Tuple[torch.Tensor, int, int]] = None):
        """srcs: (tensor, ld).  out_ptr_ld = (storage tensor, float offset, ld) of the raw output.  dy_ptr_ld: where the
        gradient of the output lives (default: out.grad)."""
        self.layer, self.srcs, self.out, self.residual = layer, list(srcs), out, residual
        self.tap_label, self.row_scale = tap_label, row_scale
        self.accumulate_master = False  # True: another convolution on the same weights has already written the master gradient
        self.stride, self.dil, self.pad = stride, dilation, pad
        self.batch, self.in_h, self.in_w = batch, in_h, in_w
        k = layer.k
        eff = (k - 1) * dilation + 1
        self.out_h = (in_h + 2 * pad - eff) // stride + 1
        self.out_w = (in_w + 2 * pad - eff) // stride + 1
        d = layer.desc   # (a fresh ConvDesc is all zeros: no epilogue, no fused head, automatic tile -- here and in the data gradients' below)
        d.batch, d.in_h, d.in_w, d.out_h, d.out_w = batch, in_h, in_w, self.out_h, self.out_w
        d.cout, d.kh, d.kw, d.stride, d.dilation, d.pad = layer.cout, k, k, stride, dilation, pad
        d.num_sources = len(srcs)
        for i, (t, ld) in enumerate(srcs):
            cs = d.src[i]
            cs.data, cs.channels, cs.ld, cs.mode = t.data.data_ptr(), layer.sources[i][0], ld, _lib.SRC_DIRECT
            cs.sel = cs.pre_scale = cs.pre_shift = None
        d.weights = layer.wp.data_ptr()
        d.weights_halo = _ptr(layer.wp_halo)
        d.tap_label, d.row_scale = _ptr(tap_label), _ptr(row_scale)
        d.residual = residual.data.data_ptr() if residual is not None else None
        d.residual_ld = layer.cout
        st, off, ld = out_ptr_ld
        d.out_raw, d.out_raw_ld = st.data_ptr() + 4 * off, ld
        d.out_act_ld = layer.cout
        self.dy_ptr_ld = dy_ptr_ld
        # the full-resolution 1x1 heads (32 -> K / ver_dim): streaming kernels on the Keras kernel itself (csrc/head1x1.hip) unless CASAPOSE_HEAD_CONV=generic
        self.head_fast = (k == 1 and stride == 1 and pad == 0 and len(srcs) == 1 and layer.sources[0] == (32, 32) and layer.cout <= 32
                          and tap_label is None and row_scale is None and residual is None and srcs[0][1] % 4 == 0
                          and os.environ.get("CASAPOSE_HEAD_CONV", "stream") != "generic")
        self._out_ptr_ld = out_ptr_ld
        self.record_prefix = None   # (tensor, ld, floats): dense rows this head copies in front of its own columns (TrainPlan._whole_records)
        # fused normalisation around a Winograd layer (TrainPlan._fuse_winograd): `stats_to` = the normalisation op whose batch statistics this
        # op's output transform accumulates; `pre_norm[s]` = the normalisation op whose normalise + activate this op's input transform of
        # source s applies itself (its stored activation is then never written)
        self.stats_to: Optional["BnActOp"] = None
        self.pre_norm: Dict[int, "BnActOp"] = {}
        self.pre_bn: Optional["BnActOp"] = None   # fused normalisation (TrainPlan._fuse_heads): this head reads the RAW tensor and applies pre_bn's tables itself
        self.gemm: Optional[GemmRoute] = None         # 1x1 GEMM route (setup_gemm)
        self.wino_fwd: Optional[WinoGemm] = None      # Winograd forward and data gradients by source index (setup_winograd)
        self.wino_dgrad: Dict[int, WinoGemm] = {}
        self._wV = self._wM = None                    # the plan's shared Winograd scratch (bind_winograd)
        self._cin = sum(s[1] for s in layer.sources)
        self._routes: Optional[Routes] = None         # the kernel family of every launch (routes): resolved once, by the plan or on first use
        self.mon_ptr: Optional[int] = None        # the f16x2 forward's monitor slot (TrainPlan._arm_f16x2)
        self.bw16: Optional[BwdSlot] = None   # the direct data / weight gradients' backward slot record (TrainPlan._finish_plan)
        # data-gradient descriptors
        for s, ent in enumerate(layer.dgrad):
            if ent is None:
                continue
            t, ld = srcs[s]
            assert t.needs_grad and ld == t.c
            g = ent.desc
            g.batch = batch
            g.in_h, g.in_w = (in_h + 2 * pad - (eff - 1), in_w + 2 * pad - (eff - 1)) if stride == 2 else (self.out_h, self.out_w)
            if stride == 2:
                assert dilation == 1 and g.in_h == 2 * self.out_h and g.in_w == 2 * self.out_w, "stride-2 data gradient expects even geometry"
            g.out_h, g.out_w = in_h, in_w
            g.cout, g.kh, g.kw, g.stride, g.dilation, g.pad = ent.cout, k, k, 1, dilation, dilation * (k - 1) - pad
            g.num_sources = 1
            g.src[0].channels = ent.cin
            g.src[0].mode = _lib.SRC_ZERO_INSERT_X2 if stride == 2 else _lib.SRC_DIRECT
            g.src[0].sel = g.src[0].pre_scale = g.src[0].pre_shift = None
            g.weights, g.weights_halo = ent.w.data_ptr(), _ptr(ent.w_halo)
            g.tap_label, g.row_scale = _ptr(tap_label), None
            g.residual_ld = ent.cout
            g.out_raw, g.out_raw_ld = t.grad.data_ptr(), t.c
            g.out_act_ld = t.c

    # ---- 1x1 / stride-1 shortcuts as plain GEMMs on the bf16 matrix pipe -----------------------------------------------------------------
    def setup_gemm(self, first_writer: bool = True):
        """The stage shortcuts with stride 1 (resnet.py:214-220 at output stride 8: stage 1, 3 and 4) are GEMMs rows x cin x cout.  In the conv modes
        `split` / `bf16` the forward and the data gradient run on the bf16-pipe GEMM of the Winograd path (csrc/wino_gemm_split.hip: exact
        three-way splits, or hi + mid planes in the bf16 mode) and, where cin and cout are multiples of 128, the weight gradient on its
        transposed partner (csrc/wino_wgrad_split.hip) -- instead of the fp32-MFMA implicit-GEMM kernel (84 TFLOP/s on the 256 -> 512 shortcut).
        CASAPOSE_SC_GEMM=0 keeps the fp32 kernels.  The GEMM data gradient writes without accumulating: it exists only for the FIRST writer of the
        source's gradient (first_writer: no later op of the tape reads the source; a stand-alone op is the only reader)."""
        assert self._routes is None, "the routes of %s are resolved" % self.layer.name
        L = self.layer
        planes = self.layer.mode_planes
        if not planes or os.environ.get("CASAPOSE_SC_GEMM", "1") == "0":
            return
        rows = self.batch * self.out_h * self.out_w
        cin = L.sources[0][0]
        st_, off_, ld_ = self._out_ptr_ld
        if (L.k != 1 or self.stride != 1 or self.pad != 0 or len(self.srcs) != 1 or L.sources[0][1] != cin or self.srcs[0][1] != cin or cin % 32
                or L.cout % 32 or rows % 128 or self.residual is not None or self.row_scale is not None or self.tap_label is not None
                or self.head_fast or ld_ != L.cout or L.layout != 0 or self.out is None
                or (self.dy_ptr_ld is not None and (self.dy_ptr_ld[1] != 0 or self.dy_ptr_ld[2] != L.cout))):
            return
        dev = L.master.device
        idx_t = (np.arange(cin, dtype=np.int32)[None, :] * L.cout + np.arange(L.cout, dtype=np.int32)[:, None]).reshape(-1)   # [co][ci] -> master [ci][co]
        exact = 3 if planes == 3 else 2
        Uf = torch.empty(L.cout * cin, dtype=torch.float32, device=dev)
        self.gemm = GemmRoute(rows=rows, cin=cin, idx_t=torch.from_numpy(idx_t).to(dev), Uf=Uf,
                              fwd=SplitWeights(Uf, _lib.PLANES_F16X2 if L.fwd_f16x2 else exact, (1, L.cout, cin)),   # U[co][ci] = W[ci][co]
                              # U[ci][co]: the master itself
                              dgrad=SplitWeights(L.master, exact, (1, cin, L.cout)) if L.dgrad[0] is not None and first_writer else None)
        L.refresh_hooks.append(self._refresh_gemm)

    def _refresh_gemm(self, stream: int):
        L, g = self.layer, self.gemm
        check(_lib.load().cp_gather_f32(L.master.data_ptr(), g.idx_t.data_ptr(), g.idx_t.numel(), g.Uf.data_ptr(), stream), "cp_gather_f32(%s)" % L.name)
        for sw in (g.fwd, g.dgrad):
            if sw is not None:
                sw.repack(stream)

    # ---- Winograd F(4x4,3x3) for the deep layers (csrc/wino.hip): forward and data gradient ------------------------
    def setup_winograd(self):
        """Decide which of this op's convolutions (forward, per-source data gradient) take the Winograd path and return the
        scratch sizes (floats of V, floats of M) they need; bind_winograd() completes the descriptors."""
        from .engine import TRAIN_WINO_GEMM_SPLIT, WinoConv, wino_eligible

        assert self._routes is None, "the routes of %s are resolved" % self.layer.name
        L = self.layer
        nv = nm = 0
        if L.k != 3 or self.stride != 1 or self.pad != self.dil or self.tap_label is not None or L.layout != 0:
            return 0, 0
        _, tp = WinoConv.tiles(self.batch, self.in_h, self.in_w, self.dil)
        dev = L.master.device
        # The training plan keeps the K >= 256 threshold of the fp32 GEMM.  Measured in round 3 with the dilated 128 -> 256 layer
        # (stage3_unit1_conv1) on the Winograd path as in the inference plan: no gain on the step (510 vs 519 images/s: its weight gradient
        # falls back to the fp32 grouped GEMM), and the F(4x4,3x3) rounding of one more layer in the forward moved the config-13 gradient
        # comparison from 6e-5 to 3e-3 (the proxy-voting loss divides by |v|^2: gradients are very sensitive to the forward's last bits).
        # In the bf16 conv mode (3e-2 gates) the same layer does take the Winograd path: no bf16-pipe kernel covers a dilated 3x3 directly, so it
        # would otherwise be the one deep layer left on the fp32 MFMA (forward 0.60 ms at 99 TFLOP/s).
        # Round 6: the fp32-LEVEL default (forward in the fp16 two-way split, the config-13 comparison gated at 1e-2 like the fp32 MFMA's) takes it too:
        # forward 0.59 -> Winograd GEMM on fp16 pairs, weight gradient through the Winograd planes instead of the fp32 MFMA kernel.
        split_gemm = self.dil > 1 and (self.layer.mode_planes == 1 or (self.layer.fwd_f16x2 and os.environ.get("CASAPOSE_TRAIN_WINO_DILATED_128", "1") == "1"))
        # the GEMMs on the bf16 matrix pipe read pre-split planes of U: hi + mid in the bf16 conv mode (three products, not fp32-equivalent: that
        # mode's gates are 3e-2), else the exact split; the forward's may be the fp16 pair.  bwd16: the backward GEMMs may move to the fp16 pair
        # (e = None while the exact split runs and the slot measures)
        exact = 2 if L.mode_planes == 1 else 3
        bwd16 = L.mode_planes == 3 and TRAIN_WINO_GEMM_SPLIT and train_bwd_f16x2()

        def record(cout, ktot, arith, **kw):
            U = torch.zeros(36 * cout * ktot, dtype=torch.float32, device=dev)
            return WinoGemm(U=U, ktot=ktot, cout=cout, tp=tp, desc=ConvDesc(),
                            split=SplitWeights(U, arith, (36, cout, ktot), two_buffers=True) if TRAIN_WINO_GEMM_SPLIT else None, **kw)

        if all(s[0] == s[1] for s in L.sources) and wino_eligible(3, 1, self.dil, self.pad, L.sources, L.cout, split_gemm=split_gemm):
            ktot = sum(s[0] for s in L.sources)
            # the forward's transformed input is kept per layer (not in the shared scratch): the weight gradient multiplies it again
            self.wino_fwd = record(L.cout, ktot, _lib.PLANES_F16X2 if L.fwd_f16x2 else exact,
                                   V=torch.zeros(36 * tp * ktot, dtype=torch.float32, device=dev),  # padding tiles stay zero
                                   dU=torch.empty(36 * L.cout * ktot, dtype=torch.float32, device=dev), wdesc=ConvDesc(),
                                   slot=BwdSlot("wino_wgrad", self) if bwd16 else None)   # the weight-gradient GEMM in f16x2: transformed dY x 2^e
            nv, nm = max(nv, 36 * tp * ktot), max(nm, 36 * tp * L.cout)
        c0 = 0
        for s, (ent, (cp, cr)) in enumerate(zip(L.dgrad, L.sources)):
            if ent is not None and L.cout % 32 == 0 and wino_eligible(3, 1, self.dil, self.dil, [(L.cout, L.cout)], cr, split_gemm=split_gemm):
                w = self.wino_dgrad[s] = record(cr, L.cout, exact, c0=c0)
                if bwd16:
                    w.slot = BwdSlot("wino_dgrad", self, entry=w)
                nv, nm = max(nv, 36 * tp * L.cout), max(nm, 36 * tp * cr)
            c0 += cr
        if self._wino_gemms():
            L.refresh_hooks.append(self._refresh_winograd)
        return nv, nm

    def _wino_gemms(self) -> List[WinoGemm]:
        return ([self.wino_fwd] if self.wino_fwd is not None else []) + list(self.wino_dgrad.values())

    def _refresh_winograd(self, stream: int):
        lib = _lib.load()
        L = self.layer
        cin, cout = self._cin, L.cout
        m = L.master.data_ptr()
        if self.wino_fwd is not None:
            c0 = k0 = 0
            for cp, cr in L.sources:  # master is HWIO [3][3][cin][cout]
                check(lib.cp_wino_transform_weights_f32(m + 4 * c0 * cout, 3 * cin * cout, cin * cout, cout, 1, 0, cr, cout, self.wino_fwd.ktot, k0,
                                                        self.wino_fwd.U.data_ptr(), stream), "cp_wino_transform_weights_f32")
                c0 += cr
                k0 += cp
        for s, w in self.wino_dgrad.items():  # flipped taps, K index = forward output channel, output = forward input channel
            check(lib.cp_wino_transform_weights_f32(m + 4 * w.c0 * cout, 3 * cin * cout, cin * cout, 1, cout, 1, cout, w.cout, w.ktot, 0,
                                                    w.U.data_ptr(), stream), "cp_wino_transform_weights_f32")
        for w in self._wino_gemms():
            if w.split is not None:
                w.split.repack(stream)

    def wgrad_f16x2(self) -> bool:
        """the direct weight gradient on fp16 pairs: dY inside the band (the switch its data gradient uses) and X too (the forward still f16x2)"""
        return self.bw16 is not None and self.bw16.on and not self.bw16.dead and self.layer.fwd_f16x2

    def set_direct_dgrad_f16x2(self, on: bool, stream: int):
        """the data gradients of this op on conv_hsplit (route split) on the fp16 two-way split (weights x 2^k re-packed as two fp16 planes) or back on
        the exact split"""
        self.bw16.on = on
        for s, route in enumerate(self.routes.dgrad):
            if route == "split":
                self.layer.dgrad[s].split.set_arith(_lib.PLANES_F16X2 if on else 3)
        self.layer._refresh_split(stream)

    def set_dgrad_exponent(self, w: WinoGemm, e: Optional[int], stream: int):
        """the power of two the transformed dY of this Winograd data gradient is multiplied by (None: back to the exact split); re-packs the weights"""
        w.slot.e = w.split.e = e
        w.split.set_arith(3 if e is None else _lib.PLANES_F16X2)
        if e is not None:
            if w.ps is None:
                w.ps = torch.empty(w.ktot, dtype=torch.float32, device=w.U.device)
            w.ps.fill_(2.0 ** e)
        self._refresh_winograd(stream)

    def demote_forward_to_exact_split(self, stream: int):
        """this op's forward on the exact three-way bf16 split from now on (its f16x2 operands left the fp16 range condition): re-packs the forward
        weights of whichever route the op takes -- the direct / stem kernel's planes, the 1x1 GEMM's, the Winograd GEMM's"""
        L = self.layer
        if not L.fwd_f16x2:
            return
        L.fwd_f16x2 = False
        for sw, refresh in ((L.split, L._refresh_split), (self.gemm and self.gemm.fwd, self._refresh_gemm),
                            (self.wino_fwd and self.wino_fwd.split, self._refresh_winograd)):
            if sw is not None and sw.arith == _lib.PLANES_F16X2:
                sw.set_arith(3)
                refresh(stream)

    def bind_winograd(self, V: torch.Tensor, M: torch.Tensor):
        self._wV, self._wM = V, M
        for w in self._wino_gemms():
            d = w.desc
            d.batch, d.in_h, d.in_w, d.out_h, d.out_w = 36, 1, w.tp, 1, w.tp
            d.cout, d.kh, d.kw, d.stride, d.dilation, d.pad = w.cout, 1, 1, 1, 1, 0
            d.num_sources = 1
            d.src[0].data, d.src[0].channels, d.src[0].ld, d.src[0].mode = V.data_ptr(), w.ktot, w.ktot, _lib.SRC_DIRECT
            d.weights = w.U.data_ptr()
            d.out_raw, d.out_raw_ld, d.out_act_ld, d.residual_ld = M.data_ptr(), w.cout, w.cout, w.cout
            d.group_rows, d.group_weight_stride = w.tp, w.cout * w.ktot
        if self.wino_fwd is not None:  # grouped 1x1 weight-gradient problem over the 36 planes: dU[p] = dM[p]^T V[p]
            w = self.wino_fwd
            g = w.wdesc
            g.batch, g.in_h, g.in_w, g.out_h, g.out_w = 1, 1, 36 * w.tp, 1, 36 * w.tp
            g.cout, g.kh, g.kw, g.stride, g.dilation, g.pad = w.cout, 1, 1, 1, 1, 0
            g.num_sources = 1
            g.src[0].data, g.src[0].channels, g.src[0].ld, g.src[0].mode = w.V.data_ptr(), w.ktot, w.ktot, _lib.SRC_DIRECT
            g.group_rows = w.tp

    def _wino_run(self, w: WinoGemm, srcs, residual_ptr, out_ptr, stream, pre=None, stats=None, mon=None):
        """srcs: list of (ptr, ld, channels); writes out_ptr[pix][w.cout] = conv (+ residual).  pre: {source index: (scale ptr, shift ptr, act)}
        applied by the input transform; stats: fp64 [2][cout] table the output transform fills with the output's batch statistics; mon: f16x2 range
        monitor slot armed around the input transforms (they report max |V| of what the f16x2 GEMM will convert; the GEMM itself stays un-armed:
        the padding rows of V hold stale data)."""
        lib = _lib.load()
        off = 0
        V = w.V if w.V is not None else self._wV
        with armed(mon):
            for i, (ptr, ld, ch) in enumerate(srcs):
                ps, pb, pa = (pre or {}).get(i, (None, None, 0))
                check(lib.cp_wino_input_transform_pre_f32(ptr, ld, ch, self.batch, self.in_h, self.in_w, self.dil, V.data_ptr(), w.ktot, off, ps, pb, pa, stream),
                      "cp_wino_input_transform_pre_f32(%s)" % self.layer.name)
                off += ch
        sw = w.split
        if sw is not None:
            check(lib.cp_wino_gemm_split_scaled_f32(V.data_ptr(), sw.planes.data_ptr(), self._wM.data_ptr(), 36 * w.tp, w.tp, w.ktot, w.cout, sw.arith, sw.out_scale,
                                                    stream), "cp_wino_gemm_split_scaled_f32(%s)" % self.layer.name)
        else:
            check(lib.cp_wino_gemm_f32(V.data_ptr(), w.U.data_ptr(), self._wM.data_ptr(), 36 * w.tp, w.tp, w.ktot, w.cout, stream),
                  "cp_wino_gemm_f32(%s)" % self.layer.name)
        check(lib.cp_wino_output_transform_stats_f32(self._wM.data_ptr(), w.cout, self.batch, self.in_h, self.in_w, self.dil, residual_ptr, w.cout, None, None,
                                                     None, 0, out_ptr, w.cout, None, w.cout, stats, stream),
              "cp_wino_output_transform_stats_f32(%s)" % self.layer.name)

    # ---- which kernel family a launch takes: decided once, read by the launches and by the accounting alike ---------------------------------
    def __setattr__(self, name, value):
        assert name not in ("pre_bn", "record_prefix") or getattr(self, "_routes", None) is None, "the routes of %s are resolved" % self.layer.name
        object.__setattr__(self, name, value)

    @property
    def routes(self) -> Routes:
        """TrainPlan._finish_plan resolves every op once its records stand (fused heads, whole records, the 1x1 GEMMs, Winograd and its fused
        normalisation); a stand-alone op resolves on first use.  setup_gemm, setup_winograd, pre_bn and record_prefix are closed from then on."""
        if self._routes is None:
            self._routes = self._resolve_routes()
        return self._routes

    def _resolve_routes(self) -> Routes:
        lib, L, g, w = _lib.load(), self.layer, self.gemm, self.wino_fwd
        head = self.head_fast and ("head" if self.pre_bn is None else "head_affine")
        if g is not None:
            fwd = "gemm"
        elif w is not None:
            fwd = "wino"
        elif head:
            fwd = head if self.record_prefix is None else "head_record"
        elif L.split is not None and L.k == 7:   # stride 2 / pad 3 / one 4-channel source: the range of the stem kernels
            fwd = "stem_split" if lib.cp_conv_selected_tile(C.byref(L.desc)) == _lib.TILE_STEM else "f32"
        else:
            fwd = "split" if L.split is not None and lib.cp_conv_split_applicable(C.byref(L.desc)) else "f32"
        # the weight-gradient GEMMs on the bf16 matrix pipe (csrc/wino_wgrad_split.hip: cout and cin multiples of 128) are the default wherever the
        # forward's GEMM is; CASAPOSE_WINO_WGRAD=f32 keeps the fp32 kernels.  conv_wgrad_split.hip covers 3x3 / stride 1 / pad 1, 32-multiple
        # sources + optional image, cout % 32 == 0
        wgemm = os.environ.get("CASAPOSE_WINO_WGRAD", "split") != "f32"
        if head:
            wgrad = head
        elif g is not None and wgemm and lib.cp_wino_wgrad_split_applicable(1, g.rows, L.cout, g.cin):
            wgrad = "gemm_split"
            g.dU = torch.empty(L.cout * g.cin, dtype=torch.float32, device=L.master.device)
        elif w is not None:
            wgrad = "wino_split" if w.split is not None and wgemm and lib.cp_wino_wgrad_split_applicable(36, w.tp, L.cout, w.ktot) else "wino_f32"
        else:
            wgrad = "direct_split" if L.mode_planes and lib.cp_conv_wgrad_split_applicable(C.byref(L.desc)) else "f32"
        dgrad: List[Optional[str]] = []
        for s, ent in enumerate(L.dgrad):
            if ent is None or head:
                dgrad.append(None if ent is None else "head" if self.pre_bn is None else "head_bn")
                continue
            # the descriptor as the launch hands it over, asked once.  The residual (the source's gradient, set by the launch only when another op
            # has written it) is probed SET, the stricter form with the same answer: it shares pointer and leading dimension with out_raw, and
            # ent.split exists only for cr % 4 == 0
            d = ent.desc
            d.src[0].data, d.src[0].ld = self._dy_at()
            d.residual = self.srcs[s][0].grad.data_ptr()
            if g is not None and g.dgrad is not None:
                dgrad.append("gemm")
            elif ent.deep and ent.split is not None and lib.cp_conv_bf16_deep_applicable(C.byref(d)):
                dgrad.append("deep")
            elif s in self.wino_dgrad:
                dgrad.append("wino")
            else:
                dgrad.append("split" if ent.split is not None and lib.cp_conv_split_applicable(C.byref(d)) else "f32")
        return Routes(fwd, wgrad, tuple(dgrad))

    def wgrad_arith(self) -> int:
        """the arithmetic this op's weight gradient runs in NOW (a key of PRODUCTS; 0: the fp32 MFMA)"""
        L, route = self.layer, self.routes.wgrad
        if route == "gemm_split":
            return 1 if L.mode_planes == 1 else 3   # CASAPOSE_CONV_MODE=bf16 rounds the operands of this GEMM to bf16 like the other weight gradients
        if route == "wino_split":
            # fp16 two-way split (train_bwd_f16x2): dM x 2^e from its monitor slot; V as it is -- the forward's monitor keeps it in the band
            # (a forward that left the band is demoted: L.fwd_f16x2 turns False and this GEMM returns to the exact split with it)
            f = self.wino_fwd.slot
            return _lib.PLANES_F16X2 if f is not None and f.e is not None and L.fwd_f16x2 else (1 if L.mode_planes == 1 else 3)
        if route == "direct_split":
            # both operands inside fp16's band: X watched by the forward's monitor, dY carrying the loss factor
            return _lib.PLANES_F16X2 if L.mode_planes == 3 and self.wgrad_f16x2() else L.mode_planes
        return 0

    def forward(self, stream: int):
        """The forward launch(es) of this layer; an f16x2 forward runs armed when the plan has given the op a monitor slot (mon_ptr)."""
        with armed(self.mon_ptr if self.layer.fwd_f16x2 and self.routes.forward != "wino" else None):   # (a Winograd forward arms its input transforms)
            self._forward(stream)

    def _forward(self, stream: int):
        lib = _lib.load()
        L, d, route = self.layer, self.layer.desc, self.routes.forward
        px = self.batch * self.out_h * self.out_w
        st_, off, old_ = self._out_ptr_ld
        if route == "gemm":
            g = self.gemm
            check(lib.cp_wino_gemm_split_scaled_f32(self.srcs[0][0].data.data_ptr(), g.fwd.planes.data_ptr(), d.out_raw, g.rows, g.rows, g.cin, L.cout, g.fwd.arith,
                                                    g.fwd.out_scale, stream), "cp_wino_gemm_split_scaled_f32(%s)" % L.name)
        elif route == "wino":
            srcs, pre = [], {}
            for i, ((t, ld), c) in enumerate(zip(self.srcs, L.sources)):
                bn = self.pre_norm.get(i)
                if bn is not None:   # read the RAW tensor; normalise + activate while loading
                    srcs.append((bn.x.data.data_ptr(), bn.x.c, c[0]))
                    pre[i] = (bn.scale.data_ptr(), bn.shift.data_ptr(), bn.act)
                else:
                    srcs.append((t.data.data_ptr(), ld, c[0]))
            self._wino_run(self.wino_fwd, srcs, self.residual.data.data_ptr() if self.residual is not None else None, d.out_raw, stream, pre=pre,
                           stats=self.stats_to.sums.data_ptr() if self.stats_to is not None else None, mon=self.mon_ptr if L.fwd_f16x2 else None)
        elif route == "head_record":
            bn = self.pre_bn
            pre, pre_ld, pre_n = self.record_prefix
            assert off == pre_n
            check(lib.cp_head1x1_fwd_affine_record_f32(bn.x.data.data_ptr(), bn.x.c, px, bn.scale.data_ptr(), bn.shift.data_ptr(), _ptr(bn.labels), bn.classes, bn.act,
                                                       L.master.data_ptr(), L.cout, pre.data_ptr(), pre_ld, pre_n, st_.data_ptr(), old_, stream),
                  "cp_head1x1_fwd_affine_record_f32(%s)" % L.name)
        elif route == "head_affine":
            bn = self.pre_bn
            check(lib.cp_head1x1_fwd_affine_f32(bn.x.data.data_ptr(), bn.x.c, px, bn.scale.data_ptr(), bn.shift.data_ptr(), _ptr(bn.labels), bn.classes, bn.act,
                                                L.master.data_ptr(), L.cout, st_.data_ptr() + 4 * off, old_, stream), "cp_head1x1_fwd_affine_f32(%s)" % L.name)
        elif route == "head":
            t, ld = self.srcs[0]
            check(lib.cp_head1x1_fwd_f32(t.data.data_ptr(), ld, px, L.master.data_ptr(), L.cout, st_.data_ptr() + 4 * off, old_, stream),
                  "cp_head1x1_fwd_f32(%s)" % L.name)
        elif route == "stem_split":
            check(lib.cp_conv2d_fwd_stem_split_scaled(C.byref(d), L.split.planes.data_ptr(), L.split.arith, L.split.out_scale, stream),
                  "cp_conv2d_fwd_stem_split(%s)" % L.name)
        elif route == "split":
            check(lib.cp_conv2d_fwd_split_scaled(C.byref(d), L.split.planes.data_ptr(), None, L.split.arith, L.split.out_scale, 1.0, stream),
                  "cp_conv2d_fwd_split(%s)" % L.name)
        else:
            check(lib.cp_conv2d_fwd_f32(C.byref(d), stream), "cp_conv2d_fwd_f32(%s)" % L.name)

    def executed_flops(self) -> Dict[str, float]:
        """FLOPs this op's launches EXECUTE per step, by matrix pipe: {"f32": fp32-MFMA FLOPs, "bf16": bf16-MFMA FLOPs} -- a Winograd layer counts
        its grouped GEMMs (36 planes x padded tiles), an arithmetic counts its PRODUCTS per fp32 product; forward + weight gradient + every data
        gradient.  (bench.py --mode train prices the step against the two pipes' peaks with it.)  Every launch is priced from routes, wgrad_arith
        and the weight records: the answers the launches read."""
        L, r = self.layer, self.routes
        out = {"f32": 0.0, "bf16": 0.0}
        direct = 2.0 * float(self.batch * self.out_h * self.out_w) * L.k * L.k * self._cin * L.cout

        def add(sw: Optional[SplitWeights], flops: float):   # a launch reading split weights runs on the bf16 pipe, one without on the fp32 MFMA
            out["f32" if sw is None else "bf16"] += (1.0 if sw is None else sw.products) * flops

        w = self.wino_fwd
        gemm = 2.0 * 36 * w.tp * w.ktot * w.cout if r.forward == "wino" else direct
        add({"gemm": self.gemm and self.gemm.fwd, "wino": w and w.split, "stem_split": L.split, "split": L.split}.get(r.forward), gemm)
        arith = self.wgrad_arith()
        if r.wgrad == "direct_split":   # conv_wgrad_split.hip takes the 32-multiple sources; the image source stays on the fp32 MFMA
            big = sum(s[1] for s in L.sources if s[0] != 4)
            out["bf16"] += PRODUCTS[arith] * direct * big / self._cin
            out["f32"] += direct * (self._cin - big) / self._cin
        else:
            out["bf16" if arith else "f32"] += (PRODUCTS[arith] if arith else 1.0) * gemm
        m_in = float(self.batch * self.in_h * self.in_w)
        for s, route in enumerate(r.dgrad):
            if route is None:
                continue
            ent = L.dgrad[s]
            d = 2.0 * m_in * L.k * L.k * ent.cin * ent.cout
            if route == "deep":
                out["bf16"] += d
            elif route == "wino":
                w = self.wino_dgrad[s]
                add(w.split, 2.0 * 36 * w.tp * w.ktot * w.cout)
            else:   # (the heads' streaming kernels, head_bn's recomputation included, are fp32 like the generic kernel)
                add({"gemm": self.gemm and self.gemm.dgrad, "split": ent.split}.get(route), d)
        return out

    def _dy_at(self) -> Tuple[int, int]:
        """(address, leading dimension) of the output's gradient: a constant of the plan"""
        if self.dy_ptr_ld is not None:
            st, off, ld = self.dy_ptr_ld
            return st.data_ptr() + 4 * off, ld
        return self.out.grad.data_ptr(), self.out.c

    def _dy(self):
        assert self.dy_ptr_ld is not None or self.out.has_grad, "gradient of %s not produced" % self.layer.name
        return self._dy_at()

    def backward(self, stream: int):
        """weight gradient, then the data gradient of every source"""
        self.backward_wgrad(stream)
        self.backward_dgrad(stream)

    def backward_wgrad(self, stream: int):
        lib = _lib.load()
        L = self.layer
        dy, dy_ld = self._dy()
        d = L.desc  # one op per layer: filled by this op's constructor
        acc = 1 if self.accumulate_master else 0
        px = self.batch * self.out_h * self.out_w
        route = self.routes.wgrad
        if route == "head_affine":   # the activated input is recomputed from the raw tensor
            bn = self.pre_bn
            check(lib.cp_head1x1_wgrad_affine_f32(bn.x.data.data_ptr(), bn.x.c, bn.scale.data_ptr(), bn.shift.data_ptr(), _ptr(bn.labels), bn.classes, bn.act,
                                                  dy, dy_ld, px, L.cout, L.master_grad.data_ptr(), acc, stream), "cp_head1x1_wgrad_affine_f32(%s)" % L.name)
        elif route == "head":
            t, ld = self.srcs[0]
            check(lib.cp_head1x1_wgrad_f32(t.data.data_ptr(), ld, dy, dy_ld, px, L.cout, L.master_grad.data_ptr(), acc, stream), "cp_head1x1_wgrad_f32(%s)" % L.name)
        elif route == "gemm_split":
            # dU[co][ci] = sum_rows dY[row][co] A[row][ci] on the bf16 pipe, then through the transpose map into the master gradient [ci][co]
            g = self.gemm
            check(lib.cp_wino_wgrad_split_f32(dy, self.srcs[0][0].data.data_ptr(), g.dU.data_ptr(), 1, g.rows, L.cout, g.cin, self.wgrad_arith(), stream),
                  "cp_wino_wgrad_split_f32(%s)" % L.name)
            check(lib.cp_scatter_f32(g.dU.data_ptr(), g.idx_t.data_ptr(), g.idx_t.numel(), L.master_grad.data_ptr(), acc, stream), "cp_scatter_f32(%s)" % L.name)
        elif route in ("wino_split", "wino_f32"):
            # weight gradient through the Winograd planes: a quarter of the MFMA work of the direct kernel (V kept from the forward)
            w = self.wino_fwd
            cin, cout = self._cin, L.cout
            f = w.slot if route == "wino_split" else None
            with armed(f.mon if f is not None and not f.dead else None):   # the transform reports max |dM|
                check(lib.cp_wino_dy_transform_f32(dy, dy_ld, cout, self.batch, self.in_h, self.in_w, self.dil, self._wM.data_ptr(), stream),
                      "cp_wino_dy_transform_f32(%s)" % L.name)
            arith = self.wgrad_arith()
            if arith == _lib.PLANES_F16X2:   # the grouped GEMM dU[p] = dM[p]^T V[p] on the 2-byte pipe (csrc/wino_wgrad_split.hip): fp16 pairs, dM x 2^e
                check(lib.cp_wino_wgrad_split_scaled_f32(self._wM.data_ptr(), w.V.data_ptr(), w.dU.data_ptr(), 36, w.tp, cout, w.ktot, arith, 2.0 ** f.e, 1.0, stream),
                      "cp_wino_wgrad_split_scaled_f32(%s)" % L.name)
            elif arith:   # ... exact splits (fp32-equivalent), or operands rounded to bf16
                check(lib.cp_wino_wgrad_split_f32(self._wM.data_ptr(), w.V.data_ptr(), w.dU.data_ptr(), 36, w.tp, cout, w.ktot, arith, stream),
                      "cp_wino_wgrad_split_f32(%s)" % L.name)
            else:
                check(lib.cp_conv2d_wgrad_f32(C.byref(w.wdesc), self._wM.data_ptr(), cout, w.dU.data_ptr(), 0, stream), "cp_conv2d_wgrad_f32(wino %s)" % L.name)
            c0 = k0 = 0
            for cp_, cr in L.sources:
                check(lib.cp_wino_weight_grad_f32(w.dU.data_ptr(), cr, cout, w.ktot, k0, 3 * cin * cout, cin * cout, cout, 1,
                                                  L.master_grad.data_ptr() + 4 * c0 * cout, acc, stream), "cp_wino_weight_grad_f32(%s)" % L.name)
                c0 += cr
                k0 += cp_
        else:
            arith = self.wgrad_arith()
            if arith:   # bf16 matrix pipe (csrc/conv_wgrad_split.hip): same packed result
                with armed(self.bw16.mon if arith == _lib.PLANES_F16X2 else None):   # (the fp16 pair: dY's overflow guard, every step)
                    check(lib.cp_conv2d_wgrad_split(C.byref(d), dy, dy_ld, L.dwp.data_ptr(), 0, arith, stream), "cp_conv2d_wgrad_split(%s)" % L.name)
            else:
                check(lib.cp_conv2d_wgrad_f32(C.byref(d), dy, dy_ld, L.dwp.data_ptr(), 0, stream), "cp_conv2d_wgrad_f32(%s)" % L.name)
            check(lib.cp_scatter_f32(L.dwp.data_ptr(), L.idx_fwd.data_ptr(), L.idx_fwd.numel(), L.master_grad.data_ptr(), acc, stream), "cp_scatter_f32")

    def backward_dgrad(self, stream: int):
        lib = _lib.load()
        L = self.layer
        dy, dy_ld = self._dy()
        for s, route in enumerate(self.routes.dgrad):
            if route is None or route == "head_bn":   # (pre_bn's backward recomputes the head's data gradient inside its two passes, cp_head1x1_bn_bwd_*)
                continue
            ent, (t, _) = L.dgrad[s], self.srcs[s]
            if route == "head":
                readable = (self.dy_ptr_ld[2] - self.dy_ptr_ld[1] % self.dy_ptr_ld[2]) if self.dy_ptr_ld is not None else self.out.c
                check(lib.cp_head1x1_dgrad_f32(dy, dy_ld, min(32, readable), self.batch * self.out_h * self.out_w, L.master.data_ptr(), L.cout,
                                               t.grad.data_ptr(), t.c, 1 if t.has_grad else 0, stream), "cp_head1x1_dgrad_f32(%s)" % L.name)
            elif route == "gemm":
                # dA[row][ci] = sum_co dY[row][co] W[ci][co]; the GEMM writes (no accumulation): no later op of the tape reads this source
                # (setup_gemm's first_writer), so this backward runs BEFORE the other consumers of its input, which then accumulate into it
                assert not t.has_grad, "the GEMM data gradient of %s is not the first writer of its source's gradient" % L.name
                g = self.gemm
                check(lib.cp_wino_gemm_split_planes_f32(dy, g.dgrad.planes.data_ptr(), t.grad.data_ptr(), g.rows, g.rows, L.cout, g.cin, g.dgrad.arith, stream),
                      "cp_wino_gemm_split_planes_f32(dgrad %s)" % L.name)
            elif route == "wino":  # stride 1, so the data gradient lives on the forward's input grid
                w = self.wino_dgrad[s]
                f = w.slot
                pre = {0: (w.ps.data_ptr(), None, _lib.ACT_NONE)} if f is not None and f.e is not None else None   # (a factor only: no shift table)
                self._wino_run(w, [(dy, dy_ld, L.cout)], t.grad.data_ptr() if t.has_grad else None, t.grad.data_ptr(), stream, pre=pre,
                               mon=f.mon if f is not None and not f.dead else None)
            else:
                g, sp = ent.desc, ent.split   # (its source: dY, set when the routes were resolved)
                g.residual = t.grad.data_ptr() if t.has_grad else None
                if route == "deep":
                    check(lib.cp_conv2d_fwd_bf16_deep(C.byref(g), sp.planes.data_ptr(), stream), "dgrad bf16 deep(%s)" % L.name)
                elif route == "split":
                    # the fp16 pair runs armed on every step: max |dY| into the op's backward slot, and its overflow guard
                    with armed(self.bw16.mon if sp.arith == _lib.PLANES_F16X2 and self.bw16 is not None else None):
                        check(lib.cp_conv2d_fwd_split_scaled(C.byref(g), sp.planes.data_ptr(), None, sp.arith, sp.out_scale, 1.0, stream), "dgrad split(%s)" % L.name)
                else:
                    check(lib.cp_conv2d_fwd_f32(C.byref(g), stream), "dgrad(%s)" % L.name)
            t.has_grad = True
        if self.residual is not None:
            add_grad(self.residual, dy, self.out.pixels * self.out.c, stream)


def add_grad(t: TT, src_ptr: int, n: int, stream: int):
    lib = _lib.load()
    if t.has_grad:
        check(lib.cp_axpby_f32(t.grad.data_ptr(), 1.0, src_ptr, 1.0, n, t.grad.data_ptr(), stream), "cp_axpby_f32")
    else:
        check(lib.cp_axpby_f32(src_ptr, 1.0, None, 0.0, n, t.grad.data_ptr(), stream), "cp_axpby_f32")
        t.has_grad = True


class BnActOp:
    """y = act(gamma[l]*(x-mean)*rstd + beta[l]) with batch statistics (optionally all-reduced across replicas)."""

    def __init__(self, plan: "TrainPlan", name: str, x: TT, y: TT, act: int, gamma: Optional[str], beta: Optional[str],
                 labels: Optional[torch.Tensor] = None, classes: int = 1, row_scale: Optional[torch.Tensor] = None,
                 pad_one: bool = False):
        self.plan, self.name, self.x, self.y, self.act = plan, name, x, y, act
        self.gamma_key, self.beta_key, self.labels, self.classes = gamma, beta, labels, classes
        self.row_scale = row_scale  # partial convolution: x = row_scale * conv, so d conv = row_scale * dx
        self.pad_one = pad_one      # bn_data: channel 3 is padding; its output is the constant 1 (see TrainPlan)
        C_ = x.c
        dev = x.data.device
        f64 = dict(dtype=torch.float64, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.sums = torch.zeros(2 * C_, **f64)
        self.mean = torch.zeros(C_, **f32)
        self.rstd = torch.zeros(C_, **f32)
        self.scale = torch.zeros(classes, C_, **f32)
        self.shift = torch.zeros(classes, C_, **f32)
        self.gamma_full = torch.ones(classes, C_, **f32)
        self.beta_full = torch.zeros(classes, C_, **f32)
        self._redchan = torch.zeros(classes * C_ * 2 + C_ * 2, **f64)   # adjacent: the backward reduce zeroes both with one fill
        self.red = self._redchan[:classes * C_ * 2]
        self.chan = self._redchan[classes * C_ * 2:]
        st = plan.store
        self.real_c = st.offsets[beta][1][-1] if beta else C_
        self.gamma_p = st.view(gamma) if gamma else None
        self.beta_p = st.view(beta) if beta else None
        self.dgamma_p = st.grad_view(gamma) if gamma else None
        self.dbeta_p = st.grad_view(beta) if beta else None
        self.mm = st.state.get(name + ".moving_mean")
        self.mv = st.state.get(name + ".moving_variance")
        # fused normalisation (TrainPlan._fuse_heads): `head` = the 1x1 head ConvOp that consumes y alone; y and its gradient are then never
        # written -- the head applies scale / shift itself and this op's backward recomputes the head's data gradient (csrc/head1x1.hip)
        self.head: Optional[ConvOp] = None
        # ... around Winograd layers (TrainPlan._fuse_winograd): `stats_from` = the convolution whose output transform has already filled
        # self.sums; `consumer` = the convolution whose input transform applies scale / shift / activation itself (y is never written)
        self.stats_from: Optional[ConvOp] = None
        self.consumer: Optional[ConvOp] = None

    def forward(self, stream: int):
        lib = _lib.load()
        x, p = self.x, self.plan
        C_ = x.c
        if self.stats_from is None:
            check(lib.cp_bn_stats_f32(x.data.data_ptr(), x.pixels, C_, C_, self.sums.data_ptr(), stream), "cp_bn_stats_f32(%s)" % self.name)
        n = p.all_reduce_stats(self.sums, x.pixels)
        upd = p.update_moving and self.mm is not None
        check(lib.cp_bn_finalize_f32(self.sums.data_ptr(), float(n), C_, self.real_c, self.classes, _ptr(self.gamma_p), _ptr(self.beta_p), BN_EPS,
                                     1 if self.pad_one else 0, BN_MOMENTUM, _ptr(self.mm) if upd else None, _ptr(self.mv) if upd else None,
                                     self.mean.data_ptr(), self.rstd.data_ptr(), self.gamma_full.data_ptr(), self.beta_full.data_ptr(),
                                     self.scale.data_ptr(), self.shift.data_ptr(), stream), "cp_bn_finalize_f32(%s)" % self.name)
        if self.head is None and self.consumer is None:
            self.materialize(stream)

    def materialize(self, stream: int):
        """y = act(x * scale[l] + shift[l]) as a stored tensor (the plain path; fused layers call it only for activation_pattern())."""
        x = self.x
        check(_lib.load().cp_affine_act_f32(x.data.data_ptr(), x.pixels, x.c, x.c, self.scale.data_ptr(), self.shift.data_ptr(), _ptr(self.labels), self.act,
                                            self.y.data.data_ptr(), x.c, stream), "cp_affine_act_f32(%s)" % self.name)

    def _backward_fused_head(self, stream: int):
        lib = _lib.load()
        x, p, hd = self.x, self.plan, self.head
        st_, off, ld = hd.dy_ptr_ld
        dout, readable = st_.data_ptr() + 4 * off, ld - off % ld
        args = (x.data.data_ptr(), x.c, dout, ld, min(32, readable), x.pixels, hd.layer.master.data_ptr(), hd.layer.cout, self.mean.data_ptr(),
                self.rstd.data_ptr(), self.gamma_full.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), _ptr(self.labels), self.classes, self.act)
        check(lib.cp_head1x1_bn_bwd_reduce_f32(*args, self.red.data_ptr(), self.chan.data_ptr(), stream), "cp_head1x1_bn_bwd_reduce_f32(%s)" % self.name)
        n = p.all_reduce_stats(self.chan, x.pixels)
        assert x.needs_grad and not x.has_grad
        check(lib.cp_head1x1_bn_bwd_apply_f32(*args, self.chan.data_ptr(), float(n), _ptr(self.row_scale), x.grad.data_ptr(), x.c, stream),
              "cp_head1x1_bn_bwd_apply_f32(%s)" % self.name)
        x.has_grad = True
        if self.dgamma_p is not None or self.dbeta_p is not None:
            check(lib.cp_bn_param_grads_f32(self.red.data_ptr(), x.c, self.real_c, self.classes, _ptr(self.dgamma_p), _ptr(self.dbeta_p), stream),
                  "cp_bn_param_grads_f32(%s)" % self.name)

    def backward(self, stream: int):
        if self.head is not None:
            return self._backward_fused_head(stream)
        lib = _lib.load()
        x, y, p = self.x, self.y, self.plan
        C_ = x.c
        if not y.needs_grad:
            return  # bn_data: its beta gradient comes from conv0's weight gradient (TrainPlan.backward)
        assert y.has_grad, "gradient of %s output not produced" % self.name
        gam, bet = self.gamma_full.data_ptr(), self.beta_full.data_ptr()
        check(lib.cp_bn_act_bwd_reduce_f32(x.data.data_ptr(), C_, y.grad.data_ptr(), C_, x.pixels, C_, self.classes, self.mean.data_ptr(),
                                           self.rstd.data_ptr(), gam, bet, _ptr(self.labels), self.act, self.scale.data_ptr(), self.shift.data_ptr(),
                                           self.red.data_ptr(), self.chan.data_ptr(), stream), "cp_bn_act_bwd_reduce_f32(%s)" % self.name)
        n = p.all_reduce_stats(self.chan, x.pixels)
        if x.needs_grad:
            check(lib.cp_bn_act_bwd_apply_f32(x.data.data_ptr(), C_, y.grad.data_ptr(), C_, x.pixels, C_, self.mean.data_ptr(), self.rstd.data_ptr(),
                                              gam, bet, _ptr(self.labels), self.act, self.scale.data_ptr(), self.shift.data_ptr(), self.chan.data_ptr(),
                                              float(n), _ptr(self.row_scale),
                                              x.grad.data_ptr(), C_, 1 if x.has_grad else 0, stream), "cp_bn_act_bwd_apply_f32(%s)" % self.name)
            x.has_grad = True
        if self.dgamma_p is not None or self.dbeta_p is not None:
            check(lib.cp_bn_param_grads_f32(self.red.data_ptr(), C_, self.real_c, self.classes, _ptr(self.dgamma_p), _ptr(self.dbeta_p), stream),
                  "cp_bn_param_grads_f32(%s)" % self.name)


class FnOp:
    def __init__(self, fwd, bwd, reads=()):
        self.forward, self.backward = fwd, bwd
        self.reads = tuple(reads)   # tensors the closure reads (TrainPlan._consumers)


def tape_readers(ops: Sequence, t: TT) -> List[int]:
    """tape indices of the ops that READ tensor t, one per read: convolution sources / residuals, normalisation inputs, the pooling / resampling closures"""
    def reads(op):
        if isinstance(op, ConvOp):
            return [s for s, _ in op.srcs] + [op.residual]
        return [op.x] if isinstance(op, BnActOp) else list(getattr(op, "reads", ()))

    return [i for i, op in enumerate(ops) for r in reads(op) if r is t]


# ------------------------------------------------------------------------------------------------
# plan
# ------------------------------------------------------------------------------------------------
class TrainPlan:
    """Buffers + tape for one (batch, H, W); `group` = torch.distributed process group for SyncBN / DP (or None)."""

    GRAD_LD = 64   # loss gradient rows: [0,32) logits (seg_dim real), [32,64) vertex (ver_dim real)
    VERT_OFF = 32

    def __init__(self, store: ParamStore, seg_dim: int, ver_dim: int, batch: int, h: int, w: int,
                 decoder_dims: Sequence[int] = DECODER_DIMS_DEFAULT, group=None, world_size: int = 1,
                 partial: Sequence[bool] = PARTIAL_DEFAULT, guided: Sequence[bool] = GUIDED_DEFAULT, bilinear: Sequence[bool] = BILINEAR_DEFAULT,
                 pvnet: bool = False, shared: Sequence[bool] = SHARED_DEFAULT, reuse_first: bool = False, skips2: bool = True, arch: Optional[Arch] = None):
        arch = arch or Arch(seg_dim, ver_dim, decoder_dims, partial, guided, bilinear, pvnet, shared, reuse_first, skips2)
        seg_dim, ver_dim, pvnet = arch.seg_dim, arch.ver_dim, arch.pvnet
        if h % 8 or w % 8:
            raise ValueError("input height/width must be multiples of 8 (got %dx%d)" % (h, w))
        if seg_dim > 32 or (ver_dim > 32 and not pvnet):
            raise ValueError("the training plan supports up to 32 classes / 32 vertex channels (more vertex channels only for `pvnet` with separated vector fields)")
        lib = _lib.load()
        self.store, self.seg_dim, self.ver_dim = store, seg_dim, ver_dim
        self.batch, self.h, self.w = batch, h, w
        self.arch, self.pvnet = arch, pvnet
        if self.pvnet:  # one merged head: its gradient row is the contiguous [seg | vertex] record
            if seg_dim + ver_dim > self.GRAD_LD:
                # `pvnet` with SEPARATED vector fields (one 2*kp slice per object, train_casapose.py:57,97-125): a wider gradient row; a multiple
                # of 32 so that the head's data gradient may read its channel-padded rows
                self.GRAD_LD = (seg_dim + ver_dim + 31) // 32 * 32
            self.VERT_OFF = seg_dim
        self.group, self.world_size = group, world_size
        self.monitor: Optional[SlotBuffer] = None   # range monitor (_arm_f16x2): slot i <-> self.ops[i], then the backward slots (self.bwd)
        self._f16x2_steps, self.f16x2_checks, self.f16x2_demoted, self._bwd_calibrated, self._dout_scale = 0, 0, [], False, 1.0
        # the data-parallel exchange of a step: which slice of the flat gradient goes out after which op is planned from the finished tape
        self.exchange = parallel.StepExchange(store.grad, group, world_size, lambda: parallel.gradient_buckets(
            store.offsets, store.size, [self._op_keys(op) for op in self.ops], forward_order(), BUCKET_STARTS), self._unscale_grads)
        self.update_moving = True
        dev = store.device
        f32 = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        B, K, V = batch, seg_dim, ver_dim
        self.out_ld = (K + V + 3) // 4 * 4   # row length of the output record, padded to 16 bytes (the LS voter stages rows as float4)
        hs = [h, h // 2, h // 4, h // 8]
        ws = [w, w // 2, w // 4, w // 8]
        self.ops: List = []
        self.convs: List[TrainConv] = []
        store.pack_reset()  # this plan's kernel layouts share one arena (one gather per weight refresh)

        def new(hh, ww, c, grad=True, name=""):
            return TT(torch.empty(B, hh, ww, c, **f32), grad, name)

        self.img4 = new(h, w, 4, False, "img4")        # raw image, channel 3 = 0 (decoder skip)
        self.x0 = new(h, w, 4, False, "bn_data")        # bn_data(image), channel 3 = 1 (see below)
        self.out = torch.zeros(B, h, w, self.out_ld, **f32)         # padded record
        self.out_view = self.out[..., :K + V]                       # what the model returns: concat(seg logits, vertex)
        self.dout = torch.zeros(B, h, w, self.GRAD_LD, **f32)
        self.labels = [torch.empty(B, hs[l], ws[l], **u8) for l in range(4)]
        self.pnorm = [torch.empty(B, hs[l], ws[l], **f32) for l in range(4)]
        self.sel = [torch.empty(B, hs[l], ws[l], **u8) for l in range(3)]
        self.sel_zero = [torch.zeros(B, hs[l], ws[l], **u8) for l in range(3)]  # plain nearest x2
        self.gmask = [torch.empty(B, hs[l], ws[l], **u8) if any(arch.bilinear) else None for l in range(3)]
        self.loss_sums = torch.zeros(3, dtype=torch.float64, device=dev)
        self.loss_ws = torch.empty(max(lib.cp_pose_loss_workspace_bytes(B, h, w), lib.cp_pose_loss_inst_workspace_bytes(B, h, w),
                                       lib.cp_pose_loss_sep_workspace_bytes(B, h, w, K)), **u8)
        self.object_loss_values = torch.zeros(B, K - 1, **f32)  # per-object proxy distances (proxy_voting_dist)
        # keypoint-reprojection loss (LS voter forward/backward)
        oc, kp = K - 1, 9
        self.est_labels = torch.empty(B, h, w, **u8)
        self.kp_counts = torch.zeros(2, B, K, dtype=torch.int32, device=dev)
        self.kp_conf_sums = torch.zeros(B, kp, dtype=torch.float64, device=dev)
        self.ls_sums = torch.zeros(B * oc * kp * 5, dtype=torch.float64, device=dev)
        self.ls_pu = torch.zeros(B * oc * kp * 4, **f32)
        self.ls_coords = torch.zeros(B, oc, kp, 2, **f32)
        self.ls_g = torch.zeros(B, oc, kp, 2, **f32)
        self.kp_loss_val = torch.zeros(1, dtype=torch.float64, device=dev)
        # what kp_loss_and_grad(device_loss=...) leaves: poses, cp_pnp_f64's info words and {solved, available but unsolved}; the running count of
        # unsolved pairs is kept by training.train_step
        self.bpnp_poses = self.bpnp_info = self.bpnp_counts = None
        self.bpnp_unsolved = 0
        self.device_bpnp = {}   # keypoint count -> DeviceBPnPLoss (training.device_bpnp_from_environment)

        def layer(rec, grad_sources):
            L = TrainConv(store, rec.key, rec.layout, rec.k, rec.cout, rec.sources, grad_sources)
            self.convs.append(L)
            return L

        def conv(L, rec, srcs, o: TT, in_h, in_w, **kw):
            op = ConvOp(L, srcs, (o.data, 0, o.c), B, in_h, in_w, stride=rec.stride, dilation=rec.dilation, pad=rec.pad, out=o, **kw)
            self.ops.append(op)
            return op

        def bn(norm, x, y, act, labels=None, row_scale=None, pad_one=False):
            gk = (norm.name + ".gamma") if norm.gamma else None
            self.ops.append(BnActOp(self, norm.name, x, y, act, gk, norm.name + ".beta", labels, K if norm.clade else 1, row_scale, pad_one))

        RELU, LEAKY, NONE = _lib.ACT_RELU, _lib.ACT_LEAKY01, _lib.ACT_NONE
        g = graph(arch)
        # ---- encoder --------------------------------------------------------------------------------
        # bn_data has no gamma; its padding channel is forced to the constant 1 so that conv0's weight gradient
        # for that (zero-weight) channel is G[t][o] = sum of dy over the positions where tap t is inside the image:
        # d beta_data[c] = sum_{t,o} W0[t,c,o] * G[t][o] without a 7x7 transposed convolution for three numbers.
        bn(g.bn_data, self.img4, self.x0, NONE, pad_one=True)
        self.bn_data_op = self.ops[-1]
        c0 = layer(g.conv0, [False])
        self.conv0 = c0
        x = new(hs[1], ws[1], 64)
        conv(c0, g.conv0, [(self.x0, 4)], x, h, w)
        x2s = new(hs[1], ws[1], 64, name="x2s")
        bn(g.bn0, x, x2s, RELU)
        pooled = new(hs[2], ws[2], 64, name="pool")

        pool_idx = torch.empty(B, hs[2], ws[2], 64, dtype=torch.uint8, device=dev)   # arg-max tap per pooled element: the adjoint routes by it

        def pool_f(stream, src=x2s, dst=pooled):
            check(lib.cp_maxpool3x3s2_idx_f32(src.data.data_ptr(), B, hs[1], ws[1], 64, dst.data.data_ptr(), pool_idx.data_ptr(), stream), "cp_maxpool3x3s2_idx_f32")

        def pool_b(stream, src=x2s, dst=pooled):
            assert dst.has_grad
            check(lib.cp_maxpool3x3s2_bwd_idx_f32(pool_idx.data_ptr(), dst.grad.data_ptr(), B, hs[1], ws[1], 64, src.grad.data_ptr(),
                                                  1 if src.has_grad else 0, stream), "cp_maxpool3x3s2_bwd_idx_f32")
            src.has_grad = True

        self.ops.append(FnOp(pool_f, pool_b, reads=[x2s]))
        xr, cur_h, cur_w = pooled, hs[2], ws[2]
        taps: Dict[str, TT] = {"x2s": x2s}
        tap = None   # the backbone output the next unit's bn1 materialises
        for u in g.units:
            oh, ow = (cur_h - 1) // u.conv1.stride + 1, (cur_w - 1) // u.conv1.stride + 1
            a = new(cur_h, cur_w, u.cin, name=u.base + "a")
            bn(u.bn1, xr, a, RELU)
            if tap:
                taps[tap] = a
            if u.sc is not None:
                sc = new(oh, ow, u.cout, name=u.base + "sc")
                sc_layer = layer(u.sc, [True])
                shortcut = sc
            else:
                shortcut = xr
            t = new(oh, ow, u.cout)
            conv(layer(u.conv1, [True]), u.conv1, [(a, u.cin)], t, cur_h, cur_w)
            if u.sc is not None:
                # the shortcut comes AFTER conv1 in the tape (both read `a`): the backward then runs its data gradient first, which lets the
                # GEMM route write `a.grad` plainly while conv1's data gradient, running after it, accumulates through its residual input
                conv(sc_layer, u.sc, [(a, u.cin)], sc, cur_h, cur_w)
            t2 = new(oh, ow, u.cout)
            bn(u.bn2, t, t2, RELU)
            xn = new(oh, ow, u.cout, name=u.base + "out")
            conv(layer(u.conv2, [True]), u.conv2, [(t2, u.cout)], xn, oh, ow, residual=shortcut)
            xr, cur_h, cur_w, tap = xn, oh, ow, u.tap
        x32s = new(cur_h, cur_w, 512, name="x32s")
        bn(g.bn1, xr, x32s, RELU)
        taps[tap] = x32s
        self.taps = taps
        skips = dict(taps, img4=self.img4)

        def upsample(prev: TT, l: int, kind: str) -> TT:
            """the previous block's output at level l as the record's upsample says (architecture.Block.upsample), materialised"""
            big = new(hs[l], ws[l], prev.c)
            sh, sw, c = hs[l] // 2, ws[l] // 2, prev.c
            selmap = self.sel[l] if kind == "guided" else self.sel_zero[l]   # plain nearest x2 = "guided" with neighbour 0 everywhere
            blend, guided = kind == "guided_bilinear", kind in ("guided", "nearest")

            def f(stream):
                x, y = prev.data.data_ptr(), big.data.data_ptr()
                if blend:
                    check(lib.cp_guided_bilinear_upsample_x2_f32(x, self.gmask[l].data_ptr(), B, sh, sw, c, y, stream), "cp_guided_bilinear_upsample_x2_f32")
                elif guided:
                    check(lib.cp_guided_upsample_x2_f32(x, selmap.data_ptr(), B, sh, sw, c, y, stream), "cp_guided_upsample_x2_f32")
                else:
                    check(lib.cp_upsample_bilinear_x2_f32(x, B, sh, sw, c, y, stream), "cp_upsample_bilinear_x2_f32")

            def b(stream):
                assert big.has_grad and not prev.has_grad
                dy, dx = big.grad.data_ptr(), prev.grad.data_ptr()
                if blend:
                    check(lib.cp_guided_bilinear_upsample_x2_bwd_f32(dy, c, self.gmask[l].data_ptr(), B, sh, sw, c, dx, stream), "cp_guided_bilinear_upsample_x2_bwd_f32")
                elif guided:
                    check(lib.cp_guided_upsample_x2_bwd_f32(dy, c, selmap.data_ptr(), B, sh, sw, c, dx, stream), "cp_guided_upsample_x2_bwd_f32")
                else:
                    check(lib.cp_upsample_bilinear_x2_bwd_f32(dy, c, B, sh, sw, c, dx, stream), "cp_upsample_bilinear_x2_bwd_f32")
                prev.has_grad = True

            self.ops.append(FnOp(f, b, reads=[prev]))
            return big

        def decoder(blocks):
            prev = None
            for i, blk in enumerate(blocks):
                c, l = blk.conv, blk.level
                labels = self.labels[l] if blk.norm.clade else None
                if c is None:  # casa_layer(y, "6", skip_conv=True): CLADE on block 1's raw convolution output
                    prev = new(hs[l], ws[l], blk.norm.channels)
                    bn(blk.norm, self._y_raw, prev, blk.act, labels)
                    continue
                if i == 0:
                    tts, gs = [(x32s, 512)], [True]
                else:   # the previous block's output, upsampled: bilinear (decoder 1), label-guided or plain nearest (decoder 2)
                    tts, gs = [(prev if blk.upsample == "none" else upsample(prev, l, blk.upsample), c.sources[0][0])], [True]
                    if blk.skip:
                        tts.append((skips[blk.skip], c.sources[1][0]))
                        gs.append(skips[blk.skip].needs_grad)
                L = layer(c, gs)
                raw = new(hs[l], ws[l], c.cout)
                act = new(hs[l], ws[l], c.cout)
                if blk.number == 1:
                    self._y_raw = raw
                pk = dict(tap_label=self.labels[l], row_scale=self.pnorm[l]) if c.partial else {}
                conv(L, c, tts, raw, hs[l], ws[l], **pk)
                bn(blk.norm, raw, act, blk.act, labels, pk.get("row_scale"))
                prev = act
            return prev

        def head(rec, feat, off, dy_off):
            self.ops.append(ConvOp(layer(rec, [True]), [(feat, rec.sources[0][0])], (self.out, off, self.out_ld), B, h, w, out=None,
                                   dy_ptr_ld=(self.dout, dy_off, self.GRAD_LD)))

        head(g.seg_head, decoder(g.decoder1), 0, 0)   # (PVNet: the one head, pose_models.py:645-696)
        self.cond_labels: Optional[torch.Tensor] = None  # ground-truth conditioning (train_vectors_with_ground_truth)
        if self.pvnet:
            self._finish_plan(f32)
            return

        def label_f(stream):
            if self.cond_labels is not None:
                self.labels[0].copy_(self.cond_labels)
            else:
                logits, ld_ = (self.seg_dense, K) if getattr(self, "seg_dense", None) is not None else (self.out, self.out_ld)
                check(lib.cp_argmax_labels(logits.data_ptr(), ld_, K, B * h * w, self.labels[0].data_ptr(), stream), "cp_argmax_labels")
            engine.label_pyramid(self.labels, self.pnorm, self.sel, self.gmask, B, h, w, stream)

        self.ops.append(FnOp(label_f, lambda stream: None))
        head(g.ver_head, decoder(g.decoder2), K, self.VERT_OFF)
        self._finish_plan(f32)

    def _finish_plan(self, f32):
        dev = self.store.device
        c0 = self.conv0
        self.store.pack_finalize()
        # two convolutions on one weight set: the op that runs LAST in the backward (first in the forward) adds to the master gradient
        seen = set()
        for op in reversed(self.ops):
            if isinstance(op, ConvOp):
                op.accumulate_master = op.layer.key in seen
                seen.add(op.layer.key)
        self.tensors = [o for o in self._all_tensors()]
        # fused training normalisation (CASAPOSE_FUSE_NORM=0 restores the separate passes everywhere)
        fuse = os.environ.get("CASAPOSE_FUSE_NORM", "1")
        if fuse not in ("0", "1"):
            raise ValueError("CASAPOSE_FUSE_NORM must be 1 (fused normalisation) or 0 (separate passes), got %r" % fuse)
        self.fuse_norm = fuse == "1"
        if self.fuse_norm:
            self._fuse_heads()
        for i, op in enumerate(self.ops):
            if isinstance(op, ConvOp):   # the backward runs the tape in reverse: a later reader of the source has written its gradient first
                op.setup_gemm(first_writer=max(tape_readers(self.ops, op.srcs[0][0])) == i)
        # Winograd for the deep 3x3 layers (forward and data gradient); shared scratch sized for the largest of them
        self.use_winograd = os.environ.get("CASAPOSE_NO_WINOGRAD", "0") != "1"
        self.wino_V = self.wino_M = None
        if self.use_winograd:
            sizes = [(op, op.setup_winograd()) for op in self.ops if isinstance(op, ConvOp)]
            nv = max([sz[0] for _, sz in sizes] + [0])
            nm = max([sz[1] for _, sz in sizes] + [0])
            if nv:
                self.wino_V = torch.empty(nv, **f32)
                self.wino_M = torch.empty(nm, **f32)
                for op, sz in sizes:
                    if sz[0]:
                        op.bind_winograd(self.wino_V, self.wino_M)
                if self.fuse_norm:
                    self._fuse_winograd()
        # gather map of conv0's packed weight-gradient entries that belong to the padding channel (c = 3)
        ramp = np.zeros((7, 7, 3, 64), np.int64)  # unused values; only the layout matters
        k0 = np.full((64, c0.ktot), -1, np.int64)
        for t in range(49):
            k0[:, t * 4 + 3] = np.arange(64) * c0.ktot + t * 4 + 3
        self.g_idx = torch.from_numpy(k0[:, [t * 4 + 3 for t in range(49)]].T.copy()).to(dev)  # [49 taps][64 cout] -> flat index into dwp
        del ramp
        # the backward GEMMs on fp16 pairs (train_bwd_f16x2), one slot each behind the forward's: Winograd data / weight gradients, direct 3x3 layers
        slots = []
        for op in (op for op in self.ops if isinstance(op, ConvOp)):
            r = op.routes   # resolved here, once: every record the kernel families depend on stands by now
            slots += [w.slot for w in list(op.wino_dgrad.values()) + [op.wino_fwd] if w is not None and w.slot is not None]
            if op.layer.mode_planes == 3 and train_bwd_f16x2() and ("split" in r.dgrad or r.wgrad == "direct_split"):
                op.bw16 = BwdSlot("direct", op)
                slots.append(op.bw16)
        for j, r in enumerate(slots):
            r.slot = len(self.ops) + j
        self.bwd = BackwardRange(slots, torch.zeros(2, dtype=torch.int32).pin_memory())

    loss_exp = property(lambda self: self.bwd.loss_exp)   # (f16x2_range.BackwardRange: the power of two on the loss, the drift moves, the skipped steps)
    f16x2_bwd_moves = property(lambda self: self.bwd.moves)
    f16x2_skipped_steps = property(lambda self: self.bwd.skipped_steps)
    _f16x2_mon = property(lambda self: self.monitor and self.monitor.dev)   # the slot words (int32 [4 * slots]) on the device

    def _consumers(self, t: TT) -> int:
        """ops that READ tensor t; taps are checked by the caller."""
        return len(tape_readers(self.ops, t))

    def _fuse_heads(self):
        """Blocks 5 / 10 -> head: the normalisation op directly before a streaming 1x1 head whose activated output nobody else reads hands its
        tables to the head (forward, weight gradient) and recomputes the head's data gradient in its own backward (csrc/head1x1.hip)."""
        for i, op in enumerate(self.ops):
            if not (isinstance(op, ConvOp) and op.head_fast and i > 0 and isinstance(self.ops[i - 1], BnActOp)):
                continue
            bn = self.ops[i - 1]
            y = op.srcs[0][0]
            if bn.y is not y or bn.x.c != 32 or bn.x.pixels % 32 or self._consumers(y) != 1 or any(t is y for t in self.taps.values()):
                continue
            if op.dy_ptr_ld is None or not bn.x.needs_grad or bn.classes > 64:
                continue
            st_, off, ld = op.dy_ptr_ld
            if ld % 4 or off % 4 or ld - off % ld < 32:
                continue
            bn.head, op.pre_bn = op, bn
        self._whole_records()

    def _whole_records(self):
        """Both fused heads write slices of the same [pixels][K + V] records, and a head that fills 36 or 108 bytes of every 144 leaves each
        128-byte line partly written: the memory system answers with a read-modify-write (556 us for the 9-column head into the records against
        209 us into dense rows, tools/debug/head_probe.py).  So the segmentation head writes DENSE rows of K logits (self.seg_dense; the arg-max
        reads those) and the vertex head, the last writer, copies them in front of its own columns: cp_head1x1_fwd_affine_record_f32 writes
        complete records.  CASAPOSE_HEAD_RECORDS=0 keeps the two slice writers."""
        self.seg_dense = None
        K, V = self.seg_dim, self.ver_dim
        heads = [op for op in self.ops if isinstance(op, ConvOp) and op.head_fast and op.pre_bn is not None]
        if os.environ.get("CASAPOSE_HEAD_RECORDS", "1") == "0" or len(heads) != 2 or K > 16 or K + V != self.out_ld:
            return
        seg, ver = heads
        if seg._out_ptr_ld != (self.out, 0, self.out_ld) or ver._out_ptr_ld != (self.out, K, self.out_ld) or seg.layer.cout != K or ver.layer.cout != V:
            return
        self.seg_dense = torch.zeros(self.out.shape[0] * self.out.shape[1] * self.out.shape[2], K, dtype=torch.float32, device=self.out.device)
        seg._out_ptr_ld = (self.seg_dense, 0, K)
        ver.record_prefix = (self.seg_dense, K, K)

    def _fuse_winograd(self):
        """Normalisation layers next to Winograd convolutions: the producer's output transform owns (tile, 4 channels) per lane and accumulates
        the batch statistics on its way out (no cp_bn_stats_f32 pass); a normalisation layer without labels whose activated output is read by ONE
        Winograd convolution only hands its tables to that convolution's input transform (no cp_affine_act_f32 pass, y never written -- the
        weight gradient of a Winograd layer multiplies the kept transformed input V, not y)."""
        convs = [op for op in self.ops if isinstance(op, ConvOp)]
        for bn in [op for op in self.ops if isinstance(op, BnActOp)]:
            if bn.head is not None or bn.pad_one:
                continue
            prod = [c for c in convs if c.out is bn.x and c.wino_fwd is not None and c.stats_to is None]
            if prod and bn.x.c == prod[0].layer.cout:
                prod[0].stats_to, bn.stats_from = bn, prod[0]
            if bn.classes != 1 or bn.labels is not None or any(t is bn.y for t in self.taps.values()) or self._consumers(bn.y) != 1:
                continue
            for c in convs:
                for i, (t, ld) in enumerate(c.srcs):
                    if t is bn.y and c.wino_fwd is not None and ld == bn.y.c and c.layer.sources[i][0] == bn.y.c:
                        c.pre_norm[i], bn.consumer = bn, c

    def _all_tensors(self):
        seen = {}
        for op in self.ops:
            for attr in ("x", "y", "out", "residual"):
                t = getattr(op, attr, None)
                if isinstance(t, TT):
                    seen[id(t)] = t
            for t, _ in getattr(op, "srcs", []):
                seen[id(t)] = t
        for t in self.taps.values():
            seen[id(t)] = t
        return list(seen.values())

    def activation_pattern(self) -> Dict[str, torch.Tensor]:
        """{normalisation layer name: bool tensor} -- the branch every ReLU / leaky pair took in the last forward (the sign of its output).
        The backward differentiates exactly this piecewise-linear function (cp_bn_act_bwd_* decide the branch with the forward's own
        expression); the gradient tests hand the pattern to the fp64 oracle so that elements sitting within rounding of a kink do not
        count as gradient error."""
        stream = torch.cuda.current_stream(self.store.device).cuda_stream
        for op in self.ops:
            if isinstance(op, BnActOp) and (op.head is not None or op.consumer is not None):
                op.materialize(stream)   # a fused layer never stored y: evaluate the forward's expression once for the pattern
        return {op.name: (op.y.data > 0).cpu() for op in self.ops if isinstance(op, BnActOp) and op.act != _lib.ACT_NONE}

    # ---- distributed hooks: the step's exchange, its log and its timing live in parallel.StepExchange ------------------
    @staticmethod
    def _op_keys(op) -> List[str]:
        """the parameter keys whose gradients are final once the backward has executed `op`"""
        return [op.layer.key] if isinstance(op, ConvOp) else ([k for k in (op.gamma_key, op.beta_key) if k] if isinstance(op, BnActOp) else [])

    def all_reduce_stats(self, table: torch.Tensor, local_pixels: int) -> int:
        """SUM the fp64 statistic table over the replicas; returns the global pixel count."""
        self.exchange.reduce_stats(table)
        return local_pixels * self.world_size

    @property
    def comm_log(self):
        return self.exchange.log

    @comm_log.setter
    def comm_log(self, log):
        self.exchange.log = log

    def start_comm_log(self):
        self.exchange.start_log()

    def comm_structure(self) -> dict:
        return self.exchange.structure()

    def start_comm_timing(self):
        self.exchange.start_timing()

    def comm_report(self) -> dict:
        return self.exchange.report()

    def all_reduce_grads(self):
        """Complete the gradient exchange started by backward() (or run it as one all-reduce if none is pending)."""
        self.exchange.wait()

    # ---- one step ------------------------------------------------------------------------------------
    def refresh_weights(self, stream: int):
        self.store.pack_refresh(stream)
        for L in self.convs:
            L.refresh(stream, hooks_only=True)

    def forward(self, img: torch.Tensor, cond_labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        lib = _lib.load()
        B, h, w = self.batch, self.h, self.w
        if tuple(img.shape) != (B, h, w, 3) or img.dtype != torch.float32 or not img.is_contiguous():
            raise ValueError("image must be a contiguous float32 [%d,%d,%d,3] tensor" % (B, h, w))
        stream = torch.cuda.current_stream(img.device).cuda_stream
        self.cond_labels = cond_labels
        check(lib.cp_pad_channels_3to4(img.data_ptr(), self.img4.data.data_ptr(), B * h * w, stream), "cp_pad_channels_3to4")
        self._poll_f16x2(stream)
        for op in self.ops:
            op.forward(stream)
        self._read_f16x2(img.device)
        return self.out_view

    # ---- range monitor of the fp16-pair forward and backward (round 6; the policy: f16x2_range.BackwardRange) -----------------------------
    def _bwd_slots(self):
        """[(op, record, entry "direct" / the wino_dgrad record / None for a Winograd weight gradient)]: the view bench.py reads"""
        return [(r.op, r, "direct" if r.kind == "direct" else r.entry) for r in self.bwd.slots]

    def _arm_f16x2(self):
        """one monitor slot per convolution op whose forward runs in the fp16 two-way split (slot i <-> self.ops[i]), then one per backward record"""
        self.monitor = SlotBuffer(len(self.ops) + len(self.bwd.slots), self.out.device)
        # the store outlives its plans (model.training_plan builds one per batch / size / group): every plan has its own host copy, and a flag
        # the previous plan's last step left in skip[0] must not skip this plan's first step (backward() clears or rewrites it every step)
        if self.store.skip is None:
            self.store.skip = torch.zeros(2, dtype=torch.int32, device=self.monitor.dev.device)
        else:
            self.store.skip[:1].zero_()
        for i, op in enumerate(self.ops):
            if isinstance(op, ConvOp):
                op.mon_ptr = self.monitor.ptr(i) if op.layer.fwd_f16x2 else None
        for r in self.bwd.slots:
            r.mon = self.monitor.ptr(r.slot)

    def _calibrate_bwd(self, stream: int):
        """after the plan's FIRST backward (exact split, slots armed): one synchronous reading gives every backward GEMM its exponent"""
        self._bwd_calibrated = True
        if self.monitor is None:
            return
        self.bwd.skip_base = int(self.store.skip[1])   # (synchronises anyway)
        if self.bwd.slots:
            words = self.monitor.read(len(self.ops))
            self.monitor.zero(len(self.ops))
            self.bwd.calibrate(words, stream)
            self._sync_guards()

    def _sync_guards(self):
        """write the guards into the backward slots (word [3]; clears their overflow bits)"""
        if self.bwd.slots:
            self.monitor.set_guards(self.bwd.guard_thresholds(), len(self.ops))

    def _collect_skip(self, multi: bool):
        """after an fp16-pair backward: store.skip[0] = MIN of the guard words over slots and ranks (a fired guard is negative), guards cleared"""
        col = self.monitor.dev.view(-1, 4)[len(self.ops):, 3]   # (the backward slots)
        torch.amin(col, dim=0, keepdim=True, out=self.store.skip[:1])
        col.bitwise_and_(0x7FFFFFFF)
        if multi:
            import torch.distributed as dist

            dist.all_reduce(self.store.skip[:1], op=dist.ReduceOp.MIN, group=self.group)

    def _read_f16x2(self, dev):
        """every F16X2_TRAIN_CHECK_EVERY-th step the slots (sticky maxima) go to pinned memory, judged at the start of a later step (_poll_f16x2)"""
        if self.monitor is not None:
            self._f16x2_steps += 1
            if self._f16x2_steps >= F16X2_TRAIN_CHECK_EVERY and self.monitor.event is None:
                self.monitor.read_async(torch.cuda.current_stream(dev), extra=(self.bwd.skip_host, self.store.skip))
                self._f16x2_steps = 0

    def _poll_f16x2(self, stream: int):
        if self.monitor is None:
            if any(isinstance(op, ConvOp) and op.layer.fwd_f16x2 for op in self.ops) or self.bwd.slots:
                self._arm_f16x2()
            return
        w = self.monitor.poll()
        if w is None:
            return
        lo, hi = engine.F16X2_AMAX_LO / engine.F16X2_MONITOR_SLACK, engine.F16X2_AMAX_HI * engine.F16X2_MONITOR_SLACK
        amax, n = decode(w)
        out = []
        for i, op in enumerate(self.ops):
            if not isinstance(op, ConvOp) or not op.layer.fwd_f16x2 or n[i] == 0:
                continue
            if _lib.load().cp_f16x2_range_check(amax[i], lo, hi, None) != 0:
                op.demote_forward_to_exact_split(stream)
                op.mon_ptr = None
                out.append("%s (max %.3g)" % (op.layer.name, amax[i]))
        demoted, moved = self.bwd.judge(w[len(self.ops):], stream)
        if moved:   # zero the backward slots' maxima (stream-ordered after the backward that reported with the old factors), then their guards
            self.monitor.zero(len(self.ops))
            self._sync_guards()
        out += demoted
        self._sync_guards()   # (a forward demoted above takes its Winograd weight gradient to the exact split: no guard)
        self.f16x2_checks += 1
        if self.bwd.count_skips(int(self.bwd.skip_host[1])):
            warnings.warn("training backward (fp16 two-way split): an operand left fp16's range and the optimizer step was skipped (%d step(s) "
                          "so far); the exponents are lowered from this reading on (TrainPlan.f16x2_skipped_steps)" % self.bwd.skipped_steps)
        if out:
            self.f16x2_demoted += out
            warnings.warn("training forward (fp16 two-way split): %d layer(s) converted operands outside [%g, %g] and run their forward on the exact bf16 split "
                          "from now on: %s" % (len(out), lo, hi, "; ".join(out)))

    def loss_and_grad(self, labels_ce: torch.Tensor, labels_fg: torch.Tensor, keypoints_yx: torch.Tensor, mask_w=1.0, vertex_w=1.0, proxy_w=1.0,
                      filter_with_segmentation=True, kp: int = 9, filter_high_proxy_errors: bool = False,
                      inst_counts: Optional[torch.Tensor] = None, inst_map: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Losses of compute_loss on the last forward's output and d loss / d output into self.dout. Returns fp64 [mask, vertex, proxy].
        keypoints_yx [B,oc,kp,2]: one keypoint set per object (cp_pose_loss_f32).  keypoints_yx [B,oc,I,kp,2] with inst_counts (int32 [B,oc],
        every entry in 0..I: the instances of the object present in the image) and optionally inst_map (uint8 [B,h,w], the instance that owns
        each pixel; without it a pixel follows the instance whose centre is nearest): several instances per object (cp_pose_loss_inst_f32)."""
        lib = _lib.load()
        B, h, w = self.batch, self.h, self.w
        stream = torch.cuda.current_stream(self.out.device).cuda_stream
        assert labels_ce.dtype == torch.uint8 and labels_fg.dtype == torch.uint8 and keypoints_yx.dtype == torch.float32
        # the power of two on the loss (train_bwd_f16x2): on the GRADIENT only -- the kernels' loss sums do not contain the weights
        self._dout_scale = S = 2.0 ** self.loss_exp
        mask_w, vertex_w, proxy_w = mask_w * S, vertex_w * S, proxy_w * S
        oc = self.seg_dim - 1
        if keypoints_yx.dim() == 5:
            return self._loss_and_grad_instances(labels_ce, labels_fg, keypoints_yx, mask_w, vertex_w, proxy_w, filter_with_segmentation, kp,
                                                 filter_high_proxy_errors, inst_counts, inst_map, stream)
        if inst_counts is not None or inst_map is not None:
            raise ValueError("inst_counts / inst_map go with keypoints_yx of shape (B, oc, I, kp, 2); got %s" % (tuple(keypoints_yx.shape),))
        assert tuple(keypoints_yx.shape) == (B, self.seg_dim - 1, kp, 2) and keypoints_yx.is_contiguous()
        if self.pvnet and oc > 1 and self.ver_dim == oc * 2 * kp:   # separated vector fields: per-object slices (compute_loss, train_casapose.py:57,97-125)
            if filter_high_proxy_errors:
                raise NotImplementedError("filter_high_proxy_errors with separated vector fields is not built")
            check(lib.cp_pose_loss_sep_f32(self.out.data_ptr(), self.out_ld, self.seg_dim, kp, labels_ce.data_ptr(), labels_fg.data_ptr(), keypoints_yx.data_ptr(),
                                           oc, B, h, w, 1 if filter_with_segmentation else 0, mask_w, vertex_w, proxy_w, self.loss_ws.data_ptr(),
                                           self.dout.data_ptr(), self.GRAD_LD, self.VERT_OFF, self.loss_sums.data_ptr(), stream), "cp_pose_loss_sep_f32")
            return self.loss_sums
        if 2 * kp > self.ver_dim:
            raise ValueError("the output holds %d vertex channels, fewer than 2 * %d keypoints" % (self.ver_dim, kp))
        check(lib.cp_pose_loss_f32(self.out.data_ptr(), self.out_ld, self.seg_dim, kp, labels_ce.data_ptr(), labels_fg.data_ptr(), keypoints_yx.data_ptr(),
                                   self.seg_dim - 1, B, h, w, 1 if filter_with_segmentation else 0, 1 if filter_high_proxy_errors else 0, mask_w, vertex_w,
                                   proxy_w, self.loss_ws.data_ptr(), self.dout.data_ptr(), self.GRAD_LD, self.VERT_OFF, self.loss_sums.data_ptr(),
                                   self.object_loss_values.data_ptr(), stream), "cp_pose_loss_f32")
        return self.loss_sums

    def _loss_and_grad_instances(self, labels_ce, labels_fg, keypoints_yx, mask_w, vertex_w, proxy_w, filter_with_segmentation, kp,
                                 filter_high_proxy_errors, inst_counts, inst_map, stream) -> torch.Tensor:
        """loss_and_grad's second form (the weights already carry the plan's 2^loss_exp)"""
        B, h, w, oc = self.batch, self.h, self.w, self.seg_dim - 1
        I = int(keypoints_yx.shape[2])
        if tuple(keypoints_yx.shape) != (B, oc, I, kp, 2) or not keypoints_yx.is_contiguous():
            raise ValueError("keypoints_yx must be contiguous (B, oc, I, kp, 2) = (%d, %d, I, %d, 2); got %s" % (B, oc, kp, tuple(keypoints_yx.shape)))
        if self.pvnet and oc > 1 and self.ver_dim == oc * 2 * kp:
            raise NotImplementedError("several instances per object with the separated vector fields of `pvnet` are not built")
        if 2 * kp > self.ver_dim:
            raise ValueError("the output holds %d vertex channels, fewer than 2 * %d keypoints" % (self.ver_dim, kp))
        if inst_counts is None:
            raise ValueError("keypoints_yx with an instance axis needs inst_counts (int32 [B, oc])")
        counts_host = inst_counts.detach().cpu() if isinstance(inst_counts, torch.Tensor) else torch.as_tensor(inst_counts)
        if tuple(counts_host.shape) != (B, oc) or counts_host.dtype != torch.int32:
            raise ValueError("inst_counts must be int32 (B, oc) = (%d, %d); got %s %s" % (B, oc, counts_host.dtype, tuple(counts_host.shape)))
        if int(counts_host.min()) < 0 or int(counts_host.max()) > I:      # the small array, on the host, before it is uploaded
            raise ValueError("inst_counts holds %d..%d; every count must be in 0..%d, the instances of keypoints_yx"
                             % (int(counts_host.min()), int(counts_host.max()), I))
        counts_dev = counts_host.to(self.out.device).contiguous() if not (isinstance(inst_counts, torch.Tensor) and inst_counts.is_cuda) else inst_counts.contiguous()
        if inst_map is not None and (inst_map.dtype != torch.uint8 or tuple(inst_map.shape) != (B, h, w) or not inst_map.is_contiguous()):
            raise ValueError("inst_map must be contiguous uint8 (B, h, w) = (%d, %d, %d); got %s %s" % (B, h, w, inst_map.dtype, tuple(inst_map.shape)))
        check(_lib.load().cp_pose_loss_inst_f32(self.out.data_ptr(), self.out_ld, self.seg_dim, kp, labels_ce.data_ptr(), labels_fg.data_ptr(),
                                                keypoints_yx.data_ptr(), oc, I, counts_dev.data_ptr(), inst_map.data_ptr() if inst_map is not None else None,
                                                B, h, w, 1 if filter_with_segmentation else 0, 1 if filter_high_proxy_errors else 0, mask_w, vertex_w,
                                                proxy_w, self.loss_ws.data_ptr(), self.dout.data_ptr(), self.GRAD_LD, self.VERT_OFF,
                                                self.loss_sums.data_ptr(), self.object_loss_values.data_ptr(), stream), "cp_pose_loss_inst_f32")
        return self.loss_sums

    def kp_loss_and_grad(self, labels_gt: torch.Tensor, gt_xy: torch.Tensor, affine: torch.Tensor, kp_w: float, max_pixel_error: float = 25.0,
                         min_num: int = 50, confidence_regularization: bool = False, vote_with_gt: bool = True, kp: int = 9,
                         min_num_gt: Optional[int] = None, filter_with_gt: bool = True, coords: Optional[torch.Tensor] = None,
                         backward: bool = True, host_loss: Optional[Callable] = None, device_loss=None) -> torch.Tensor:
        """keypoint_reprojection_loss (loss_functions.py:207-344, use_bpnp_reprojection_loss=False) on the last forward's
        output; ADDS kp_w * d loss / d output to self.dout (call after loss_and_grad).  gt_xy [B,oc,kp,2]: projected
        ground-truth keypoints in image pixels; affine [B,6]: crop->image map (crop_to_image_affine).  Returns the
        fp64 loss value (device scalar).  `coords` (optional, [B,oc,kp,2] (y,x)) replaces the internal vote (evaluation with the
        component-filtered voter; implies backward=False); min_num_gt / filter_with_gt as in loss_functions.py:221-222,246-252.
        `host_loss(coords, avail) -> (loss, g_yx)` replaces the reprojection kernel (the BPnP variant, whose PnP solve and
        implicit gradient run on the host like the reference's BPNP_fast).  `device_loss` (a pose_estimation.device_bpnp.DeviceBPnPLoss with
        its targets bound) computes the same variant on the device, straight into ls_g and kp_loss_val, without a host round trip; it leaves
        bpnp_poses [B,oc,1,3,4], bpnp_info [B,oc,4] and bpnp_counts [2] (solved, available but unsolved) as device tensors.  An available pair
        it cannot solve counts as unavailable there, where host_loss raises.  The two are mutually exclusive."""
        if host_loss is not None and device_loss is not None:
            raise ValueError("kp_loss_and_grad takes host_loss or device_loss, not both")
        lib = _lib.load()
        B, h, w, K = self.batch, self.h, self.w, self.seg_dim
        oc = K - 1
        out = self.out
        stream = torch.cuda.current_stream(out.device).cuda_stream
        conf_off = K + 2 * kp
        check(lib.cp_argmax_labels(out.data_ptr(), self.out_ld, K, B * h * w, self.est_labels.data_ptr(), stream), "cp_argmax_labels")
        check(lib.cp_kp_stats_f32(out.data_ptr(), self.out_ld, conf_off, labels_gt.data_ptr(), self.est_labels.data_ptr(), B, h, w, K, kp,
                                  self.kp_counts.data_ptr(), self.kp_conf_sums.data_ptr(), stream), "cp_kp_stats_f32")
        vote_labels = labels_gt if vote_with_gt else self.est_labels
        if coords is None:
            check(lib.cp_ls_vote_f32(out.data_ptr(), self.out_ld, 0, K, conf_off, vote_labels.data_ptr(), B, h, w, oc, kp, self.ls_sums.data_ptr(),
                                     self.ls_coords.data_ptr(), stream), "cp_ls_vote_f32")
        else:
            self.ls_coords.copy_(coords.reshape(B, oc, kp, 2))
            backward = False
        # objects_available (loss_functions.py:236-252): > min_num pixels in the estimated AND (filter_with_gt) the ground-truth mask
        avail = self.kp_counts[1, :, 1:] > min_num
        if filter_with_gt:
            avail = avail & (self.kp_counts[0, :, 1:] > (min_num if min_num_gt is None or min_num_gt < 0 else min_num_gt))
        avail = avail.to(torch.float32).contiguous()
        self.objects_available = avail
        if host_loss is not None:
            lv, g = host_loss(self.ls_coords, avail)
            self.ls_g.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).reshape(B, oc, kp, 2))
            self.kp_loss_val.fill_(float(lv))
        elif device_loss is not None:
            self.bpnp_poses, self.bpnp_info, self.bpnp_counts = device_loss.run(self.ls_coords, gt_xy, affine, avail, max_pixel_error, kp_w, self.ls_g,
                                                                                self.kp_loss_val)
        else:
            check(lib.cp_kp_reproj_loss_f32(self.ls_coords.data_ptr(), gt_xy.data_ptr(), affine.data_ptr(), avail.data_ptr(), B, oc, kp, max_pixel_error,
                                            kp_w, self.ls_g.data_ptr(), self.kp_loss_val.data_ptr(), stream), "cp_kp_reproj_loss_f32")
        loss = self.kp_loss_val[0]
        if self._dout_scale != 1.0:   # this term's gradient joins one that carries the loss factor
            self.ls_g.mul_(self._dout_scale)
        coef = None
        if confidence_regularization:
            cnt = self.kp_counts[0, :, 1:].sum(dim=1, keepdim=True).double()       # foreground pixels of the target mask
            safe = torch.where(cnt > 0, cnt, torch.ones_like(cnt))
            cl = torch.where(cnt > 0, self.kp_conf_sums / safe, torch.zeros_like(self.kp_conf_sums))
            loss = loss + torch.abs(cl - 0.7).mean()
            coef = (kp_w * self._dout_scale * torch.sign(cl - 0.7) / (B * kp) / safe * (cnt > 0)).to(torch.float32).contiguous()
        if backward:
            check(lib.cp_ls_vote_bwd_f32(out.data_ptr(), self.out_ld, K, conf_off, vote_labels.data_ptr(), B, h, w, oc, kp, self.ls_sums.data_ptr(),
                                         self.ls_g.data_ptr(), self.ls_pu.data_ptr(), labels_gt.data_ptr() if coef is not None else None, _ptr(coef),
                                         self.dout.data_ptr(), self.GRAD_LD, self.VERT_OFF, self.VERT_OFF + 2 * kp, 1, stream), "cp_ls_vote_bwd_f32")
        self._keep_coef = coef
        return loss

    def backward(self):
        """Back-propagate self.dout through the tape into store.grad.  With replicas, the SUM all-reduce of each gradient bucket is
        launched (asynchronously, on the collective library's stream) as soon as the backward has passed the bucket's first layer, so
        the exchange of the decoders' gradients overlaps the encoder's backward convolutions (self.exchange); all_reduce_grads() waits for them."""
        stream = torch.cuda.current_stream(self.out.device).cuda_stream
        for t in self.tensors:
            t.has_grad = False
        multi = self.exchange.begin_backward()
        # the direct data gradients' operand range: max |dY| by a reduction pass of its own, on the step before a reading of the slots only
        check_now = self.monitor is not None and (not self._bwd_calibrated or self._f16x2_steps >= F16X2_TRAIN_CHECK_EVERY - 1)
        for i in range(len(self.ops) - 1, -1, -1):
            op = self.ops[i]
            b = op.bw16 if check_now and isinstance(op, ConvOp) else None
            if b is not None and b.mon and not b.dead:
                dy_, ld_ = op._dy()
                check(_lib.load().cp_amax_f32(dy_, op.batch * op.out_h * op.out_w, ld_, op.layer.cout, b.mon, stream), "cp_amax_f32(dY %s)" % op.layer.name)
            op.backward(stream)
            self.exchange.after_op(i, stream)   # (the bucket holding bn_data.beta is completed below)
        if not self._bwd_calibrated:
            self._calibrate_bwd(stream)   # (this backward ran on the exact split)
            if self.store.skip is not None:
                self.store.skip[:1].zero_()
        elif self.bwd.slots and self.bwd.skip_base is not None:   # (armed and calibrated)
            self._collect_skip(multi)
        elif self.store.skip is not None:
            self.store.skip[:1].zero_()   # no fp16-pair backward in this step (calibrating, or a plan without one): nothing to skip
        # d beta of bn_data from the padding-channel entries of conv0's weight gradient (see __init__)
        G = self.conv0.dwp[self.g_idx.reshape(-1)].view(49, 64)            # [tap][cout]
        W0 = self.store.view("conv0.kernel").reshape(49, 3, 64)               # [tap][c][cout]
        dbeta = torch.einsum("tco,to->c", W0.double(), G.double())
        self.store.grad_view("bn_data.beta").copy_(dbeta)
        self.exchange.finish_backward(stream)
        # the loss carried a power of two (loss_exp): it leaves the flat gradient here -- bucket by bucket in front of each exchange above (the
        # buckets tile the buffer; every replica has its OWN factor, so it must be gone before replicas are summed), in one piece otherwise
        if not multi:
            self._unscale_grads(stream, 0, self.store.grad.numel())
        self._dout_scale = 1.0

    def _unscale_grads(self, stream: int, a: int, e: int):
        if self._dout_scale != 1.0 and e > a:
            g = self.store.grad[a:e]
            check(_lib.load().cp_axpby_f32(g.data_ptr(), 1.0 / self._dout_scale, g.data_ptr(), 0.0, e - a, g.data_ptr(), stream), "cp_axpby_f32(gradient / loss factor)")

    def train_step(self, img, labels_ce, labels_fg, keypoints_yx, lr: float, cond_labels=None, weights=(1.0, 1.0, 1.0),
                   filter_with_segmentation=True, kp_args: Optional[dict] = None):
        """One optimisation step.  kp_args (optional): keyword arguments of kp_loss_and_grad.  Returns the fp64 device
        vector [mask, vertex, proxy] (and, with kp_args, the keypoint loss as a second value)."""
        stream = torch.cuda.current_stream(img.device).cuda_stream
        self.exchange.begin_step()
        self.forward(img, cond_labels)
        sums = self.loss_and_grad(labels_ce, labels_fg, keypoints_yx, *weights, filter_with_segmentation=filter_with_segmentation)
        kp_loss = self.kp_loss_and_grad(**kp_args) if kp_args is not None else None
        self.backward()
        self.all_reduce_grads()
        self.store.adam_step(lr, stream)
        self.refresh_weights(stream)
        return sums if kp_loss is None else (sums, kp_loss)


def crop_to_image_affine(offsets: np.ndarray) -> np.ndarray:
    """[B,6] row-major 2x3 matrices mapping crop pixels (x,y) back to the original image, the composition applied by
    transform_points_back_tf_batch (ransac_voting.py:124-158) with the offsets layout used at its call site
    (loss_functions.py:276-285): [h_crop, w_crop, -, -, dx, dy, angle_deg, scale, sx, sy]."""
    o = np.asarray(offsets, np.float64)
    hc, wc, dx, dy, ang, sc, sx, sy = o[:, 0], o[:, 1], o[:, 4], o[:, 5], o[:, 6], o[:, 7], o[:, 8], o[:, 9]
    ar = -ang * (np.pi / 180.0)
    a, b = np.cos(ar), np.sin(ar)
    c = (1.0 - a) * sx / 2.0 - b * sy / 2.0
    d = b * sx / 2.0 + (1.0 - a) * sy / 2.0
    A = np.stack([a / sc, b / sc, a * (wc - dx) + b * (hc - dy) + c, -b / sc, a / sc, -b * (wc - dx) + a * (hc - dy) + d], axis=1)
    return A.astype(np.float32)


def project_keypoints(points_3d: np.ndarray, cam: np.ndarray, poses: np.ndarray) -> np.ndarray:
    """project_tf_batch (ransac_voting.py:185-194): points_3d [...,kp,3], cam [3,3], poses [...,3,4] -> [...,kp,2] (x,y)."""
    p = np.asarray(points_3d, np.float64)
    rt = np.asarray(poses, np.float64)
    camp = p @ np.swapaxes(rt[..., :3], -1, -2) + np.swapaxes(rt[..., 3:], -1, -2)
    pix = camp @ np.asarray(cam, np.float64).T
    z = pix[..., 2:]
    return np.where(z != 0, pix[..., :2] / np.where(z != 0, z, 1.0), 0.0).astype(np.float32)
