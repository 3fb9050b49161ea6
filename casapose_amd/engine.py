"""Host-side execution of the CASAPose forward on MI355X.

The arithmetic lives in libcasapose_hip.so (casapose_amd/csrc); this module only owns
device memory (PyTorch-ROCm tensors), folds the inference-mode normalisation layers into
per-channel / per-class affine tables, packs the Keras-layout kernels into the K order
the implicit-GEMM kernel expects, and issues the launches in graph order.

Graph followed: CASAPoseConditional5 (casapose/pose_models/models/pose_models.py:513-635)
over ResNet-18 with output stride 8 (models/resnet.py:183-328).  Layer / weight names are
the Keras names of the reference so weights map 1:1.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, check
from .architecture import (BILINEAR_DEFAULT, DECODER_DIMS_DEFAULT, GUIDED_DEFAULT, PARTIAL_DEFAULT, SHARED_DEFAULT, STAGE_DILATION,  # noqa: F401
                           STAGE_FILTERS, STAGE_STRIDE, Arch, graph)
from .f16x2_range import SlotBuffer, armed, decode

BN_EPS = 2e-5  # resnet.py:44; _normalization_layers.py:108

# Hard label maps the forward already computed (arg-max of its own logits), keyed by the storage
# address of the network output: the voting layer receives `torch.split` views of that output and
# can reuse the map instead of re-reading 708 MB of logits.  An entry owns a COPY of the map (the
# plan's own label buffer is overwritten by the next forward), holds a weak reference to the output
# tensor and remembers its version counter: an in-place edit of the output (views share the counter)
# or a dead / re-used storage is a miss, and the voter recomputes the arg-max from the logits.
import weakref

_LABEL_CACHE: Dict[int, Tuple["weakref.ReferenceType", torch.Tensor, int]] = {}


def _remember_labels(out: torch.Tensor, labels: torch.Tensor):
    """keep the label map of `out`; entries whose output tensor has died go first, then the oldest (round 6: a wholesale clear() above eight entries
    could drop the map of an output the caller still holds)"""
    for k in [k for k, (ref, _, _) in _LABEL_CACHE.items() if ref() is None]:
        _LABEL_CACHE.pop(k, None)
    while len(_LABEL_CACHE) >= 8:
        _LABEL_CACHE.pop(next(iter(_LABEL_CACHE)))
    _LABEL_CACHE[out.untyped_storage().data_ptr()] = (weakref.ref(out), labels, out._version)


def cached_labels(storage_ptr: int, shape: Tuple[int, int, int], version: Optional[int] = None) -> Optional[torch.Tensor]:
    hit = _LABEL_CACHE.get(storage_ptr)
    if hit is None:
        return None
    ref, labels, ver = hit
    if ref() is None or tuple(labels.shape) != tuple(shape) or (version is not None and version != ver) or ref()._version != ver:
        _LABEL_CACHE.pop(storage_ptr, None)
        return None
    return labels



def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def fold_bn(params: Dict[str, np.ndarray], name: str, pad_to: Optional[int] = None):
    """Inference-mode (Sync)BatchNormalization as y = x*scale + shift (fp64 fold, fp32 store)."""
    var = params[name + ".moving_variance"].astype(np.float64)
    mean = params[name + ".moving_mean"].astype(np.float64)
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    gamma = params.get(name + ".gamma")
    beta = params.get(name + ".beta")
    scale = rstd if gamma is None else gamma.astype(np.float64) * rstd
    shift = -mean * scale
    if beta is not None:
        shift = shift + beta.astype(np.float64)
    if pad_to is not None and pad_to > scale.size:
        scale = np.concatenate([scale, np.zeros(pad_to - scale.size)])
        shift = np.concatenate([shift, np.zeros(pad_to - shift.size)])
    return scale.astype(np.float32), shift.astype(np.float32)


def fold_clade(params: Dict[str, np.ndarray], name: str):
    """ClassAdaptiveWeightedNormalization with a hard label (one-hot mask):
    y = gamma[l]*(x-mean)*rstd + beta[l]  ->  tables [classes][C]
    (_normalization_layers.py:119-139)."""
    var = params[name + ".moving_variance"].astype(np.float64)
    mean = params[name + ".moving_mean"].astype(np.float64)
    rstd = 1.0 / np.sqrt(var + BN_EPS)
    gamma = params[name + ".gamma"].astype(np.float64)
    beta = params[name + ".beta"].astype(np.float64)
    scale = gamma * rstd[None, :]
    shift = beta - gamma * (mean * rstd)[None, :]
    return scale.astype(np.float32), shift.astype(np.float32)


def label_pyramid(labels: Sequence[torch.Tensor], pnorm: Sequence[torch.Tensor], sel: Sequence[torch.Tensor], gmask: Sequence[Optional[torch.Tensor]],
                  batch: int, h: int, w: int, stream: int):
    """From the hard label map labels[0]: the label pyramid labels[1..3], the partial convolutions' row scales pnorm[0..3], the guided
    upsampling's neighbour maps sel[0..2] and -- where allocated -- the GuidedBilinearUpsampling match masks gmask[0..2] (pose_models.py:547-559)."""
    lib = _lib.load()
    lab = (C.c_void_p * 4)(*[t.data_ptr() for t in labels])
    pn = (C.c_void_p * 4)(*[t.data_ptr() for t in pnorm])
    sl = (C.c_void_p * 3)(*[t.data_ptr() for t in sel])
    check(lib.cp_label_pyramid(labels[0].data_ptr(), batch, h, w, lab, pn, sl, stream), "cp_label_pyramid")
    for l in range(3):
        if gmask[l] is not None:
            check(lib.cp_guided_match_mask(labels[l].data_ptr(), labels[l + 1].data_ptr(), batch, h >> l, w >> l, gmask[l].data_ptr(), stream),
                  "cp_guided_match_mask")


class FusedConv:
    """One cp_conv2d_fwd_f32 launch with its packed weights and descriptor."""

    def __init__(self, name: str, kernel: np.ndarray, layout: int, kh: int, kw: int, cout: int,
                 sources: Sequence[Tuple[int, int]], device: torch.device, want_split: bool = True):
        lib = _lib.load()
        self.name = name
        self.kh, self.kw, self.cout = kh, kw, cout
        self.sources = list(sources)
        ns = len(sources)
        chans = (C.c_int * 2)(*([s[0] for s in sources] + [0] * (2 - ns)))
        real = (C.c_int * 2)(*([s[1] for s in sources] + [0] * (2 - ns)))
        self.ktot = lib.cp_conv_ktot(kh, kw, ns, chans)
        w = np.ascontiguousarray(kernel, dtype=np.float32)
        cin = sum(s[1] for s in sources)
        expect = (kh, kw, cin, cout) if layout == 0 else (cin, kh, kw, cout)
        if tuple(w.shape) != expect:
            raise ValueError("%s: kernel shape %s, expected %s" % (name, w.shape, expect))
        self.wp = None
        self.wp_stem_split_f32 = None
        self.stem_split = 0     # 3 / 1: this binding runs the stem on the bf16 matrix pipe (set by ForwardPlan)
        if all(s[0] == 4 or s[0] % 32 == 0 for s in sources):   # (16-multiple sources exist only for the bf16-pipe kernel below)
            packed = np.empty((cout, self.ktot), dtype=np.float32)
            check(lib.cp_conv_pack_weights_host(w.ctypes.data, layout, kh, kw, cout, ns, chans, real, packed.ctypes.data),
                  "cp_conv_pack_weights_host(%s)" % name)
            self.wp = torch.from_numpy(packed).to(device)
        # second packing for the LDS-resident halo-tile kernel (3x3, cout <= 64, 32-multiple sources [+ image])
        self.wp_halo = None
        halo_ok = kh == 3 and kw == 3 and cout <= 64 and sources[0][0] % 32 == 0 and (ns == 1 or sources[1][0] == 4 or sources[1][0] % 32 == 0)
        if halo_ok:
            nfl = lib.cp_conv_halo_weight_floats(cout, ns, chans)
            ph = np.empty(nfl, dtype=np.float32)
            check(lib.cp_conv_pack_weights_halo_host(w.ctypes.data, layout, cout, ns, chans, real, ph.ctypes.data),
                  "cp_conv_pack_weights_halo_host(%s)" % name)
            self.wp_halo = torch.from_numpy(ph).to(device)
        if kh == 7 and kw == 7 and cout == 64 and ns == 1 and sources[0][0] == 4:  # the ResNet stem: packing of csrc/conv_stem.hip (used at stride 2 / pad 3)
            ph = np.empty(25 * 2 * 64 * 4, dtype=np.float32)
            check(lib.cp_conv_pack_weights_stem_host(w.ctypes.data, layout, sources[0][1], ph.ctypes.data), "cp_conv_pack_weights_stem_host(%s)" % name)
            self.wp_halo = torch.from_numpy(ph).to(device)
            if want_split:   # the same layer on the bf16 matrix pipe (csrc/conv_stem_split.hip): fp32 image of its fragment stream
                ps = np.empty(lib.cp_conv_stem_split_weight_floats(), dtype=np.float32)
                check(lib.cp_conv_pack_weights_stem_split_host(w.ctypes.data, layout, sources[0][1], ps.ctypes.data), "cp_conv_pack_weights_stem_split_host(%s)" % name)
                self.wp_stem_split_f32 = torch.from_numpy(ps).to(device)
        # third packing: the fp32 image of the fragment stream of csrc/conv_hsplit.hip (3x3 / cout <= 512 in passes of 64 / 16-multiple sources [+ image]);
        # its bf16 planes (3 = exact split, 1 = plain bf16) are made on the device when a mode asks for them
        self.wp_split_f32 = None
        self._split_planes: Dict[int, torch.Tensor] = {}
        self._descale: Dict[int, float] = {}
        self.split_mode = 0
        split_ok = (kh == 3 and kw == 3 and cout <= 512 and cout % 4 == 0 and sources[0][0] % 16 == 0 and sources[0][0] != 4
                    and (ns == 1 or (sources[1][0] == 4 and cout <= 32) or sources[1][0] % 16 == 0))
        if split_ok and want_split:
            nfl = lib.cp_conv_split_weight_floats(cout, ns, chans)
            ps = np.empty(nfl, dtype=np.float32)
            check(lib.cp_conv_pack_weights_split_host(w.ctypes.data, layout, cout, ns, chans, real, ps.ctypes.data), "cp_conv_pack_weights_split_host(%s)" % name)
            self.wp_split_f32 = torch.from_numpy(ps).to(device)
        self.desc = ConvDesc()
        self._keep: List[torch.Tensor] = []
        self.head_w: Optional[torch.Tensor] = None
        self.head_cout = 0
        self._gemm: Optional[dict] = None   # set by enable_gemm_split() for the CURRENT binding only
        self.head_in_scale, self._head_tabs = 1.0, None   # f16x2 range guard: power of two on the fused head's operand (set_head_in_scale)
        self.deep_bf16 = False              # bf16 conv mode: this binding runs on csrc/conv_bf16d.hip (set by ForwardPlan)
        self.mon_ptr: Optional[int] = None  # f16x2 range monitor: device address of this layer's slot while a forward runs armed (ForwardPlan._run_armed)

    def _make_planes(self, key: int, image: torch.Tensor, planes: int, stream: Optional[int]) -> torch.Tensor:
        """2-byte operand planes of an fp32 fragment image: 3 = exact bf16 split, 1 = bf16, PLANES_F16X2 = the fp16 two-way split of image * 2^e (the
        inverse factor is kept in _descale[key]: the kernels multiply their accumulators by it)."""
        if key not in self._split_planes:
            lib = _lib.load()
            out = torch.empty(image.numel() // 512 * (planes & 15) * 1024, dtype=torch.uint8, device=image.device)
            st = torch.cuda.current_stream(out.device).cuda_stream if stream is None else stream
            scale = float(lib.cp_f16x2_weight_scale(float(image.abs().max()))) if planes == _lib.PLANES_F16X2 else 1.0
            check(lib.cp_conv_split_weights_scaled_f32(image.data_ptr(), image.numel(), planes, scale, out.data_ptr(), st), "cp_conv_split_weights_scaled_f32")
            self._split_planes[key] = out
            self._descale[key] = 1.0 / scale
        return self._split_planes[key]

    def split_weights(self, planes: int, stream: Optional[int] = None) -> torch.Tensor:
        """operand planes of the weights for cp_conv2d_fwd_split / cp_conv2d_fwd_stem_split (made once per mode)."""
        image = self.wp_split_f32 if self.wp_split_f32 is not None else self.wp_stem_split_f32
        return self._make_planes(planes, image, planes, stream)

    def head_split_weights(self, planes: int, stream: Optional[int] = None) -> torch.Tensor:
        return self._make_planes(-planes, self.head_w_split_f32, planes, stream)

    def attach_head(self, kernel_1x1: np.ndarray):
        """Fuse a following 1x1 convolution (HWIO [1,1,32,q], no bias / activation) into this layer's epilogue."""
        lib = _lib.load()
        w = np.ascontiguousarray(kernel_1x1, dtype=np.float32).reshape(32, -1)
        if self.cout != 32 or self.wp_halo is None or not (1 <= w.shape[1] <= 32):
            raise ValueError("%s: a fused head needs a 3x3 halo-kernel layer with 32 output channels" % self.name)
        packed = np.empty(1024, dtype=np.float32)
        check(lib.cp_conv_pack_head_weights_host(w.ctypes.data, w.shape[1], packed.ctypes.data), "cp_conv_pack_head_weights_host")
        self.head_w = torch.from_numpy(packed).to(self.wp_halo.device)
        self.head_cout = int(w.shape[1])
        ps = np.empty(1024, dtype=np.float32)   # the same head for the bf16-pipe kernel
        check(lib.cp_conv_pack_head_split_host(w.ctypes.data, w.shape[1], ps.ctypes.data), "cp_conv_pack_head_split_host")
        self.head_w_split_f32 = torch.from_numpy(ps).to(self.wp_halo.device)

    def bind(self, *, batch, in_h, in_w, stride=1, dilation=1, pad=0, srcs, tap_label=None, row_scale=None,
             residual=None, scale=None, shift=None, epi_label=None, act=0, out_raw=None, out_raw_ld=None,
             out_act=None, out_act_ld=None, tile_hint=0, head_out=None, head_out_ld=0, head_label_out=None, head_label_classes=0):
        """srcs: list of dicts(data=tensor, ld=int, mode=int, sel=tensor|None, pre=(scale,shift)|None)."""
        d = self.desc
        self._gemm = None   # a GEMM route decided for an earlier shape must not survive a re-bind (rows would be stale: out-of-bounds launch)
        self.deep_bf16 = False
        self.head_in_scale, self._head_tabs, self._epi_tabs = 1.0, None, (scale, shift)
        eh = (self.kh - 1) * dilation + 1
        ew = (self.kw - 1) * dilation + 1
        d.batch, d.in_h, d.in_w = batch, in_h, in_w
        d.out_h = (in_h + 2 * pad - eh) // stride + 1
        d.out_w = (in_w + 2 * pad - ew) // stride + 1
        d.cout, d.kh, d.kw = self.cout, self.kh, self.kw
        d.stride, d.dilation, d.pad = stride, dilation, pad
        d.num_sources = len(srcs)
        self._srcs = list(srcs)   # (ForwardPlan.f16x2_operand_ranges reads the source tensors back)
        keep = [self.wp] if self.wp is not None else []
        for i, s in enumerate(srcs):
            cs = d.src[i]
            cs.data = _ptr(s["data"])
            cs.channels = self.sources[i][0]
            cs.ld = s["ld"]
            cs.mode = s.get("mode", _lib.SRC_DIRECT)
            cs.sel = _ptr(s.get("sel"))
            pre = s.get("pre")
            cs.pre_scale = _ptr(pre[0]) if pre else None
            cs.pre_shift = _ptr(pre[1]) if pre else None
            keep += [s["data"], s.get("sel")] + (list(pre) if pre else [])
        d.weights = _ptr(self.wp)
        d.weights_halo = _ptr(self.wp_halo)
        d.tap_label = _ptr(tap_label)
        d.row_scale = _ptr(row_scale)
        d.residual = _ptr(residual)
        d.residual_ld = self.cout
        d.scale, d.shift = _ptr(scale), _ptr(shift)
        d.epi_label = _ptr(epi_label)
        d.act = act
        d.out_raw = _ptr(out_raw)
        d.out_raw_ld = out_raw_ld if out_raw_ld is not None else self.cout
        d.out_act = _ptr(out_act)
        d.out_act_ld = out_act_ld if out_act_ld is not None else self.cout
        # tile_hint TILE_SPLIT3 / TILE_BF16 / TILE_F16X2 (Python-side values): run on csrc/conv_hsplit.hip when the layer is in its range
        self.split_mode = 0
        if tile_hint in (_lib.TILE_SPLIT3, _lib.TILE_BF16, _lib.TILE_F16X2):
            if self.wp_split_f32 is None:
                raise _lib.CasaposeHipError("%s: the bf16-pipe kernel covers 3x3 / cout <= 512 / 16-multiple sources only" % self.name)
            self.split_mode = {_lib.TILE_SPLIT3: 3, _lib.TILE_BF16: 1, _lib.TILE_F16X2: _lib.PLANES_F16X2}[tile_hint]
            tile_hint = 0
        d.tile_hint = tile_hint
        d.head_weights = _ptr(self.head_w) if head_out is not None else None
        d.head_out = _ptr(head_out)
        d.head_cout = self.head_cout if head_out is not None else 0
        d.head_out_ld = head_out_ld
        d.head_label_out = _ptr(head_label_out) if head_out is not None else None
        d.head_label_classes = head_label_classes if head_label_out is not None else 0
        keep += [head_label_out, tap_label, row_scale, residual, scale, shift, epi_label, out_raw, out_act]
        self._keep = [k for k in keep if k is not None]
        return d.out_h, d.out_w

    def enable_gemm_split(self, kernel_hwio: np.ndarray, planes: int) -> bool:
        """1x1 / stride 1 / one source / plain output: the layer is a GEMM rows x cin x cout, which the bf16-pipe GEMM of the Winograd path
        (csrc/wino_gemm_split.hip) computes as it is -- 3 planes exact split (fp32-equivalent), 2 planes hi + mid (the bf16 conv mode).
        Called by the forward plan in the opt-in conv modes after bind(); False when the descriptor is outside that shape."""
        d = self.desc
        rows = d.batch * d.out_h * d.out_w
        cin = self.sources[0][0]
        ok = (self.kh == 1 and self.kw == 1 and d.stride == 1 and d.pad == 0 and d.num_sources == 1 and d.src[0].mode == _lib.SRC_DIRECT
              and not d.src[0].pre_scale and d.src[0].ld == cin and self.sources[0][1] == cin and cin % 32 == 0 and rows % 128 == 0
              and d.out_raw and d.out_raw_ld == self.cout and not d.out_act and not d.scale and not d.residual and not d.row_scale
              and not d.tap_label and not d.head_out and d.act == 0)
        self._gemm = None
        if not ok:
            return False
        U = torch.from_numpy(np.ascontiguousarray(kernel_hwio.reshape(cin, self.cout).T[None])).to(torch.float32).to(self.wp.device if self.wp is not None else "cuda")
        if planes == _lib.PLANES_F16X2:
            Us, c_scale = split_wino_weights_f16x2(U, 1, self.cout, cin)
        else:
            Us, c_scale = split_wino_weights(U, 1, self.cout, cin), 1.0
        self._gemm = dict(Us=Us, rows=rows, k=cin, planes=planes, c_scale=c_scale)
        return True

    def set_head_in_scale(self, factor: float):
        """The fused 1x1 head of an f16x2 binding converts this layer's activated output t = act(v * scale + shift), which exists in registers only.
        Multiply the tables by a power of two: act(2^e x) = 2^e act(x) exactly for ReLU / leaky ReLU, so the head sees 2^e t and its accumulator
        factor (head_descale) takes 2^-e.  Only where nothing else receives t (no out_act) and a table exists."""
        d = self.desc
        scale, shift = self._epi_tabs
        if not d.head_out or d.out_act or scale is None or self.split_mode != _lib.PLANES_F16X2:
            raise _lib.CasaposeHipError("%s: no fused f16x2 head whose operand could be scaled" % self.name)
        self.head_in_scale = float(factor)
        self._head_tabs = (scale * factor, shift * factor)
        d.scale, d.shift = self._head_tabs[0].data_ptr(), self._head_tabs[1].data_ptr()

    def f16x2_active(self) -> bool:
        """does the CURRENT binding convert operands with the fp16 two-way split?"""
        return _lib.PLANES_F16X2 in (self.split_mode, self.stem_split, (self._gemm or {}).get("planes", 0))

    def demote_to_exact_split(self, kernel_hwio: Optional[np.ndarray] = None):
        """this binding's f16x2 launches on the exact three-way bf16 split instead (planes are made on first use)"""
        if self.split_mode == _lib.PLANES_F16X2:
            self.split_mode = 3
        if self.stem_split == _lib.PLANES_F16X2:
            self.stem_split = 3
        if self._gemm is not None and self._gemm["planes"] == _lib.PLANES_F16X2:
            if kernel_hwio is None or not self.enable_gemm_split(kernel_hwio, 3):
                raise _lib.CasaposeHipError("%s: cannot re-route the 1x1 GEMM to the exact split" % self.name)

    def run(self, stream: int):
        """One launch; while the plan runs armed (mon_ptr set) an f16x2 binding reports max |x| of what it converts into its monitor slot."""
        with armed(self.mon_ptr if self.mon_ptr and self.f16x2_active() else None):
            self._launch(stream)

    def _launch(self, stream: int):
        lib = _lib.load()
        g = self._gemm
        if g is not None:
            d = self.desc
            assert g["rows"] == d.batch * d.out_h * d.out_w, "%s: GEMM route bound for another shape" % self.name
            check(lib.cp_wino_gemm_split_scaled_f32(d.src[0].data, g["Us"].data_ptr(), d.out_raw, g["rows"], g["rows"], g["k"], self.cout, g["planes"], g["c_scale"],
                                                    stream), "cp_wino_gemm_split_scaled_f32(%s)" % self.name)
            return
        if self.deep_bf16:
            check(lib.cp_conv2d_fwd_bf16_deep(C.byref(self.desc), self.split_weights(1, stream).data_ptr(), stream), "cp_conv2d_fwd_bf16_deep(%s)" % self.name)
            return
        if self.stem_split:
            wsp = self.split_weights(self.stem_split, stream)
            check(lib.cp_conv2d_fwd_stem_split_scaled(C.byref(self.desc), wsp.data_ptr(), self.stem_split, self._descale[self.stem_split], stream),
                  "cp_conv2d_fwd_stem_split(%s)" % self.name)
            return
        if self.split_mode:
            if not lib.cp_conv_split_applicable(C.byref(self.desc)):
                raise _lib.CasaposeHipError("%s: descriptor outside the range of cp_conv2d_fwd_split" % self.name)
            head = self.head_split_weights(self.split_mode, stream).data_ptr() if self.desc.head_out else None
            wsp = self.split_weights(self.split_mode, stream)
            check(lib.cp_conv2d_fwd_split_scaled(C.byref(self.desc), wsp.data_ptr(), head, self.split_mode, self._descale[self.split_mode],
                                                 self._descale[-self.split_mode] / self.head_in_scale if head else 1.0, stream), "cp_conv2d_fwd_split(%s)" % self.name)
            return
        check(lib.cp_conv2d_fwd_f32(C.byref(self.desc), stream), "cp_conv2d_fwd_f32(%s)" % self.name)

    @property
    def flops(self) -> float:
        d = self.desc
        cin = sum(s[1] for s in self.sources)
        head = 2.0 * d.batch * d.out_h * d.out_w * 32 * d.head_cout if d.head_out else 0.0
        return 2.0 * d.batch * d.out_h * d.out_w * self.kh * self.kw * cin * self.cout + head


# The Winograd GEMM as exact 3-way bf16 splits on the bf16 matrix pipe (fp32-EQUIVALENT: every product exact, fp32 accumulation, measured
# error <= the fp32 MFMA's; csrc/wino_gemm_split.hip).  Round 3: the DEFAULT of both plans -- the training plan since round 2, the
# inference plan whenever its conv mode is "split" (its default, see CasaposeNet); CASAPOSE_WINO_GEMM=f32 restores the fp32 MFMA in both,
# CASAPOSE_WINO_GEMM=split forces the split GEMM even with conv_mode="f32".
WINO_GEMM_SPLIT = os.environ.get("CASAPOSE_WINO_GEMM", "") == "split"
WINO_GEMM_F32 = os.environ.get("CASAPOSE_WINO_GEMM", "") == "f32"
TRAIN_WINO_GEMM_SPLIT = os.environ.get("CASAPOSE_WINO_GEMM", "split") == "split"
# default arithmetic of the inference plan's convolutions (CasaposeNet(conv_mode=None)):
#   "f16x2" (default since round 4) = every fp32 operand as an fp16 pair hi + lo (reproduced to within one fp32 ulp), the three exact products hi*hi, hi*lo, lo*hi
#           accumulated in fp32 on the fp16 matrix pipe, for every layer the split kernels cover: fp32-LEVEL -- against fp64 its error is at or below
#           the fp32 MFMA's on the GEMM, on single convolutions and on the whole network (tests/test_gpu_f16x2.py) -- with half the MFMAs of "split";
#   "split" = exact three-way bf16 splits, six products (fp32-equivalent for any finite operand, no range conditions: the round-3 default);
#   "f32"   = the fp32 MFMA everywhere;   "bf16" = bf16 operands (3e-2 gates)
DEFAULT_INFER_CONV_MODE = "f16x2"
# The range condition of f16x2 (csrc/split_f16.h) is CHECKED, per layer, on the first forward of every plan (and again after set_params / load_weights,
# which drop the plans): a layer whose converted operands leave [F16X2_AMAX_LO, F16X2_AMAX_HI] gets an exact remedy -- a power of two on a Winograd layer's
# V or on a fused head's operand, the exact three-way bf16 split for a direct layer (ForwardPlan._calibrate) -- with one warning naming the layers.  Below LO the low halves are fp16 subnormals (absolute 2^-25: worse than 2^-24 of the tensor's
# maximum); HI = 65504 / 4 leaves two octaves for later batches before a conversion clamps (and a clamp is graceful, split_f16.h: the maximum over a
# batch of 4800 tiles x 36 planes x K channels moves by tens of per cent between batches, not by factors).  CASAPOSE_F16X2_GUARD=0 / CasaposeNet(f16x2_guard=False)
# switch the check off (the unguarded plan of round 4: tests compare the two).
F16X2_GUARD = os.environ.get("CASAPOSE_F16X2_GUARD", "1") != "0"
F16X2_AMAX_LO = 0.5
F16X2_AMAX_HI = 65504.0 / 4.0
# Round 6: the measurements come from the converting kernels themselves (monitor slots behind the C ABI: cp_f16x2_monitor_set, include/casapose_hip.h) and
# the guard STAYS on after the calibration: EVERY forward of a guarded plan runs armed, so the slots are sticky maxima over everything the plan has
# converted since they were last read (measured cost, A/B in one call: 2149.5 -> 2141.5 images/s, 0.37 %; CASAPOSE_F16X2_MONITOR=0 arms the calibration
# passes only).  Every F16X2_MONITOR_EVERY-th forward the slots are copied to pinned host memory asynchronously, zeroed behind the copy, and judged at
# the start of a later forward -- no synchronisation on the hot path.  A layer whose converted maximum has left [LO / SLACK, HI * SLACK] (a later
# batch far above or below the one the plan was calibrated on) re-arms the calibration with one warning.  SLACK = 2 keeps HI * SLACK at half the
# fp16 maximum: nothing clamps before the monitor reacts.
F16X2_MONITOR = os.environ.get("CASAPOSE_F16X2_MONITOR", "1") != "0"
F16X2_MONITOR_EVERY = max(1, int(os.environ.get("CASAPOSE_F16X2_MONITOR_EVERY", "8")))
F16X2_MONITOR_SLACK = 2.0
# the last fused head writes whole output records (ForwardPlan._whole_records).  Opt-in: three one-call A/Bs on three boxes gave +0.7 %, -0.1 % and -0.2 %
# on the step (block 10's epilogue pays 0.05-0.06 ms for the copy; what comes back from the kernels that no longer share HBM with read-modify-writes
# depends on the box) -- not a gain one can rely on.  The training plan's heads, stand-alone streaming kernels, do write whole records by default.
WHOLE_RECORDS = os.environ.get("CASAPOSE_INFER_HEAD_RECORDS", "0") == "1"
BF16_DEEP = os.environ.get("CASAPOSE_BF16_DEEP", "1") != "0"   # bf16 conv mode: deep layers on csrc/conv_bf16d.hip (0: two-plane Winograd)
STEM_SPLIT = os.environ.get("CASAPOSE_STEM_SPLIT", "1") != "0"   # A/B switch: conv0 on csrc/conv_stem_split.hip in the split / bf16 conv modes


def split_wino_weights(U: torch.Tensor, groups: int, n: int, k: int, out: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """cp_wino_split_weights_f32: [groups][n][k] fp32 -> the fragment-major hi / mid / lo bf16 planes cp_wino_gemm_split_f32 reads."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(lib.cp_wino_split_weights_bytes(groups, n, k), dtype=torch.uint8, device=U.device)
    st = torch.cuda.current_stream(U.device).cuda_stream if stream is None else stream
    check(lib.cp_wino_split_weights_f32(U.data_ptr(), groups, n, k, out.data_ptr(), st), "cp_wino_split_weights_f32")
    return out


def split_wino_weights_f16x2(U: torch.Tensor, groups: int, n: int, k: int, stream: Optional[int] = None):
    """cp_wino_split_weights_scaled_f32 with CP_PLANES_F16X2: the fp16 two-way split of U * 2^e (e from max |U|: csrc/split_f16.h).  Returns the
    plane buffer and c_scale = 2^-e, the factor cp_wino_gemm_split_scaled_f32 multiplies its accumulators by."""
    lib = _lib.load()
    out = torch.empty(lib.cp_wino_split_weights_bytes(groups, n, k), dtype=torch.uint8, device=U.device)
    st = torch.cuda.current_stream(U.device).cuda_stream if stream is None else stream
    scale = float(lib.cp_f16x2_weight_scale(float(U.abs().max())))
    check(lib.cp_wino_split_weights_scaled_f32(U.data_ptr(), groups, n, k, _lib.PLANES_F16X2, scale, out.data_ptr(), st), "cp_wino_split_weights_scaled_f32")
    return out, 1.0 / scale


class WinoConv:
    """A deep 3x3 / stride-1 convolution executed as Winograd F(4x4,3x3): input transform(s), ONE grouped 1x1 launch over
    the 36 planes, output transform with the fused epilogue (csrc/wino.hip).  Same interface as FusedConv.run()."""

    def __init__(self, name: str, kernel_hwio: np.ndarray, cout: int, sources: Sequence[Tuple[int, int]], device: torch.device,
                 split_planes: Optional[int] = None):
        lib = _lib.load()
        self.name, self.cout, self.sources = name, cout, list(sources)
        self.kh = self.kw = 3
        self.ktot = sum(s[0] for s in sources)
        if self.ktot % 32 or cout % 4:
            raise ValueError("%s: Winograd path needs 32-multiple input channels and 4-multiple output channels" % name)
        w = np.ascontiguousarray(kernel_hwio, dtype=np.float32)
        cin = sum(s[1] for s in sources)
        if tuple(w.shape) != (3, 3, cin, cout):
            raise ValueError("%s: kernel shape %s, expected %s" % (name, w.shape, (3, 3, cin, cout)))
        U = np.zeros((36, cout, self.ktot), np.float32)
        c0 = k0 = 0
        for cpad, creal in sources:
            check(lib.cp_wino_pack_weights_host(w.ctypes.data, cin, cout, c0, cpad, creal, self.ktot, k0, U.ctypes.data), "cp_wino_pack_weights_host(%s)" % name)
            c0 += creal
            k0 += cpad
        self.U = torch.from_numpy(U).to(device)
        # pre-split bf16 planes of the opt-in GEMM; split_planes = 2 (the bf16 conv mode): hi + mid planes only, three products, NOT fp32-equivalent
        self.planes = split_planes or 3
        self.c_scale = 1.0
        if self.planes == _lib.PLANES_F16X2:   # the fp16 two-way split: weights times a power of two, the GEMM undoes it
            self.Us, self.c_scale = split_wino_weights_f16x2(self.U, 36, cout, self.ktot)
        else:
            self.Us = split_wino_weights(self.U, 36, cout, self.ktot) if (WINO_GEMM_SPLIT or split_planes) else None
        self.desc = ConvDesc()  # the grouped GEMM
        self._keep: List = []
        self.v_scale, self._vs_vec, self._next_tabs = 1.0, None, None
        self.fuse_next, self.skip_input = None, False
        self.mon_ptr: Optional[int] = None   # f16x2 range monitor slot of THIS layer's V while a forward runs armed

    def demote_to_exact_split(self):
        """the fp16 two-way split of this layer's GEMM replaced by the exact three-way bf16 split (operands outside the fp16 range condition)"""
        if self.planes == _lib.PLANES_F16X2:
            self.Us, self.c_scale, self.planes = split_wino_weights(self.U, 36, self.cout, self.ktot), 1.0, 3

    @staticmethod
    def tiles(batch, h, w, dilation) -> Tuple[int, int]:
        t, tp = C.c_int(0), C.c_int(0)
        check(_lib.load().cp_wino_tiles(batch, h, w, dilation, C.byref(t), C.byref(tp)), "cp_wino_tiles")
        return t.value, tp.value

    def bind(self, *, batch, in_h, in_w, dilation, srcs, V, M, residual=None, scale=None, shift=None, epi_label=None, act=0,
             out_raw=None, out_act=None):
        """srcs: list of dicts(data=tensor, ld=int); V / M: scratch tensors of at least 36*Tp*ktot and 36*Tp*cout floats."""
        self.batch, self.h, self.w, self.dil = batch, in_h, in_w, dilation
        self.T, self.Tp = self.tiles(batch, in_h, in_w, dilation)
        if V.numel() < 36 * self.Tp * self.ktot or M.numel() < 36 * self.Tp * self.cout:
            raise ValueError("%s: Winograd scratch too small" % self.name)
        self.srcs, self.V, self.M = list(srcs), V, M
        self.v_scale, self._vs_vec, self._next_tabs = 1.0, None, None   # f16x2 range guard (ForwardPlan._calibrate): power of two applied to V
        self.epi = dict(residual=residual, scale=scale, shift=shift, epi_label=epi_label, act=act, out_raw=out_raw, out_act=out_act)
        d = self.desc
        d.batch, d.in_h, d.in_w, d.out_h, d.out_w = 36, 1, self.Tp, 1, self.Tp
        d.cout, d.kh, d.kw, d.stride, d.dilation, d.pad = self.cout, 1, 1, 1, 1, 0
        d.num_sources = 1
        d.src[0].data, d.src[0].channels, d.src[0].ld, d.src[0].mode = V.data_ptr(), self.ktot, self.ktot, _lib.SRC_DIRECT
        d.src[0].sel = d.src[0].pre_scale = d.src[0].pre_shift = None
        d.weights, d.weights_halo = self.U.data_ptr(), None
        d.tap_label = d.row_scale = d.residual = d.scale = d.shift = d.epi_label = None
        d.residual_ld, d.act = self.cout, 0
        d.out_raw, d.out_raw_ld, d.out_act, d.out_act_ld = M.data_ptr(), self.cout, None, self.cout
        d.tile_hint = 0
        d.head_weights = d.head_out = None
        d.head_label_out, d.head_label_classes = None, 0
        d.head_cout = d.head_out_ld = 0
        d.group_rows, d.group_weight_stride = self.Tp, self.cout * self.ktot
        self._keep = [V, M, residual, scale, shift, epi_label, out_raw, out_act] + [s["data"] for s in srcs]
        return in_h, in_w

    def _input_transform(self, src_ptr: int, ld: int, cpad: int, off: int, stream: int):
        """V[.., off : off + cpad] = B^T d B of one source; with v_scale != 1 through the transform's per-channel input affine (x * 2^e + 0: exact)"""
        with armed(self.mon_ptr if self.planes == _lib.PLANES_F16X2 else None):
            self._input_transform_launch(src_ptr, ld, cpad, off, stream)

    def _input_transform_launch(self, src_ptr: int, ld: int, cpad: int, off: int, stream: int):
        lib = _lib.load()
        if self.v_scale == 1.0:
            check(lib.cp_wino_input_transform_f32(src_ptr, ld, cpad, self.batch, self.h, self.w, self.dil, self.V.data_ptr(), self.ktot, off, stream),
                  "cp_wino_input_transform_f32(%s)" % self.name)
            return
        if self._vs_vec is None or self._vs_vec[0] != self.v_scale:
            n = max(c for c, _ in self.sources)
            self._vs_vec = (self.v_scale, torch.full((n,), self.v_scale, dtype=torch.float32, device=self.V.device), torch.zeros(n, dtype=torch.float32, device=self.V.device))
        check(lib.cp_wino_input_transform_pre_f32(src_ptr, ld, cpad, self.batch, self.h, self.w, self.dil, self.V.data_ptr(), self.ktot, off,
                                                  self._vs_vec[1].data_ptr(), self._vs_vec[2].data_ptr(), _lib.ACT_NONE, stream), "cp_wino_input_transform_pre_f32(%s)" % self.name)

    def _tables_for_next(self):
        """(scale, shift) pointers of this layer's epilogue when its fused output -> input transform writes the NEXT layer's V: the tables times the
        next layer's v_scale (ReLU / leaky ReLU commute with a positive factor, a power of two is exact) -- the activated map itself is not stored"""
        e, nxt = self.epi, self.fuse_next
        if nxt.v_scale == 1.0:
            return _ptr(e["scale"]), _ptr(e["shift"])
        if e["scale"] is None:
            raise _lib.CasaposeHipError("%s: cannot scale the fused transform's output without a normalisation table" % self.name)
        if self._next_tabs is None or self._next_tabs[0] != nxt.v_scale:
            self._next_tabs = (nxt.v_scale, e["scale"] * nxt.v_scale, e["shift"] * nxt.v_scale)
        return self._next_tabs[1].data_ptr(), self._next_tabs[2].data_ptr()

    def launches(self) -> List[Tuple[str, Callable[[int], None]]]:
        """The launches of run() in order, as (part, fn(stream)): "in" = the input transform of every source (absent when the producer's fused
        output -> input transform writes V), "gemm" = the grouped GEMM over the 36 planes, "out" = the output transform with the epilogue, or
        the fused output -> input transform into the next layer's V.  (tools/debug/wino_parts.py times the parts one by one.)"""
        parts = [] if self.skip_input else [("in", self._transform_inputs)]
        return parts + [("gemm", self.run_gemm), ("out", self._transform_output)]

    def run(self, stream: int):
        for _, launch in self.launches():
            launch(stream)

    def _transform_inputs(self, stream: int):
        off = 0
        for (cpad, _), s in zip(self.sources, self.srcs):
            self._input_transform(s["data"].data_ptr(), s["ld"], cpad, off, stream)
            off += cpad

    def run_gemm(self, stream: int):
        lib = _lib.load()
        if self.Us is not None:
            check(lib.cp_wino_gemm_split_scaled_f32(self.V.data_ptr(), self.Us.data_ptr(), self.M.data_ptr(), 36 * self.Tp, self.Tp, self.ktot, self.cout, self.planes,
                                                    self.c_scale / self.v_scale, stream), "cp_wino_gemm_split_scaled_f32(%s)" % self.name)
        else:
            check(lib.cp_wino_gemm_f32(self.V.data_ptr(), self.U.data_ptr(), self.M.data_ptr(), 36 * self.Tp, self.Tp, self.ktot, self.cout, stream),
                  "cp_wino_gemm_f32(%s)" % self.name)

    def _transform_output(self, stream: int):
        lib = _lib.load()
        e, nxt = self.epi, self.fuse_next
        if nxt is not None:   # Y = A^T M A + epilogue, then straight into the next layer's V (the activated map stays on chip)
            sc_, sh_ = self._tables_for_next()
            with armed(nxt.mon_ptr if nxt.planes == _lib.PLANES_F16X2 else None):   # it writes the NEXT layer's V
                check(lib.cp_wino_output_input_transform_f32(self.M.data_ptr(), self.cout, self.batch, self.h, self.w, self.dil, _ptr(e["residual"]), self.cout,
                                                             sc_, sh_, e["act"], _ptr(e["out_raw"]), self.cout, None, self.cout,
                                                             self.V.data_ptr(), nxt.ktot, 0, stream), "cp_wino_output_input_transform_f32(%s)" % self.name)
            return
        check(lib.cp_wino_output_transform_f32(self.M.data_ptr(), self.cout, self.batch, self.h, self.w, self.dil, _ptr(e["residual"]), self.cout,
                                               _ptr(e["scale"]), _ptr(e["shift"]), _ptr(e["epi_label"]), e["act"], _ptr(e["out_raw"]), self.cout,
                                               _ptr(e["out_act"]), self.cout, stream), "cp_wino_output_transform_f32(%s)" % self.name)

    @property
    def flops(self) -> float:
        """FLOPs of the convolution this launch group REPLACES (2*M*9*Cin*Cout), the figure the per-layer tables quote."""
        cin = sum(s[1] for s in self.sources)
        return 2.0 * self.batch * self.h * self.w * 9 * cin * self.cout

    @property
    def gemm_flops(self) -> float:
        """FLOPs the grouped GEMM actually executes (36 planes x padded tiles)."""
        return 2.0 * 36 * self.Tp * self.ktot * self.cout


WINO_DIRECT_UNDILATED_128 = os.environ.get("CASAPOSE_WINO_DIRECT_128", "")   # "" = by conv mode (f16x2: yes), "0" / "1" force (A/B)
WINO_MIN_K = int(os.environ.get("CASAPOSE_WINO_MIN_K", "0"))      # 0 = the measured defaults below
WINO_MIN_COUT = int(os.environ.get("CASAPOSE_WINO_MIN_COUT", "128"))


def wino_eligible(kh: int, stride: int, dilation: int, pad: int, sources: Sequence[Tuple[int, int]], cout: int, split_gemm: bool = False,
                  f16x2: bool = False) -> bool:
    """Measured on MI355X (profiles/): the 4x MFMA saving beats the two transform passes once the GEMM is deep and wide enough -- K >= 256 with
    the fp32-MFMA GEMM; K >= 128 when the GEMM runs on the bf16 pipe (split_gemm: the dilated 128 -> 256 layer stage3_unit1_conv1, which no
    split kernel covers directly, 0.43 -> 0.17 ms at bs 16; the three 128 -> 128 stage-2 layers 0.37 -> 0.36 ms).  f16x2 (three products per fp32
    product): the UNDILATED 128-channel layers are faster on the direct split kernel (stage 2: 0.27 against 0.30 ms, 1882 against 1872 images/s) --
    their Winograd GEMM is HBM-bound on V and M -- so K >= 256 again for them; the dilated 128 -> 256 layer has no direct kernel and stays."""
    k = sum(s[0] for s in sources)
    min_k = WINO_MIN_K or (128 if split_gemm else 256)
    direct_128 = f16x2 if WINO_DIRECT_UNDILATED_128 == "" else WINO_DIRECT_UNDILATED_128 == "1"
    if direct_128 and dilation == 1 and split_gemm and not WINO_MIN_K:
        min_k = 256
        # Round 6 (tools/debug/wino_parts.py, bs 16): decoder block 2 (384 -> 128, undilated) takes 88 + 87 + 25 us as input transform + GEMM + output
        # transform and 178 us on the direct f16x2 kernel (the same shape with a tap mask, block 7, runs there already): with <= 128 output channels
        # the GEMM's M traffic is small but V (2.25 x the 384-channel input in fp32) is not.  Undilated layers of that width go direct whatever K.
        if cout <= 128:
            return False
    return kh == 3 and stride == 1 and pad == dilation and k >= min_k and k % 32 == 0 and cout >= WINO_MIN_COUT and cout % 4 == 0


class ForwardPlan:
    """All buffers, descriptors and the launch order for one (batch, H, W) input shape."""

    def __init__(self, net: "CasaposeNet", batch: int, h: int, w: int, fuse_upsample: bool = True, fuse_heads: bool = True):
        if h % 8 or w % 8:
            raise ValueError("input height/width must be multiples of 8 (got %dx%d)" % (h, w))
        self.net, self.batch, self.h, self.w = net, batch, h, w
        self.fuse_upsample = fuse_upsample
        self.fuse_heads = fuse_heads and net.arch.decoder_dims[4] == 32 and not net.arch.pvnet
        dev = net.device
        f32 = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        B = batch
        K, V = net.seg_dim, net.ver_dim
        self.out_ld = K + V
        self.steps: List = []  # callables taking (stream)
        self.convs: List[FusedConv] = []
        # f16x2 range guard: the first run() of this plan goes layer by layer, measures what every f16x2 layer is about to convert and demotes the
        # layers outside the range condition to the exact split (ForwardPlan._calibrate); f16x2_report keeps what it saw
        self.needs_calibration = bool(net.conv_planes == _lib.PLANES_F16X2 and net.f16x2_guard)
        self.f16x2_report: Dict[str, Tuple[float, str]] = {}
        # ... and afterwards every forward runs armed; every F16X2_MONITOR_EVERY-th the slots are read back and judged without a synchronisation (_poll_monitor)
        self.monitor: Optional[SlotBuffer] = None   # slot i <-> self.convs[i] (_run_armed)
        self._since_monitor = 0
        self.monitor_checks = self.monitor_fired = 0   # armed forwards judged so far / how many of them re-armed the calibration
        lib = _lib.load()
        P = net.device_tables
        hs = [h, h // 2, h // 4, h // 8]
        ws = [w, w // 2, w // 4, w // 8]

        def new(*shape):
            return torch.empty(*shape, **f32)

        # ---- buffers that are (re)bound per call ------------------------------------------
        self.img4 = new(B, h, w, 4)
        self.labels = [torch.empty(B, hs[l], ws[l], **u8) for l in range(4)]
        self.labels_from_head = False   # True: block 5's fused segmentation head writes labels[0] in its epilogue
        self.pnorm = [new(B, hs[l], ws[l]) for l in range(4)]
        self.sel = [torch.empty(B, hs[l], ws[l], **u8) for l in range(3)]
        self.sel_zero = [torch.zeros(B, hs[l], ws[l], **u8) for l in range(3)]  # plain nearest x2 = "guided" with neighbour 0 everywhere
        self.gmask = [torch.empty(B, hs[l], ws[l], **u8) if any(net.arch.bilinear) else None for l in range(3)]  # GuidedBilinearUpsampling match masks
        self._out_bound: List[Tuple[FusedConv, int, str]] = []  # (conv, channel offset, descriptor field) writing into the per-call output
        self._bufs: List[torch.Tensor] = []

        self.wino_V = self.wino_M = None

        L, g = net.layers_by_name, net.graph

        def conv(rec, act_private: bool = False, **kw):
            """rec: the architecture.Conv record (its layer, stride, dilation and padding); act_private: nothing but the NEXT convolution of the
            plan reads this layer's activated output (lets two consecutive Winograd layers hand it over on chip: WinoConv.fuse_next)"""
            layer = L[rec.name]
            kw.update(stride=rec.stride, dilation=rec.dilation, pad=rec.pad)
            wl = net.wino_by_name.get(layer.name) if net.use_winograd else None
            plain = all(s.get("mode", _lib.SRC_DIRECT) == _lib.SRC_DIRECT and not s.get("pre") for s in kw["srcs"])
            # bf16 conv mode: the deep 3x3 layers (cout a multiple of 128, any of the dilations, no labels) on the direct bf16-operand kernel
            # (csrc/conv_bf16d.hip) instead of the two-plane Winograd path: measured 1.15-1.6x per layer at bs 16 (CASAPOSE_BF16_DEEP=0: Winograd)
            if (net.conv_planes == 1 and BF16_DEEP and layer.wp_split_f32 is not None and plain and layer.kh == 3 and layer.cout % 128 == 0
                    and kw.get("tap_label") is None and kw.get("epi_label") is None and kw.get("head_out") is None and kw.get("stride", 1) == 1):
                layer.bind(batch=B, **kw)
                if lib.cp_conv_bf16_deep_applicable(C.byref(layer.desc)):
                    layer.deep_bf16 = True
                    self.convs.append(layer)
                    self.steps.append(layer.run)
                    return
            if (wl is not None and plain and kw.get("tap_label") is None and kw.get("head_out") is None and kw.get("stride", 1) == 1
                    and kw.get("out_raw_ld") is None and kw.get("out_act_ld") is None and all(s["ld"] == c[0] for s, c in zip(kw["srcs"], wl.sources))):
                _, tp = WinoConv.tiles(B, kw["in_h"], kw["in_w"], kw.get("dilation", 1))
                nv, nm = 36 * tp * wl.ktot, 36 * tp * wl.cout
                if self.wino_V is None or self.wino_V.numel() < nv:
                    self.wino_V = torch.empty(nv, **f32)
                if self.wino_M is None or self.wino_M.numel() < nm:
                    self.wino_M = torch.empty(nm, **f32)
                self._wino_pending.append((wl, dict(batch=B, in_h=kw["in_h"], in_w=kw["in_w"], dilation=kw.get("dilation", 1), srcs=kw["srcs"],
                                                    residual=kw.get("residual"), scale=kw.get("scale"), shift=kw.get("shift"), epi_label=kw.get("epi_label"),
                                                    act=kw.get("act", 0), out_raw=kw.get("out_raw"), out_act=kw.get("out_act")), bool(act_private)))
                self.convs.append(wl)
                self.steps.append(wl.run)
                return
            layer.bind(batch=B, **kw)
            # conv mode (CASAPOSE_INFER_CONV_MODE / CasaposeNet(conv_mode=...), default "split"): the 3x3 / stride-1 layers off the Winograd path on the
            # bf16 matrix pipe (csrc/conv_hsplit.hip), 3 planes = exact three-way split (fp32-equivalent), 1 plane = bf16 operands; layers outside
            # its range (stem, strided and dilated layers, ...) keep the fp32-MFMA kernels
            layer.stem_split = 0
            planes = net.planes_for(layer.name)   # the net's conv mode, or the exact split for a layer the f16x2 guard has demoted
            if planes and layer.wp_split_f32 is not None and lib.cp_conv_split_applicable(C.byref(layer.desc)):
                layer.split_mode = planes
            elif (planes and STEM_SPLIT and layer.wp_stem_split_f32 is not None and kw.get("stride", 1) == 2 and kw.get("pad", 0) == 3
                  and kw.get("dilation", 1) == 1 and lib.cp_conv_selected_tile(C.byref(layer.desc)) == _lib.TILE_STEM):
                layer.stem_split = planes   # conv0 on the bf16 matrix pipe (exact split / bf16 operands), csrc/conv_stem_split.hip
            elif planes and layer.kh == 1 and layer.name + ".kernel" in net.params:
                layer.enable_gemm_split(np.asarray(net.params[layer.name + ".kernel"], np.float32), planes if planes in (3, _lib.PLANES_F16X2) else 2)
            self.convs.append(layer)
            self.steps.append(layer.run)

        self._wino_pending: List = []  # bound at the end, when the shared scratch has its final size

        # ---- encoder (resnet.py:246-305) ---------------------------------------------------
        x2s = new(B, hs[1], ws[1], 64)
        conv(g.conv0, in_h=h, in_w=w, srcs=[dict(data=self.img4, ld=4, pre=P[g.bn_data.name])],
             scale=P[g.bn0.name][0], shift=P[g.bn0.name][1], act=_lib.ACT_RELU, out_act=x2s)
        a = new(B, hs[2], ws[2], 64)
        s1, b1 = P[g.units[0].bn1.name]

        def pool(stream, src=x2s, dst=a, s1=s1, b1=b1):
            check(lib.cp_maxpool3x3s2_f32(src.data_ptr(), B, hs[1], ws[1], 64, s1.data_ptr(), b1.data_ptr(), 1,
                                          dst.data_ptr(), stream), "cp_maxpool3x3s2_f32")

        self.steps.append(pool)
        self._bufs += [x2s, a]
        cur_h, cur_w = hs[2], ws[2]
        x_raw = None
        taps: Dict[str, torch.Tensor] = {"x2s": x2s}
        for j, u in enumerate(g.units):
            oh, ow = (cur_h - 1) // u.conv1.stride + 1, (cur_w - 1) // u.conv1.stride + 1
            t = new(B, oh, ow, u.cout)
            bn2 = P[u.bn2.name]
            if u.sc is not None:
                sc = new(B, oh, ow, u.cout)
                conv(u.sc, in_h=cur_h, in_w=cur_w, srcs=[dict(data=a, ld=u.cin)], out_raw=sc)
                shortcut = sc
            else:
                shortcut = x_raw
            conv(u.conv1, in_h=cur_h, in_w=cur_w, act_private=True,   # t feeds conv2 only
                 srcs=[dict(data=a, ld=u.cin)], scale=bn2[0], shift=bn2[1], act=_lib.ACT_RELU, out_act=t)
            nxt = g.units[j + 1] if j + 1 < len(g.units) else None
            # a unit followed by one without a shortcut conv keeps its RAW sum (the next unit's shortcut), and its activated output feeds that
            # unit's conv1 only; the last unit of a stage also feeds the next stage's 1x1 shortcut / the decoders / the backbone's taps
            private = nxt is not None and nxt.sc is None
            x_raw = new(B, oh, ow, u.cout) if private else None
            nbn = P[nxt.bn1.name if nxt is not None else g.bn1.name]
            a_next = new(B, oh, ow, u.cout)
            conv(u.conv2, in_h=oh, in_w=ow, srcs=[dict(data=t, ld=u.cout)], act_private=private,
                 residual=shortcut, out_raw=x_raw, scale=nbn[0], shift=nbn[1], act=_lib.ACT_RELU, out_act=a_next)
            self._bufs += [t, shortcut, a_next]
            a, cur_h, cur_w = a_next, oh, ow
            if u.tap:
                taps[u.tap] = a
        self.taps = taps
        self.encoder_steps = len(self.steps)   # run_encoder() stops here: the bare ResNet-18 backbone (resnet.py:319: the model's five outputs)
        x32s, skips = taps["x32s"], dict(taps, img4=self.img4)

        def sources(i, blk, prev):
            """the block's input list: x32s for the first block, else the previous block's output as the record's upsample says (fused into
            the convolution's loaders, or materialised by a streaming pass first) + the skip tap"""
            if i == 0:
                return [dict(data=x32s, ld=512)]
            l, pc = blk.level, blk.conv.sources[0][0]
            src0, mode, sel = prev, _lib.SRC_DIRECT, None
            # bilinear: the convolution's loaders interpolate the x2 source from the half-resolution tile (staged in LDS by csrc/conv_hsplit.hip);
            # guided / nearest: they gather it by the label-guided neighbour map (nearest x2 = "guided" with neighbour 0 everywhere).
            # fuse_upsample=False materialises both in a separate streaming pass (the unfused reference), and GuidedBilinearUpsampling, a
            # 4-tap blend, is always materialised
            if fuse_upsample and blk.upsample == "bilinear":
                mode = _lib.SRC_BILINEAR_X2
            elif fuse_upsample and blk.upsample in ("guided", "nearest"):
                mode, sel = _lib.SRC_NEAREST_SEL, self.sel[l] if blk.upsample == "guided" else self.sel_zero[l]
            elif blk.upsample != "none":
                src0 = new(B, hs[l], ws[l], pc)
                self.steps.append(self._upsample_step(blk.upsample, prev, src0, l, pc))
                self._bufs.append(src0)
            srcs = [dict(data=src0, ld=pc, mode=mode, sel=sel)]
            if blk.skip:
                srcs.append(dict(data=skips[blk.skip], ld=blk.conv.sources[1][0]))
            return srcs

        # ---- decoder 1 (pose_models.py:541-546) -------------------------------------------
        self.out = None  # bound per call
        prev = None
        for i, blk in enumerate(g.decoder1):
            c, l = blk.conv, blk.level
            bn = P[blk.norm.name]
            o = new(B, hs[l], ws[l], c.cout)
            srcs = sources(i, blk, prev)
            if self.fuse_heads and i == 4:  # blocks 5 + pv_final_conv_segmentation in one launch; the 32-channel tensor is never stored
                L[c.name].attach_head(net.params[g.seg_head.key])
                # ... and the hard label map (arg-max of the K logits) straight from the head's registers: no pass over the strided records
                conv(c, in_h=hs[l], in_w=ws[l], srcs=srcs, scale=bn[0], shift=bn[1], act=blk.act,
                     head_out=self.img4, head_out_ld=self.out_ld, head_label_out=self.labels[0], head_label_classes=K)
                self._out_bound.append((L[c.name], 0, "head_out"))
                self.labels_from_head = True
            else:
                extra = {}
                if i == 0 and net.arch.reuse_first:
                    self.y_raw = new(B, hs[l], ws[l], c.cout)
                    extra = dict(out_raw=self.y_raw)
                conv(c, in_h=hs[l], in_w=ws[l], srcs=srcs, scale=bn[0], shift=bn[1], act=blk.act, out_act=o, **extra)
            self._bufs.append(o)
            prev = o
        self.fuse_head2 = False
        if not self.fuse_heads:   # (PVNet: one head for all K + ver_dim channels; no conditioning, no second decoder)
            conv(g.seg_head, in_h=h, in_w=w, srcs=[dict(data=prev, ld=g.seg_head.sources[0][0])], out_raw=self.img4, out_raw_ld=self.out_ld)
            self._out_bound.append((L[g.seg_head.name], 0, "out_raw"))
        self.seg_input_ptr = None  # set per call when the model has a data_segmentation input
        if net.arch.pvnet:
            self._bind_winograd()
            return

        # ---- hard label map + pyramid (pose_models.py:547-559) -----------------------------
        def label_step(stream):
            if self.seg_input_ptr is not None:
                src, ld = self.seg_input_ptr, K
            else:
                src, ld = self.out.data_ptr(), self.out_ld
            if self.seg_input_ptr is not None or not self.labels_from_head:   # else block 5's fused head has written labels[0] already
                check(lib.cp_argmax_labels(src, ld, K, B * h * w, self.labels[0].data_ptr(), stream), "cp_argmax_labels")
            label_pyramid(self.labels, self.pnorm, self.sel, self.gmask, B, h, w, stream)

        self.steps.append(label_step)

        # ---- decoder 2 (pose_models.py:561-616) -------------------------------------------
        prev = None
        for i, blk in enumerate(g.decoder2):
            c, l = blk.conv, blk.level
            tab = P[blk.norm.name]
            o = new(B, hs[l], ws[l], blk.norm.channels)
            if c is None:  # casa_layer(y, "6", skip_conv=True): CLADE + ReLU on block 1's raw convolution output
                def clade_step(stream, src=self.y_raw, dst=o, tab=tab, lab=self.labels[l], n=B * hs[l] * ws[l], c=blk.norm.channels, act=blk.act):
                    check(lib.cp_affine_act_f32(src.data_ptr(), n, c, c, tab[0].data_ptr(), tab[1].data_ptr(), lab.data_ptr(), act,
                                                dst.data_ptr(), c, stream), "cp_affine_act_f32(pv_block_6_clade)")

                self.steps.append(clade_step)
                self._bufs.append(o)
                prev = o
                continue
            srcs = sources(i, blk, prev)
            pk = dict(tap_label=self.labels[l], row_scale=self.pnorm[l]) if c.partial else {}
            # the fused head lives in the halo kernel, which gathers a guided/nearest x2 source only together with the tap mask
            fused = self.fuse_heads and i == 4 and (c.partial or not fuse_upsample or blk.upsample == "guided_bilinear")
            self.fuse_head2 = fused if i == 4 else False
            if fused:  # block 10 + pv_final_conv_vertex in one launch
                L[c.name].attach_head(net.params[g.ver_head.key])
                conv(c, in_h=hs[l], in_w=ws[l], srcs=srcs, scale=tab[0], shift=tab[1], epi_label=self.labels[l],
                     act=blk.act, head_out=self.img4, head_out_ld=self.out_ld, **pk)
                self._out_bound.append((L[c.name], K, "head_out"))
            else:
                conv(c, in_h=hs[l], in_w=ws[l], srcs=srcs, scale=tab[0], shift=tab[1], epi_label=self.labels[l],
                     act=blk.act, out_act=o, **pk)
            self._bufs.append(o)
            prev = o
        if not self.fuse_head2:
            conv(g.ver_head, in_h=h, in_w=w, srcs=[dict(data=prev, ld=g.ver_head.sources[0][0])], out_raw=self.img4, out_raw_ld=self.out_ld)
            self._out_bound.append((L[g.ver_head.name], K, "out_raw"))
        self._whole_records(L, K, B * h * w, new)
        self._bind_winograd()

    def _bind_winograd(self):
        lib = _lib.load()
        for wl, kw, _ in self._wino_pending:
            wl.bind(V=self.wino_V, M=self.wino_M, **kw)
            wl.fuse_next, wl.skip_input = None, False
        # consecutive Winograd layers A -> B of one geometry where B's only source is A's activated output and nothing else reads it: A's output
        # transform writes B's transformed input directly (cp_wino_output_input_transform_f32); the activated map is not stored
        for (a, ka, private), (b, kb, _) in zip(self._wino_pending, self._wino_pending[1:]):
            if not private:
                continue
            ia, ib = self.steps.index(a.run), self.steps.index(b.run)
            same = all(ka[k] == kb[k] for k in ("batch", "in_h", "in_w", "dilation"))
            if (ib == ia + 1 and same and len(kb["srcs"]) == 1 and kb["srcs"][0]["data"] is ka["out_act"] and ka["out_act"] is not None
                    and ka["epi_label"] is None and b.ktot == a.cout
                    and lib.cp_wino_output_input_applicable(ka["batch"], ka["in_h"], ka["in_w"], ka["dilation"], a.cout)):
                a.fuse_next, b.skip_input = b, True
        self._wino_pending = []

    # ---- f16x2 range guard (the C-ABI side: cp_f16x2_monitor_set / cp_f16x2_range_check / cp_amax_f32) -----------------------------
    _mon = property(lambda self: self.monitor and self.monitor.dev)            # the slot words (int32 [4 * convs]) on the device ...
    _mon_host = property(lambda self: self.monitor and self.monitor.host)      # ... and as the last reading left them in pinned memory

    def _run_armed(self, stream: int, fresh: bool = True):
        """One forward with every f16x2 layer reporting into its monitor slot (slot i <-> self.convs[i]; include/casapose_hip.h): the converting
        kernels fold max |x| of what they convert -- a direct layer's staged sources, the stem's image through its input affine, a 1x1 GEMM's rows,
        the planes V a Winograd transform writes, the activated map a fused head converts in registers -- into the slot with one atomic per wave.
        fresh = False keeps what earlier armed forwards left in the slots (the monitor's sticky maxima)."""
        if self.monitor is None:
            self.monitor = SlotBuffer(len(self.convs), self.net.device)
        elif fresh:
            self.monitor.zero()
        for i, c in enumerate(self.convs):
            c.mon_ptr = self.monitor.ptr(i)
        try:
            for step in self.steps:
                step(stream)
        finally:
            for c in self.convs:   # (never left attached: a layer run outside a plan's forward must not write into a plan's slots)
                c.mon_ptr = None

    def _judge(self, words: np.ndarray, lo: float, hi: float):
        """[(layer, "in" | "head", max |x| as converted, status, power of two)] for every slot that reported; status as cp_f16x2_range_check:
        0 inside [lo, hi], 1 rescale by the power of two, 2 no power of two helps (or not finite)"""
        lib = _lib.load()
        (ins, n), (heads, _) = decode(words), decode(words, 2)
        out = []
        for i, c in enumerate(self.convs):
            if n[i] == 0:
                continue
            for kind, amax in (("in", ins[i]), ("head", heads[i])):
                if kind == "head" and (amax == 0.0 or isinstance(c, WinoConv)):
                    continue
                r = C.c_float(1.0)
                st = lib.cp_f16x2_range_check(amax, lo, hi, C.byref(r))
                out.append((c, kind, amax, st, float(r.value)))
        return out

    def _producer_of(self, wl: "WinoConv") -> Optional["WinoConv"]:
        for c in self.convs:
            if isinstance(c, WinoConv) and c.fuse_next is wl:
                return c
        return None

    def _calibrate(self, stream: int):
        """Fit every f16x2 layer to what it converts: armed forwards (_run_armed), one host read per pass, exact remedies, repeated until a pass
        finds every layer inside [F16X2_AMAX_LO, F16X2_AMAX_HI] (a layer downstream of a clamping one is measured again once that one is fixed;
        the bench network settles in one pass, adversarial statistics in two or three).  Three places convert fp32 activations to fp16 pairs:
          * a Winograd layer's GEMM converts V = B^T d B (measured where it is written: the layer's own input transform or the producing layer's
            fused output -> input transform): the transform multiplies by a power of two (WinoConv.v_scale: exact) and the GEMM's accumulator
            factor undoes it -- the weights' remedy (cp_f16x2_weight_scale) applied to the activations;
          * a fused 1x1 head converts the activated 32-channel map that never reaches HBM (measured in the epilogue's registers): the normalisation
            table feeding the activation is multiplied by the power of two (ReLU / leaky ReLU are positively homogeneous: act(s x) = s act(x)
            exactly) and the head's accumulator factor undoes it (FusedConv.head_in_scale);
          * the direct kernels, the stem and the 1x1 GEMMs convert stored tensors that other layers read too: the layer runs on the exact
            three-way bf16 split (no range condition) -- for this plan and, through net.f16x2_fallback, for later plans (CasaposeNet.recalibrate()
            forgets that).
        The last pass IS the forward whose output run() returns.  Afterwards the monitor keeps watching (run(), _poll_monitor)."""
        net = self.net
        lo, hi = F16X2_AMAX_LO, F16X2_AMAX_HI
        changed: Dict[str, str] = {}

        def note(name: str, amax: float, what: str, action: str):
            self.f16x2_report[name] = (amax, action)
            if action != "f16x2":
                changed[name] = "%s (max |%s| = %.3g: %s)" % (name, what, amax, action)

        settled = False
        for _ in range(8):
            self._run_armed(stream)
            words = self.monitor.read()
            acted = False
            for c, kind, amax, st, r in self._judge(words, lo, hi):
                if isinstance(c, WinoConv):
                    a0 = amax / c.v_scale   # as the un-scaled transform would write it
                    prod = self._producer_of(c) if c.skip_input else None
                    can_scale = (not c.skip_input) or (prod is not None and prod.epi["scale"] is not None)
                    if st == 1 and can_scale:
                        c.v_scale *= r
                        acted = True
                    elif st != 0:
                        c.demote_to_exact_split()
                        c.v_scale = 1.0
                        acted = True
                    note(c.name, a0, "V", "exact bf16 split" if c.planes != _lib.PLANES_F16X2 else ("f16x2" if c.v_scale == 1.0 else "f16x2, V x %g" % c.v_scale))
                elif kind == "in":
                    if st != 0:
                        net.f16x2_fallback[c.name] = "max |a| = %.3g outside [%g, %g]" % (amax, lo, hi)
                        c.demote_to_exact_split(net.params.get(c.name + ".kernel"))
                        note(c.name, amax, "a", "exact bf16 split")
                        self.f16x2_report.pop(c.name + ":head", None)
                        acted = True
                    else:
                        note(c.name, amax, "a", "f16x2")
                elif c.name not in net.f16x2_fallback:   # the fused head's operand (a layer demoted in this very pass no longer converts it)
                    a0 = amax / c.head_in_scale
                    if st == 1:
                        c.set_head_in_scale(c.head_in_scale * r)
                        acted = True
                    elif st != 0:
                        net.f16x2_fallback[c.name] = "head operand max = %.3g" % a0
                        c.demote_to_exact_split(net.params.get(c.name + ".kernel"))
                        note(c.name, a0, "head a", "exact bf16 split")
                        acted = True
                        continue
                    note(c.name + ":head", a0, "head a", "f16x2" if c.head_in_scale == 1.0 else "f16x2, head input x %g" % c.head_in_scale)
            if not acted:
                settled = True
                break
        self.needs_calibration = False
        self._since_monitor, self.monitor.event = 0, None
        self.monitor.zero()   # the monitor's window starts behind the calibration (a sticky maximum of the calibration batch would hide a later, smaller regime)
        if not settled:
            warnings.warn("conv_mode f16x2: the range calibration did not settle in 8 passes; the plan keeps its last fit")
        if changed and not net._f16x2_warned:
            net._f16x2_warned = True
            warnings.warn("conv_mode f16x2: %d layer(s) outside the fp16 range condition [%g, %g] were rescaled by a power of two or moved to the exact bf16 split: %s"
                          % (len(changed), lo, hi, "; ".join(changed.values())))

    def _poll_monitor(self):
        """judge an armed forward whose slots have arrived in pinned host memory (never waits): a layer outside [LO / SLACK, HI * SLACK] -- a batch far
        from the one the plan was calibrated on -- re-arms the calibration, with a warning"""
        words = self.monitor.poll()
        if words is None:
            return
        lo, hi = F16X2_AMAX_LO / F16X2_MONITOR_SLACK, F16X2_AMAX_HI * F16X2_MONITOR_SLACK
        out = [(c.name + (":head" if kind == "head" else ""), amax) for c, kind, amax, st, _ in self._judge(words, lo, hi) if st != 0]
        self.monitor_checks += 1
        if out:
            self.monitor_fired += 1
            self.needs_calibration = True
            self.net._f16x2_warned = False
            warnings.warn("conv_mode f16x2: the range monitor found %d layer(s) converting operands outside [%g, %g] (%s): this batch is far from the one the "
                          "plan was calibrated on; calibrating again" % (len(out), lo, hi, "; ".join("%s max %.3g" % o for o in out[:6])))

    def recalibrate(self):
        """calibrate again on the next forward (keeps what net.f16x2_fallback has demoted: CasaposeNet.recalibrate() forgets that too)"""
        self.needs_calibration = bool(self.net.conv_planes == _lib.PLANES_F16X2 and self.net.f16x2_guard)

    def _device_amax(self, t: torch.Tensor) -> float:
        """max |t| through cp_amax_f32 (diagnostics; synchronises)"""
        slot = torch.zeros(4, dtype=torch.int32, device=t.device)
        check(_lib.load().cp_amax_f32(t.data_ptr(), 1, 0, t.numel(), slot.data_ptr(), torch.cuda.current_stream(t.device).cuda_stream), "cp_amax_f32")
        return float(slot[:1].cpu().numpy().view(np.float32)[0])

    def f16x2_operand_ranges(self) -> Dict[str, Optional[Tuple[float, float]]]:
        """The range condition of the fp16 two-way split made checkable.  Call after a forward: for every layer this plan runs in
        f16x2, (max |a| over the layer's source tensors, upper bound of the magnitude its split converts) -- the bound is max |a| itself for the
        direct kernels (an interpolated / selected source is a convex combination of the stored one; the stem's input affine is applied), 100 x
        max |a| for a Winograd layer (V = B^T d B: the rows of B^T sum to at most 10 in magnitude).  fp32-level accuracy needs the first number
        >= ~1 and the second <= 65504.  None: the layer's input exists only inside a fused output -> input transform (it is the activated,
        normalised output of the layer before it)."""
        out: Dict[str, Optional[Tuple[float, float]]] = {}
        for conv in self.convs:
            if hasattr(conv, "gemm_flops"):   # WinoConv
                if conv.planes != _lib.PLANES_F16X2:
                    continue
                if conv.skip_input:
                    out[conv.name] = None
                    continue
                amax = max(self._device_amax(s["data"]) for s in conv.srcs)
                out[conv.name] = (amax, 100.0 * amax)
                continue
            planes = conv.split_mode or conv.stem_split or ((conv._gemm or {}).get("planes", 0))
            if planes != _lib.PLANES_F16X2:
                continue
            amax = 0.0
            for sdict in conv._srcs:
                a = self._device_amax(sdict["data"])
                pre = sdict.get("pre")
                if pre:
                    a = a * self._device_amax(pre[0]) + self._device_amax(pre[1])
                amax = max(amax, a)
            out[conv.name] = (amax, amax)
        return out

    def _upsample_step(self, kind: str, src: torch.Tensor, dst: torch.Tensor, l: int, c: int):
        """a materialised x2 upsampling of src into dst (level l) -- kind as architecture.Block.upsample"""
        lib = _lib.load()
        B, sh, sw = self.batch, self.h >> (l + 1), self.w >> (l + 1)
        if kind == "bilinear":
            def step(stream):
                check(lib.cp_upsample_bilinear_x2_f32(src.data_ptr(), B, sh, sw, c, dst.data_ptr(), stream), "cp_upsample_bilinear_x2_f32")
        elif kind == "guided_bilinear":
            mask = self.gmask[l]

            def step(stream):
                check(lib.cp_guided_bilinear_upsample_x2_f32(src.data_ptr(), mask.data_ptr(), B, sh, sw, c, dst.data_ptr(), stream),
                      "cp_guided_bilinear_upsample_x2_f32")
        else:
            sel = self.sel[l] if kind == "guided" else self.sel_zero[l]

            def step(stream):
                check(lib.cp_guided_upsample_x2_f32(src.data_ptr(), sel.data_ptr(), B, sh, sw, c, dst.data_ptr(), stream), "cp_guided_upsample_x2_f32")
        return step

    def conv_flops(self) -> float:
        return sum(c.flops for c in self.convs)

    def run_encoder(self, img: torch.Tensor) -> List[torch.Tensor]:
        """The encoder alone: the five taps of the reference's backbone model in its output order (resnet.py:251-252,291,303-305,319) --
        relu0 [B,H/2,W/2,64], stage2_unit1_relu1 [B,H/4,W/4,64], stage3_unit1_relu1 [B,H/8,W/8,128], stage4_unit1_relu1 [B,H/8,W/8,256],
        relu1 [B,H/8,W/8,512].  The tensors are the plan's own buffers (valid until the next run)."""
        B, h, w = self.batch, self.h, self.w
        if tuple(img.shape) != (B, h, w, 3) or img.dtype != torch.float32 or not img.is_contiguous():
            raise ValueError("image must be a contiguous float32 [%d,%d,%d,3] tensor" % (B, h, w))
        stream = torch.cuda.current_stream(img.device).cuda_stream
        check(_lib.load().cp_pad_channels_3to4(img.data_ptr(), self.img4.data_ptr(), B * h * w, stream), "cp_pad_channels_3to4")
        for step in self.steps[:self.encoder_steps]:
            step(stream)
        return [self.taps[n] for n in ("x2s", "x4s", "x8s", "x16s", "x32s")]

    def _whole_records(self, L, K, pixels, new):
        """Both fused heads write slices of the same [pixels][K + V] output records -- 36 and 108 of every 144 bytes, in launches far apart -- and a
        partly written 128-byte line costs the memory system a read-modify-write (measured on the training heads: 2.2-2.7x the time of the same bytes
        as whole lines; tools/debug/head_probe.py).  So block 5's head writes DENSE rows of K logits (self.seg_dense) and block 10's, the last
        writer, copies them in front of its own columns (cp_conv_desc.head_prefix, the HS_PREFIX instantiations of csrc/conv_hsplit.hip): whole lines
        only.  Where it applies: both heads fused on the 2-byte-pipe kernel, block 10 a partial convolution, 8 <= K <= 12, K + V a multiple of 4.
        Opt-in (CASAPOSE_INFER_HEAD_RECORDS=1): see WHOLE_RECORDS."""
        self.seg_dense = None
        b5, b10 = L.get("pv_block_5_conv2d"), L.get("pv_block_10_prepare_conv2d")
        if (not WHOLE_RECORDS or not (self.labels_from_head and self.fuse_head2) or b5 is None or b10 is None or not (8 <= K <= 12) or self.out_ld % 4
                or b5.split_mode not in (3, _lib.PLANES_F16X2) or b10.split_mode not in (3, _lib.PLANES_F16X2) or not b10.desc.tap_label
                or b10.desc.head_cout + K != self.out_ld):
            return
        bound = {(id(l), f): o for l, o, f in self._out_bound}
        if bound.get((id(b5), "head_out")) != 0 or bound.get((id(b10), "head_out")) != K:
            return
        self.seg_dense = new(pixels, K)
        b5.desc.head_out, b5.desc.head_out_ld = self.seg_dense.data_ptr(), K
        b10.desc.head_prefix, b10.desc.head_prefix_n, b10.desc.head_prefix_ld = self.seg_dense.data_ptr(), K, K
        self._out_bound = [(l, o, f) for l, o, f in self._out_bound if not (l is b5 and f == "head_out") and not (l is b10 and f == "head_out")]
        self._out_bound.append((b10, 0, "head_out"))   # block 10 addresses the record itself

    def run(self, img: torch.Tensor, seg_input: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        lib = _lib.load()
        B, h, w = self.batch, self.h, self.w
        if tuple(img.shape) != (B, h, w, 3) or img.dtype != torch.float32 or not img.is_contiguous():
            raise ValueError("image must be a contiguous float32 [%d,%d,%d,3] tensor" % (B, h, w))
        stream = torch.cuda.current_stream(img.device).cuda_stream
        if out is None:
            out = torch.empty(B, h, w, self.out_ld, dtype=torch.float32, device=img.device)
        self.out = out
        for layer, off, field in self._out_bound:
            setattr(layer.desc, field, out.data_ptr() + 4 * off)
        if seg_input is not None:
            if tuple(seg_input.shape) != (B, h, w, self.net.seg_dim) or seg_input.dtype != torch.float32 or not seg_input.is_contiguous():
                raise ValueError("segmentation input must be a contiguous float32 [%d,%d,%d,%d] tensor" % (B, h, w, self.net.seg_dim))
            self.seg_input_ptr = seg_input.data_ptr()
        else:
            self.seg_input_ptr = None
        check(lib.cp_pad_channels_3to4(img.data_ptr(), self.img4.data_ptr(), B * h * w, stream), "cp_pad_channels_3to4")
        guard = self.net.conv_planes == _lib.PLANES_F16X2 and self.net.f16x2_guard
        if guard and not self.needs_calibration:
            self._poll_monitor()   # (may re-arm the calibration: a finished armed forward found a layer outside the band)
        if self.needs_calibration:
            self._calibrate(stream)
        elif guard and F16X2_MONITOR:
            self._run_armed(stream, fresh=False)   # sticky: the slots keep the maxima of every forward since they were last read
            self._since_monitor += 1
            if self._since_monitor >= F16X2_MONITOR_EVERY and self.monitor.event is None:
                self.monitor.read_async(torch.cuda.current_stream(img.device))   # judged at the start of a later forward, when the copy has landed
                self._since_monitor = 0
        else:
            for step in self.steps:
                step(stream)
            self._since_monitor += 1
        if self.net.arch.pvnet:
            _LABEL_CACHE.pop(out.untyped_storage().data_ptr(), None)
            return out
        if seg_input is None:  # labels[0] is the arg-max of THIS output's logits
            _remember_labels(out, self.labels[0].clone())
        else:
            _LABEL_CACHE.pop(out.untyped_storage().data_ptr(), None)
        return out


class CasaposeNet:
    """Parameters + launch plans of casapose_c_gcu5 on one GPU."""

    def __init__(self, params: Dict[str, np.ndarray], seg_dim: int, ver_dim: int, device: torch.device,
                 decoder_dims: Sequence[int] = DECODER_DIMS_DEFAULT, fuse_upsample: bool = True, fuse_heads: bool = True,
                 partial: Sequence[bool] = PARTIAL_DEFAULT, guided: Sequence[bool] = GUIDED_DEFAULT, use_winograd: bool = True,
                 bilinear: Sequence[bool] = BILINEAR_DEFAULT, pvnet: bool = False, shared: Sequence[bool] = SHARED_DEFAULT,
                 reuse_first: bool = False, skips2: bool = True, conv_mode: Optional[str] = None, f16x2_guard: Optional[bool] = None,
                 arch: Optional[Arch] = None):
        _lib.load()  # fail loudly if the HIP library is missing
        if device.type != "cuda":
            raise _lib.CasaposeHipError("casapose_amd runs on a ROCm GPU only (got device %s); there is no CPU fallback" % device)
        self.device = device
        self.arch = arch or Arch(seg_dim, ver_dim, decoder_dims, partial, guided, bilinear, pvnet, shared, reuse_first, skips2)
        self.graph = graph(self.arch)
        self.seg_dim, self.ver_dim = self.arch.seg_dim, self.arch.ver_dim
        self.fuse_upsample = fuse_upsample
        self.fuse_heads = fuse_heads
        self.use_winograd = use_winograd and os.environ.get("CASAPOSE_NO_WINOGRAD", "0") != "1"
        mode = conv_mode if conv_mode is not None else os.environ.get("CASAPOSE_INFER_CONV_MODE", DEFAULT_INFER_CONV_MODE)
        if mode not in ("f32", "split", "f16x2", "bf16"):
            raise ValueError("conv_mode must be f32, split, f16x2 or bf16 (got %r)" % mode)
        self.conv_mode = mode
        self.conv_planes = {"f32": 0, "split": 3, "f16x2": _lib.PLANES_F16X2, "bf16": 1}[mode]
        self.f16x2_guard = F16X2_GUARD if f16x2_guard is None else bool(f16x2_guard)
        self.f16x2_fallback: Dict[str, str] = {}   # layer -> why it left f16x2 (ForwardPlan._calibrate); reset by set_params
        self._f16x2_warned = False
        self.plans: Dict[Tuple[int, int, int], ForwardPlan] = {}
        self.set_params(params)

    def recalibrate(self):
        """Forget everything the f16x2 range guard has decided -- demoted layers (f16x2_fallback), powers of two on V and on the heads' operands -- and
        calibrate again on the next forward.  For a caller whose first batch was not representative (a blank warm-up image); the monitor does the
        incremental form of this by itself when a later batch leaves the band."""
        self.f16x2_fallback, self._f16x2_warned = {}, False
        self.plans.clear()

    def planes_for(self, layer_name: str) -> int:
        """operand planes of one layer: the conv mode's, or 3 (exact split) once the f16x2 guard has demoted the layer"""
        return 3 if (self.conv_planes == _lib.PLANES_F16X2 and layer_name in self.f16x2_fallback) else self.conv_planes

    def set_params(self, params: Dict[str, np.ndarray]):
        self.params = {k: np.asarray(v, dtype=np.float32) for k, v in params.items()}
        self.f16x2_fallback, self._f16x2_warned = {}, False   # new parameters: every plan calibrates again on its first forward
        dev = self.device
        p = self.params
        tabs: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

        def put(name, pair):
            tabs[name] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in pair)

        g = self.graph
        norms = [g.bn_data, g.bn0] + [n for u in g.units for n in (u.bn1, u.bn2)] + [g.bn1] + [b.norm for b in g.decoder1 + g.decoder2]
        for n in norms:
            put(n.name, fold_clade(p, n.name) if n.clade else fold_bn(p, n.name, pad_to=4 if n is g.bn_data else None))
        self.device_tables = tabs

        L: Dict[str, FusedConv] = {}
        Wn: Dict[str, WinoConv] = {}
        planes = 2 if self.conv_mode == "bf16" else (self.conv_planes if self.conv_mode in ("split", "f16x2") and not WINO_GEMM_F32 else None)
        convs = [g.conv0] + [c for u in g.units for c in (u.sc, u.conv1, u.conv2)] + [b.conv for b in g.decoder1 + g.decoder2] + [g.seg_head, g.ver_head]
        for c in convs:
            if c is None:
                continue
            w = p[c.key]
            L[c.name] = FusedConv(c.name, w, c.layout, c.k, c.k, c.cout, c.sources, dev, want_split=bool(self.conv_planes))
            if self.use_winograd and not c.partial and wino_eligible(c.k, c.stride, c.dilation, c.pad, c.sources, c.cout, split_gemm=bool(planes) or WINO_GEMM_SPLIT,
                                                                      f16x2=self.conv_mode == "f16x2"):
                Wn[c.name] = WinoConv(c.name, w if c.layout == 0 else np.transpose(w, (1, 2, 0, 3)), c.cout, c.sources, dev, split_planes=planes)
        self.layers_by_name = L
        self.wino_by_name = Wn
        self.plans.clear()

    def plan(self, batch: int, h: int, w: int) -> ForwardPlan:
        key = (batch, h, w)
        if key not in self.plans:
            # descriptors live inside the FusedConv objects, so one plan is active at a time
            self.plans.clear()
            self.plans[key] = ForwardPlan(self, batch, h, w, self.fuse_upsample, self.fuse_heads)
        return self.plans[key]

    def forward(self, img: torch.Tensor, seg_input: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        b, h, w, _ = img.shape
        return self.plan(b, h, w).run(img, seg_input, out)
