"""Functional wrappers over the C ABI (one call = one or two kernel launches).

Every function takes contiguous float32 / uint8 CUDA tensors in NHWC and returns new device
tensors.  They are thin: argument checking lives in the library (cp_last_error), and
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .engine import FusedConv


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.CasaposeHipError("casapose_amd ops need CUDA (ROCm) tensors; there is no CPU fallback")


def conv2d_fused(sources: Sequence[torch.Tensor], kernel: np.ndarray, *, layout: int = 0, stride: int = 1, dilation: int = 1,
                 pad: int = 0, modes: Optional[Sequence[int]] = None, sels: Optional[Sequence[Optional[torch.Tensor]]] = None,
                 pre: Optional[Sequence[Optional[Tuple[torch.Tensor, torch.Tensor]]]] = None, real_channels: Optional[Sequence[int]] = None,
                 in_hw: Optional[Tuple[int, int]] = None, tap_label=None, row_scale=None, residual=None, scale=None, shift=None,
                 epi_label=None, act: int = 0, want_raw: bool = True, want_act: bool = False, tile_hint: int = 0):
    """One fused convolution (see cp_conv2d_fwd_f32 in include/casapose_hip.h).
    `kernel` is the Keras-layout host array (HWIO, or IHWO when layout=1).  Returns
    (out_raw | None, out_act | None)."""
    _need_cuda(*sources)
    dev = sources[0].device
    b = sources[0].shape[0]
    modes = list(modes) if modes is not None else [0] * len(sources)
    sels = list(sels) if sels is not None else [None] * len(sources)
    pre = list(pre) if pre is not None else [None] * len(sources)
    chans = [s.shape[3] for s in sources]
    real = list(real_channels) if real_channels is not None else chans
    kh, kw = (kernel.shape[0], kernel.shape[1]) if layout == 0 else (kernel.shape[1], kernel.shape[2])
    cout = kernel.shape[3]
    if in_hw is None:
        h0, w0 = sources[0].shape[1], sources[0].shape[2]
        in_hw = (h0, w0) if modes[0] == 0 else (2 * h0, 2 * w0)
    layer = FusedConv("conv2d_fused", kernel, layout, kh, kw, cout, list(zip(chans, real)), dev)
    eh, ew = (kh - 1) * dilation + 1, (kw - 1) * dilation + 1
    oh = (in_hw[0] + 2 * pad - eh) // stride + 1
    ow = (in_hw[1] + 2 * pad - ew) // stride + 1
    out_raw = torch.empty(b, oh, ow, cout, dtype=torch.float32, device=dev) if want_raw else None
    out_act = torch.empty(b, oh, ow, cout, dtype=torch.float32, device=dev) if want_act else None
    srcs = [dict(data=s, ld=s.shape[3], mode=m, sel=sl, pre=p) for s, m, sl, p in zip(sources, modes, sels, pre)]
    layer.bind(batch=b, in_h=in_hw[0], in_w=in_hw[1], stride=stride, dilation=dilation, pad=pad, srcs=srcs,
               tap_label=tap_label, row_scale=row_scale, residual=residual, scale=scale, shift=shift, epi_label=epi_label,
               act=act, out_raw=out_raw, out_act=out_act, tile_hint=tile_hint)
    layer.run(_stream(sources[0]))
    return out_raw, out_act


def pad_channels_3to4(img: torch.Tensor) -> torch.Tensor:
    _need_cuda(img)
    b, h, w, c = img.shape
    assert c == 3
    out = torch.empty(b, h, w, 4, dtype=torch.float32, device=img.device)
    check(_lib.load().cp_pad_channels_3to4(img.data_ptr(), out.data_ptr(), b * h * w, _stream(img)), "cp_pad_channels_3to4")
    return out


def maxpool3x3s2(x: torch.Tensor, scale=None, shift=None, relu=False) -> torch.Tensor:
    _need_cuda(x)
    b, h, w, c = x.shape
    out = torch.empty(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, dtype=torch.float32, device=x.device)
    check(_lib.load().cp_maxpool3x3s2_f32(x.data_ptr(), b, h, w, c, scale.data_ptr() if scale is not None else None,
                                          shift.data_ptr() if shift is not None else None, int(relu), out.data_ptr(), _stream(x)),
          "cp_maxpool3x3s2_f32")
    return out


def upsample_bilinear_x2(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    b, h, w, c = x.shape
    out = torch.empty(b, 2 * h, 2 * w, c, dtype=torch.float32, device=x.device)
    check(_lib.load().cp_upsample_bilinear_x2_f32(x.data_ptr(), b, h, w, c, out.data_ptr(), _stream(x)), "cp_upsample_bilinear_x2_f32")
    return out


def guided_upsample_x2(x: torch.Tensor, sel: torch.Tensor) -> torch.Tensor:
    _need_cuda(x, sel)
    b, h, w, c = x.shape
    out = torch.empty(b, 2 * h, 2 * w, c, dtype=torch.float32, device=x.device)
    check(_lib.load().cp_guided_upsample_x2_f32(x.data_ptr(), sel.data_ptr(), b, h, w, c, out.data_ptr(), _stream(x)), "cp_guided_upsample_x2_f32")
    return out


def argmax_labels(logits: torch.Tensor, classes: Optional[int] = None, offset: int = 0) -> torch.Tensor:
    """uint8 arg-max over logits[..., offset:offset+classes]."""
    _need_cuda(logits)
    b, h, w, ld = logits.shape
    classes = classes if classes is not None else ld - offset
    out = torch.empty(b, h, w, dtype=torch.uint8, device=logits.device)
    check(_lib.load().cp_argmax_labels(logits.data_ptr() + 4 * offset, ld, classes, b * h * w, out.data_ptr(), _stream(logits)), "cp_argmax_labels")
    return out


def label_pyramid(labels0: torch.Tensor):
    """Returns (labels[4], pnorm[4], sel[3]) -- see cp_label_pyramid."""
    _need_cuda(labels0)
    b, h, w = labels0.shape
    dev = labels0.device
    hs = [h, h // 2, h // 4, h // 8]
    ws = [w, w // 2, w // 4, w // 8]
    labels = [labels0] + [torch.empty(b, hs[l], ws[l], dtype=torch.uint8, device=dev) for l in range(1, 4)]
    pnorm = [torch.empty(b, hs[l], ws[l], dtype=torch.float32, device=dev) for l in range(4)]
    # guided-upsampling selection maps exist only between levels whose sizes are exactly 2:1
    sel = [torch.empty(b, hs[l], ws[l], dtype=torch.uint8, device=dev) if (hs[l] == 2 * hs[l + 1] and ws[l] == 2 * ws[l + 1] and hs[l + 1] > 0) else None
           for l in range(3)]
    lab = (C.c_void_p * 4)(*[t.data_ptr() if t.numel() else None for t in labels])
    pn = (C.c_void_p * 4)(*[t.data_ptr() if t.numel() else None for t in pnorm])
    sl = (C.c_void_p * 3)(*[t.data_ptr() if t is not None else None for t in sel])
    check(_lib.load().cp_label_pyramid(labels0.data_ptr(), b, h, w, lab, pn, sl, _stream(labels0)), "cp_label_pyramid")
    return labels, pnorm, sel


def ls_vote(field: torch.Tensor, seg_off: int, dir_off: int, conf_off: int, objects: int, kp: int = 9,
            labels: Optional[torch.Tensor] = None, return_sums: bool = False, sigmoid_weights: bool = False):
    """cp_ls_vote_f32 on a [B,H,W,ld] record tensor.  Returns keypoints [B,objects,kp,2] (y,x)."""
    _need_cuda(field, labels)
    b, h, w, ld = field.shape
    lib = _lib.load()
    sums = torch.empty(b, objects, kp, 5, dtype=torch.float64, device=field.device)
    out = torch.empty(b, objects, kp, 2, dtype=torch.float32, device=field.device)
    check(lib.cp_ls_vote_w_f32(field.data_ptr(), ld, seg_off, dir_off, conf_off, labels.data_ptr() if labels is not None else None,
                               b, h, w, objects, kp, 1 if sigmoid_weights else 0, sums.data_ptr(), out.data_ptr(), _stream(field)), "cp_ls_vote_w_f32")
    return (out, sums) if return_sums else out


def ccl_instance_labels(labels: torch.Tensor, objects: int, max_instances: int, min_size: int):
    """cp_ccl_instance_labels on a uint8 label map [B,H,W]: the `max_instances` largest components of each object as separate slots.
    Returns (slot_map uint8 [B,H,W], inst int32 [B,objects,max_instances,2] = (size, image-local root), (0, -1) for an empty slot).
    Instance r of object o (1-based) has the slot id (o-1)*max_instances + r + 1 (include/casapose_hip.h states the rule)."""
    _need_cuda(labels)
    b, h, w = labels.shape
    lib = _lib.load()
    # sizes the library refuses give 0 bytes here; the call below then says what is wrong
    ws = torch.empty(max(int(lib.cp_ccl_instance_workspace_bytes(b, h, w, objects, max_instances)), 1), dtype=torch.uint8, device=labels.device)
    slot_map = torch.empty_like(labels)
    inst = torch.empty(b, max(objects, 0), max(max_instances, 0), 2, dtype=torch.int32, device=labels.device)
    check(lib.cp_ccl_instance_labels(labels.data_ptr(), b, h, w, objects, max_instances, min_size, ws.data_ptr(), slot_map.data_ptr(), inst.data_ptr(),
                                     _stream(labels)), "cp_ccl_instance_labels")
    return slot_map, inst


def ls_vote_slots(rec: torch.Tensor, do: int, co: int, slots: int, kp: int, slot_map: torch.Tensor, sigmoid_weights: bool = False,
                  return_sums: bool = False):
    """cp_ls_vote_slots_f32 on a [B,H,W,ld] record tensor with directions at `do` and confidences at `co`: one vote per slot of `slot_map`
    (uint8 [B,H,W], values 0..slots: as with ls_vote's labels, a larger value is the caller's error and undefined outside the production record --
    ccl_instance_labels never makes one, and nothing here reads the map back to check).  Returns keypoints [B,slots,kp,2] (y,x)."""
    _need_cuda(rec, slot_map)
    b, h, w, ld = rec.shape
    if tuple(slot_map.shape) != (b, h, w) or slot_map.dtype != torch.uint8 or not slot_map.is_contiguous():
        raise ValueError("ls_vote_slots: slot_map must be a contiguous uint8 [%d, %d, %d] tensor" % (b, h, w))
    sums = torch.empty(b, max(slots, 0), kp, 5, dtype=torch.float64, device=rec.device)
    out = torch.empty(b, max(slots, 0), kp, 2, dtype=torch.float32, device=rec.device)
    check(_lib.load().cp_ls_vote_slots_f32(rec.data_ptr(), ld, do, co, slot_map.data_ptr(), b, h, w, slots, kp, 1 if sigmoid_weights else 0,
                                           sums.data_ptr(), out.data_ptr(), _stream(rec)), "cp_ls_vote_slots_f32")
    return (out, sums) if return_sums else out


def ls_vote_slots_robust(rec: torch.Tensor, do: int, co: int, slots: int, kp: int, slot_map: torch.Tensor, cutoff: float = 4.0, passes: int = 2,
                         sigmoid_weights: bool = False, return_sums: bool = False):
    """cp_ls_vote_slots_robust_f32: ls_vote_slots followed by `passes` reweighted passes, every term weighted by Tukey's biweight (cut-off
    `cutoff` pixels) of the distance of the current estimate from the pixel's line; include/casapose_hip.h states the rule.  Returns keypoints
    [B,slots,kp,2] (y,x); with return_sums also the plain sums and the last pass's reweighted sums, fp64 [B,slots,kp,5] each (views of one
    workspace; the second is not written with passes = 0)."""
    _need_cuda(rec, slot_map)
    b, h, w, ld = rec.shape
    if tuple(slot_map.shape) != (b, h, w) or slot_map.dtype != torch.uint8 or not slot_map.is_contiguous():
        raise ValueError("ls_vote_slots_robust: slot_map must be a contiguous uint8 [%d, %d, %d] tensor" % (b, h, w))
    ws = torch.empty(2, b, max(slots, 0), kp, 5, dtype=torch.float64, device=rec.device)
    out = torch.empty(b, max(slots, 0), kp, 2, dtype=torch.float32, device=rec.device)
    check(_lib.load().cp_ls_vote_slots_robust_f32(rec.data_ptr(), ld, do, co, slot_map.data_ptr(), b, h, w, slots, kp, 1 if sigmoid_weights else 0,
                                                  float(cutoff), int(passes), ws.data_ptr(), out.data_ptr(), _stream(rec)),
          "cp_ls_vote_slots_robust_f32")
    return (out, ws[0], ws[1]) if return_sums else out


def ls_slot_covariance(rec: torch.Tensor, do: int, co: int, slots: int, kp: int, slot_map: torch.Tensor, keypoints: torch.Tensor, cutoff=None,
                       sigmoid_weights: bool = False, return_sums: bool = False):
    """cp_ls_slot_covariance_f32: a covariance per (image, slot, keypoint) of `keypoints` (fp32 [B,slots,kp,2] in (y,x), either slot voter's
    result; only read) from one more pass over the slot map; include/casapose_hip.h states the rule.  cutoff: pixels of Tukey's biweight, None
    (or 0) for no reweighting.  Returns (cov fp32 [B,slots,kp,3] = (sxx, sxy, syy) in (x,y) pixels, three NaNs where there is none,
    stat fp32 [B,slots,kp,2] = (sigma2, kept)); with return_sums also the five sums (A00, A01, A11, Q, Wall), fp64 [B,slots,kp,5]."""
    _need_cuda(rec, slot_map, keypoints)
    b, h, w, ld = rec.shape
    if tuple(slot_map.shape) != (b, h, w) or slot_map.dtype != torch.uint8 or not slot_map.is_contiguous():
        raise ValueError("ls_slot_covariance: slot_map must be a contiguous uint8 [%d, %d, %d] tensor" % (b, h, w))
    n = max(slots, 0)
    if keypoints.dtype != torch.float32 or keypoints.numel() != b * n * kp * 2 or not keypoints.is_contiguous():
        raise ValueError("ls_slot_covariance: keypoints must be a contiguous float32 tensor of [%d, %d, %d, 2] values" % (b, n, kp))
    sums = torch.empty(b, n, kp, 5, dtype=torch.float64, device=rec.device)
    cov = torch.empty(b, n, kp, 3, dtype=torch.float32, device=rec.device)
    stat = torch.empty(b, n, kp, 2, dtype=torch.float32, device=rec.device)
    check(_lib.load().cp_ls_slot_covariance_f32(rec.data_ptr(), ld, do, co, slot_map.data_ptr(), b, h, w, slots, kp, 1 if sigmoid_weights else 0,
                                                0.0 if cutoff is None else float(cutoff), keypoints.data_ptr(), sums.data_ptr(), cov.data_ptr(),
                                                stat.data_ptr(), _stream(rec)), "cp_ls_slot_covariance_f32")
    return (cov, stat, sums) if return_sums else (cov, stat)


VOTE_SPLIT_DEFAULTS = dict(kp_index=0, cell=4, vote_stride=2, min_votes=12, rel_percent=25, nms_radius=2, gate=4.0, min_size=50)


def vote_split_labels(labels: torch.Tensor, field_record: torch.Tensor, dir_off: int, objects: int, max_instances: int, return_workspace: bool = False,
                      **params):
    """cp_vote_split_labels on a uint8 label map [B,H,W] and a [B,H,W,ld] record tensor with directions at `dir_off`: touching instances of one
    object split by their votes for the object's centre (keypoint `kp_index`, 0 by default).  params: VOTE_SPLIT_DEFAULTS' keys; include/casapose_hip.h
    states the rule.  Returns (slot_map uint8 [B,H,W], inst int32 [B,objects,max_instances,4] = (pixels, votes, peak cy, peak cx), peaks float32
    [B,objects,max_instances,2] in (y,x)); slot ids are ccl_instance_labels'.  return_workspace adds the workspace (a uint8 tensor; its parts lie
    where cp_vote_split_workspace_layout says)."""
    unknown = set(params) - set(VOTE_SPLIT_DEFAULTS)
    if unknown:
        raise TypeError("vote_split_labels: unknown parameter(s) %s (known: %s)" % (sorted(unknown), sorted(VOTE_SPLIT_DEFAULTS)))
    p = dict(VOTE_SPLIT_DEFAULTS, **params)
    _need_cuda(labels, field_record)
    b, h, w = labels.shape
    if (tuple(field_record.shape[:3]) != (b, h, w) or field_record.dim() != 4 or field_record.dtype != torch.float32 or not field_record.is_contiguous()
            or labels.dtype != torch.uint8 or not labels.is_contiguous()):
        raise ValueError("vote_split_labels: labels must be a contiguous uint8 [B,H,W] tensor and field_record a contiguous float32 [B,H,W,ld] one")
    ld = field_record.shape[3]
    lib = _lib.load()
    # sizes the library refuses give 0 bytes here; the call below then says what is wrong
    ws = torch.empty(max(int(lib.cp_vote_split_workspace_bytes(b, h, w, objects, max_instances, int(p["cell"]))), 16), dtype=torch.uint8,
                     device=labels.device)
    slot_map = torch.empty_like(labels)
    inst = torch.empty(b, max(objects, 0), max(max_instances, 0), 4, dtype=torch.int32, device=labels.device)
    peaks = torch.empty(b, max(objects, 0), max(max_instances, 0), 2, dtype=torch.float32, device=labels.device)
    check(lib.cp_vote_split_labels(labels.data_ptr(), field_record.data_ptr(), ld, dir_off, int(p["kp_index"]), b, h, w, objects, max_instances,
                                   int(p["cell"]), int(p["vote_stride"]), int(p["min_votes"]), int(p["rel_percent"]), int(p["nms_radius"]),
                                   float(p["gate"]), int(p["min_size"]), ws.data_ptr(), slot_map.data_ptr(), inst.data_ptr(), peaks.data_ptr(),
                                   _stream(labels)), "cp_vote_split_labels")
    return (slot_map, inst, peaks, ws) if return_workspace else (slot_map, inst, peaks)
