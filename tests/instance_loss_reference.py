"""TEST INFRASTRUCTURE -- tests/loss_reference.py's staged fp64 restatement with an INSTANCE axis, as cp_pose_loss_inst_f32 evaluates it
(csrc/loss_kernels.hip), written from the entry's header comment (include/casapose_hip.h) and the reference lines it cites:
  which instance a pixel's vertex target follows: the one whose keypoint 0 is nearest, first minimum     (utils/image_utils.py:17-63, tf.argmin)
  the proxy distance of a keypoint: the minimum over the object's instances, per keypoint, first minimum (utils/loss_functions.py:109-111,170-172)
  absent instances (index >= the object's count) are padding and take part in nothing                    (vectorfield_dataset.py:458-470)
With an instance map both terms use the instance the map names.  Nothing here imports the package under test.
tests/test_instance_loss_reference.py anchors it to loss_reference.merged (I = 1) and to oracle/loss_functions_ref.py (I > 1) on the CPU."""
from types import SimpleNamespace

import numpy as np
import torch

from loss_reference import MAX_VALUE, MIN_OBJECT_PIXEL, _cross_entropy, _sl1, _t, segmentation_filter


def first_argmin(values):
    """index of the FIRST minimum along axis 0 of a torch fp64 tensor (tf.argmin / reduce_min), written out; inf entries never win over a finite one"""
    best = values[0].clone()
    arg = torch.zeros(values.shape[1:], dtype=torch.int64)
    for r in range(1, values.shape[0]):
        better = values[r] < best
        best = torch.where(better, values[r], best)
        arg = torch.where(better, torch.full_like(arg, r), arg)
    return arg


def second_gap(values):
    """second smallest minus smallest along axis 0 (inf where fewer than two finite entries): how far the choice of the minimum is from a tie"""
    s, _ = torch.sort(values, dim=0)
    if s.shape[0] < 2:
        return torch.full(values.shape[1:], np.inf, dtype=torch.float64)
    gap = s[1] - s[0]
    return torch.where(torch.isfinite(s[1]), gap, torch.full_like(gap, np.inf))


def instance_foreground(fg, counts, inst_map):
    """a foreground pixel stays iff its object has an instance and, with a map, the map names one of them"""
    b = fg.shape[0]
    n = np.concatenate([np.zeros((b, 1), np.int64), counts.astype(np.int64)], 1)[np.arange(b)[:, None, None], fg]     # count of the pixel's object
    keep = n > 0
    if inst_map is not None:
        keep &= inst_map.astype(np.int64) < n
    return np.where(keep, fg, 0)


def _pixel_terms(v, fg, kpts, counts, inst_map):
    """v [b,h,w,kp,2] torch fp64; fg [b,h,w] int64 (already through instance_foreground); kpts [b,objects,I,kp,2]; counts [b,objects].
    -> smooth-L1 vertex terms [b,h,w,kp,2], smooth-L1 proxy terms [b,h,w,kp] (zero on background), and raw: the chosen instances and the gaps"""
    b, h, w = fg.shape
    I = kpts.shape[2]
    fgt = torch.from_numpy(fg)
    on = fgt != 0
    obj = torch.clamp(fgt - 1, min=0)
    bi = torch.arange(b)[:, None, None]
    n = torch.from_numpy(counts.astype(np.int64))[bi, obj]                                   # [b,h,w]
    valid = (torch.arange(I)[:, None, None, None] < n[None]) & on[None]                      # [I,b,h,w]
    present = np.arange(I)[None, None, :] < counts[:, :, None]
    k = _t(np.where(present[..., None, None], kpts, 0.0))[bi, obj]                          # [b,h,w,I,kp,2]; padding (any value, NaN too) never enters
    k = k.permute(3, 0, 1, 2, 4, 5)                                                          # [I,b,h,w,kp,2]
    cy = (torch.arange(h, dtype=torch.float64) + 0.5)[None, None, :, None, None]
    cx = (torch.arange(w, dtype=torch.float64) + 0.5)[None, None, None, :, None]
    ay, ax = k[..., 0] - cy, k[..., 1] - cx                                                  # [I,b,h,w,kp]
    inf = torch.full((), np.inf, dtype=torch.float64)
    centre = torch.where(valid, torch.sqrt(ay[..., 0] ** 2 + ax[..., 0] ** 2), inf)          # [I,b,h,w]
    if inst_map is not None:
        rv = torch.from_numpy(inst_map.astype(np.int64)) * on
        centre_gap = torch.full((b, h, w), np.inf, dtype=torch.float64)
    else:
        rv = first_argmin(centre) * on
        centre_gap = second_gap(centre)
    pick = lambda t, r: torch.gather(t, 0, r[None].expand((1,) + t.shape[1:]))[0]            # noqa: E731  t [I,...] at instance r [...]
    rv5 = rv[..., None].expand(b, h, w, ay.shape[-1])
    vay, vax = pick(ay, rv5), pick(ax, rv5)
    tn = torch.sqrt(vay * vay + vax * vax)
    it = 1.0 / torch.clamp(tn, min=1e-12)
    vy, vx = v[..., 0], v[..., 1]
    ey, ex = (vy - vay * it).abs(), (vx - vax * it).abs()
    n2 = vy * vy + vx * vx
    nz = n2 > 0
    nr = torch.sqrt(torch.where(nz, n2, torch.ones_like(n2)))
    num = vy[None] * ax - vx[None] * ay                                                      # [I,b,h,w,kp]
    cand = torch.where(valid[..., None] & nz[None], num.abs() / nr[None], inf)
    if inst_map is not None:
        rp = rv5
        proxy_gap = torch.full(n2.shape, np.inf, dtype=torch.float64)
    else:
        rp = first_argmin(cand.detach()) * on[..., None]
        proxy_gap = second_gap(cand.detach())
    dist = torch.where(nz, pick(num, rp).abs() / nr, torch.zeros_like(n2))
    m = on[..., None].to(torch.float64)
    raw = SimpleNamespace(on=on.numpy(), rv=rv.numpy(), rp=rp.numpy(), centre_gap=centre_gap.numpy(), proxy_gap=proxy_gap.numpy(),
                          n2=n2.detach().numpy(), dist=(dist * m).detach().numpy(), target=torch.stack([vay * it, vax * it], -1).numpy() * m[..., None].numpy())
    return torch.stack([_sl1(ey), _sl1(ex)], -1) * m[..., None], _sl1(dist) * m, raw


def merged_instances(out, labels_ce, labels_fg, kpts, counts, inst_map, K, kp, seg_filter, proxy_filter, weights=(1.0, 0.5, 0.015)):
    """cp_pose_loss_inst_f32.  kpts [b,K-1,I,kp,2] (y,x); counts int [b,K-1] in 0..I; inst_map uint8 [b,h,w] or None (the nearest-centre rule).
    Returns what loss_reference.merged returns, stage by stage, with raw.rv / raw.rp (the instances the vertex and the proxy term took) and
    raw.centre_gap / raw.proxy_gap (how far each choice was from a tie, in pixels; inf where there was no choice)."""
    out = np.asarray(out)
    b, h, w = labels_fg.shape
    objects = K - 1
    z = _t(out[..., :K]).requires_grad_(True)
    v = _t(out[..., K:K + 2 * kp]).requires_grad_(True)
    v5 = v.reshape(b, h, w, kp, 2)
    fg0 = segmentation_filter(out[..., :K], labels_fg) if seg_filter else labels_fg.astype(np.int64)
    fg0 = instance_foreground(fg0, counts, inst_map)
    count0 = (fg0 != 0).reshape(b, -1).sum(1)
    with torch.no_grad():
        _, px, _ = _pixel_terms(v5, fg0, kpts, counts, inst_map)
        per_px = px.sum(-1).numpy()
    objsum, objcnt = np.zeros((b, objects)), np.zeros((b, objects), np.int64)
    for o in range(objects):
        m = fg0 == o + 1
        objcnt[:, o] = m.reshape(b, -1).sum(1)
        objsum[:, o] = (per_px * m).reshape(b, -1).sum(1)
    value = np.where(objcnt >= MIN_OBJECT_PIXEL, objsum / (kp * objcnt + 1e-3), 0.0)
    bad = ~(value < MAX_VALUE)
    fg1 = fg0
    if proxy_filter:
        drop = np.concatenate([np.zeros((b, 1), bool), bad], 1)
        fg1 = np.where(drop[np.arange(b)[:, None, None], fg0], 0, fg0)
    count1 = (fg1 != 0).reshape(b, -1).sum(1)
    mask = _cross_entropy(z, labels_ce)
    e, d, raw = _pixel_terms(v5, fg1, kpts, counts, inst_map)
    nrm = _t(1.0 / (2.0 * kp * count1 + 1e-3))
    vertex = (e.reshape(b, -1).sum(1) * nrm).mean()
    proxy = (d.reshape(b, -1).sum(1) * nrm).mean()
    (weights[0] * mask + weights[1] * vertex + weights[2] * proxy).backward()
    return SimpleNamespace(fg0=fg0.astype(np.uint8), count0=count0, objsum=objsum, objcnt=objcnt, value=value, bad=bad, fg1=fg1.astype(np.uint8),
                           count1=count1, mask=mask.item(), vertex=vertex.item(), proxy=proxy.item(), grad_logits=z.grad.numpy(),
                           grad_dirs=v.grad.numpy(), raw=raw)
