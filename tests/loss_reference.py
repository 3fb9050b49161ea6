"""TEST INFRASTRUCTURE -- a staged fp64 restatement of compute_loss's three terms (train_casapose.py:40-145) as the pose-loss kernels evaluate
them (csrc/loss_kernels.hip, csrc/loss_functional.hip), written from the formulas in the kernels' header comments and the lines they cite:
  mask   : mean softmax cross-entropy against labels_ce                                            (train_casapose.py:59-60)
  vertex : smooth-L1 between the predicted directions and the unit vectors pixel centre -> keypoint  (utils/loss_functions.py:14-44)
  proxy  : smooth-L1 of the distance between the keypoint and the line through the pixel centre along the predicted direction, 0 for a zero
           direction (divide_no_nan)                                                               (utils/loss_functions.py:132-203)
Unlike the oracles (torch_train_ref.losses, loss_functions_ref.compute_loss_separated) it takes labels_ce and labels_fg SEPARATELY -- target_seg and
filtered_seg of train_casapose.py:62-63 -- and returns every intermediate the kernels leave in their workspace.  Nothing here imports the package
under test.  tests/test_loss_reference.py anchors it to the two oracles on the CPU."""
from types import SimpleNamespace

import numpy as np
import torch

MIN_OBJECT_PIXEL = 20      # proxy_voting_dist, loss_functions.py:47: objects below it report 0
MAX_VALUE = 5.0            # train_casapose.py:82: an object is kept iff its value < 5


def _sl1(a):
    return torch.where(a < 1.0, 0.5 * a * a, a - 0.5)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def first_argmax(logits):
    """index of the FIRST maximum along the last axis (tf.argmax), written out so that it does not rest on a library's tie rule"""
    best = logits[..., 0].copy()
    arg = np.zeros(logits.shape[:-1], np.int64)
    for k in range(1, logits.shape[-1]):
        better = logits[..., k] > best
        best = np.where(better, logits[..., k], best)
        arg = np.where(better, k, arg)
    return arg


def segmentation_filter(logits, labels_fg):
    """filter_vertex_with_segmentation (train_casapose.py:64-69): a foreground pixel stays iff the arg-max prediction equals its label"""
    lab = labels_fg.astype(np.int64)
    return np.where(first_argmax(np.asarray(logits, np.float64)) == lab, lab, 0)


def _pixel_terms(v, fg, kpts):
    """v [b,h,w,kp,2] (dy,dx) torch fp64, fg [b,h,w] int64 numpy (0 = background), kpts [b,objects,kp,2] (y,x) ->
    per (pixel, keypoint, component) smooth-L1 of the vertex error [b,h,w,kp,2], per (pixel, keypoint) smooth-L1 of the proxy distance [b,h,w,kp],
    both zero on background, and the raw quantities the kernels branch on"""
    b, h, w = fg.shape
    fgt = torch.from_numpy(fg)
    on = (fgt != 0)
    k = _t(kpts)[torch.arange(b)[:, None, None], torch.clamp(fgt - 1, min=0)]            # [b,h,w,kp,2]
    cy = (torch.arange(h, dtype=torch.float64) + 0.5)[None, :, None, None]
    cx = (torch.arange(w, dtype=torch.float64) + 0.5)[None, None, :, None]
    ay, ax = k[..., 0] - cy, k[..., 1] - cx                                               # pixel centre -> keypoint
    tn = torch.sqrt(ay * ay + ax * ax)
    it = 1.0 / torch.clamp(tn, min=1e-12)                                                 # tf.math.l2_normalize; tn == 0 gives the target (0, 0)
    vy, vx = v[..., 0], v[..., 1]
    ey, ex = (vy - ay * it).abs(), (vx - ax * it).abs()
    num = vy * ax - vx * ay
    n2 = vy * vy + vx * vx
    nz = n2 > 0
    dist = torch.where(nz, num.abs() / torch.sqrt(torch.where(nz, n2, torch.ones_like(n2))), torch.zeros_like(n2))
    m = on[..., None].to(torch.float64)
    raw = SimpleNamespace(on=on.numpy(), tn=tn.detach().numpy(), num=num.detach().numpy(), n2=n2.detach().numpy(), ey=ey.detach().numpy(),
                          ex=ex.detach().numpy(), dist=dist.detach().numpy())
    return torch.stack([_sl1(ey), _sl1(ex)], -1) * m[..., None], _sl1(dist) * m, raw


def _cross_entropy(z, labels_ce):
    lc = torch.from_numpy(labels_ce.astype(np.int64))
    return (torch.logsumexp(z, dim=-1) - torch.gather(z, -1, lc[..., None])[..., 0]).mean()


def merged(out, labels_ce, labels_fg, kpts, K, kp, seg_filter, proxy_filter, weights=(1.0, 0.5, 0.015)):
    """cp_pose_loss_f32.  out [b,h,w,>=K+2kp]: K logits, then 2kp directions (dy,dx); labels uint8 [b,h,w]; kpts [b,K-1,kp,2] (y,x).
    Returns fg0/count0 (after the optional segmentation filter), objsum/objcnt/value/bad [b,K-1] (on fg0), fg1/count1 (after the optional
    high-proxy-error filter: what the vertex and proxy terms use), the three losses, and the gradient of mask_w*mask + vertex_w*vertex +
    proxy_w*proxy with respect to the logits [b,h,w,K] and the directions [b,h,w,2kp]; the foreground maps are constants."""
    out = np.asarray(out)
    b, h, w = labels_fg.shape
    objects = K - 1
    z = _t(out[..., :K]).requires_grad_(True)
    v = _t(out[..., K:K + 2 * kp]).requires_grad_(True)
    v5 = v.reshape(b, h, w, kp, 2)
    fg0 = segmentation_filter(out[..., :K], labels_fg) if seg_filter else labels_fg.astype(np.int64)
    count0 = (fg0 != 0).reshape(b, -1).sum(1)
    with torch.no_grad():
        _, px, _ = _pixel_terms(v5, fg0, kpts)
        per_px = px.sum(-1).numpy()                                                       # [b,h,w]
    objsum, objcnt = np.zeros((b, objects)), np.zeros((b, objects), np.int64)
    for o in range(objects):
        m = fg0 == o + 1
        objcnt[:, o] = m.reshape(b, -1).sum(1)
        objsum[:, o] = (per_px * m).reshape(b, -1).sum(1)
    value = np.where(objcnt >= MIN_OBJECT_PIXEL, objsum / (kp * objcnt + 1e-3), 0.0)
    bad = ~(value < MAX_VALUE)
    fg1 = fg0
    if proxy_filter:
        drop = np.concatenate([np.zeros((b, 1), bool), bad], 1)                           # per label; the background is never "dropped"
        fg1 = np.where(drop[np.arange(b)[:, None, None], fg0], 0, fg0)
    count1 = (fg1 != 0).reshape(b, -1).sum(1)
    mask = _cross_entropy(z, labels_ce)
    e, d, raw = _pixel_terms(v5, fg1, kpts)
    nrm = _t(1.0 / (2.0 * kp * count1 + 1e-3))                                            # per image (smooth_l1_loss's / proxy_voting_loss_v2's normalize)
    vertex = (e.reshape(b, -1).sum(1) * nrm).mean()
    proxy = (d.reshape(b, -1).sum(1) * nrm).mean()
    (weights[0] * mask + weights[1] * vertex + weights[2] * proxy).backward()
    return SimpleNamespace(fg0=fg0.astype(np.uint8), count0=count0, objsum=objsum, objcnt=objcnt, value=value, bad=bad, fg1=fg1.astype(np.uint8),
                           count1=count1, mask=mask.item(), vertex=vertex.item(), proxy=proxy.item(), grad_logits=z.grad.numpy(),
                           grad_dirs=v.grad.numpy(), raw=raw)


def separated(out, labels_ce, labels_fg, kpts, K, kp, seg_filter, weights=(1.0, 0.5, 0.015)):
    """cp_pose_loss_sep_f32 (train_casapose.py:57,97-125).  out [b,h,w,>=K+(K-1)*2kp]: K logits, then the 2kp directions of object o at
    K + o*2kp; a pixel contributes to the slice of its own object, normalised by 2kp * (pixels of that object in its image) + 1e-3, mean over the
    batch.  Returns fg, counts [b,K] (entry 0 of an image is 0), the three losses and the gradient (logits [b,h,w,K], directions [b,h,w,(K-1)*2kp])."""
    out = np.asarray(out)
    b, h, w = labels_fg.shape
    objects = K - 1
    z = _t(out[..., :K]).requires_grad_(True)
    v = _t(out[..., K:K + objects * 2 * kp]).requires_grad_(True)
    fg = segmentation_filter(out[..., :K], labels_fg) if seg_filter else labels_fg.astype(np.int64)
    counts = np.zeros((b, K), np.int64)
    for l in range(1, K):
        counts[:, l] = (fg == l).reshape(b, -1).sum(1)
    fgt = torch.from_numpy(fg)
    own = v.reshape(b, h, w, objects, kp, 2)[torch.arange(b)[:, None, None], torch.arange(h)[None, :, None], torch.arange(w)[None, None, :],
                                             torch.clamp(fgt - 1, min=0)]                 # [b,h,w,kp,2]: the slice of the pixel's own object
    mask = _cross_entropy(z, labels_ce)
    e, d, raw = _pixel_terms(own, fg, kpts)
    nrm = _t(1.0 / (2.0 * kp * counts + 1e-3))[torch.arange(b)[:, None, None], fgt] / b   # per (image, object), at every pixel
    vertex = (e.sum((-1, -2)) * nrm).sum()
    proxy = (d.sum(-1) * nrm).sum()
    (weights[0] * mask + weights[1] * vertex + weights[2] * proxy).backward()
    return SimpleNamespace(fg=fg.astype(np.uint8), counts=counts, mask=mask.item(), vertex=vertex.item(), proxy=proxy.item(),
                           grad_logits=z.grad.numpy(), grad_dirs=v.grad.numpy(), raw=raw)
