"""Plain NumPy float64 restatements of the streaming kernels between the convolutions (csrc/aux_kernels.hip, csrc/guided_bilinear.hip and the
resampling / utility part of csrc/train_kernels.hip), written from the layer definitions, not from the kernels' closed forms:

  * the guided layers work on the four taps {(y,x),(y,x+1),(y+1,x),(y+1,x+1)} of the low-resolution map, zero padded bottom / right
    (GuidedUpsampling and GuidedBilinearUpsampling of the reference project);
  * bilinear x2 samples half-pixel centres with an edge clamp;
  * the 3x3 / stride 2 max-pool pads with ZEROS that take part in the maximum; ties go to the first maximum in raster order.

The forwards gather, the adjoints SCATTER (np.add.at per hi-res pixel and tap), so an adjoint here shares nothing with the kernels' gather form.
Where the GPU comparison is rounding-bounded the functions return, per output element, `S` = the sum of the absolute products and `n` = the
number of products in that element's sum: the bound of test_gpu_resample_stages.py is built from them."""
from types import SimpleNamespace

import numpy as np

TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))                # (dy, dx) of tap j = 2 dy + dx
SUB_WEIGHTS = np.array([[1.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.5, 0.0, 0.5, 0.0], [0.25, 0.25, 0.25, 0.25]])   # [sub-pixel, tap]


def up2(a):
    """every low-res cell repeated over its 2x2 hi-res pixels (axes 1 and 2)"""
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)


def sub_pixel(h, w):
    """[2h, 2w]: 2 (Y % 2) + (X % 2)"""
    yy, xx = np.meshgrid(np.arange(2 * h), np.arange(2 * w), indexing="ij")
    return (yy % 2) * 2 + (xx % 2)


def tap_labels(lo):
    """[B,H,W,4] the low-res label of each tap, -1 for a tap outside the map (it equals no label)"""
    b, h, w = lo.shape
    lp = np.full((b, h + 1, w + 1), -1, np.int64)
    lp[:, :h, :w] = lo
    return np.stack([lp[:, dy:dy + h, dx:dx + w] for dy, dx in TAPS], axis=-1)


def tap_values(x):
    """[B,H,W,4,C] the value of each tap, zero outside the map"""
    b, h, w, c = x.shape
    xp = np.zeros((b, h + 1, w + 1, c), np.float64)
    xp[:, :h, :w] = x
    return np.stack([xp[:, dy:dy + h, dx:dx + w] for dy, dx in TAPS], axis=3)


def matches(hi, lo):
    """[B,2H,2W,4] bool: tap j of the pixel's low-res cell carries the pixel's hi-res label"""
    return up2(tap_labels(lo)) == np.asarray(hi, np.int64)[..., None]


def match_mask(hi, lo):
    """the 4-bit set of matching taps per hi-res pixel, uint8 [B,2H,2W]"""
    return (matches(hi, lo) * np.array([1, 2, 4, 8])).sum(-1).astype(np.uint8)


def mask_bits(mask):
    return ((np.asarray(mask, np.int64)[..., None] >> np.arange(4)) & 1).astype(bool)


def sel_map(hi, lo):
    """guided nearest selection: the first matching tap of the four, else tap 0; uint8 [B,2H,2W]"""
    m = matches(hi, lo)
    return np.where(m.any(-1), np.argmax(m, axis=-1), 0).astype(np.uint8)


def guided_bilinear_coefficients(mask):
    """[B,2H,2W,4] from the layer's definition: the blend is sum_j w_j f_j with f_j = tap_j where tap j matches, else the mean of the matching
    taps (zero if none matches).  f = F tap with F[j,k] = [j == k] for a matching j and match_k / #matching otherwise, so coef = w F."""
    m = mask_bits(mask)                                                   # [B,Y,X,4]
    _, hh, ww, _ = m.shape
    w = SUB_WEIGHTS[sub_pixel(hh // 2, ww // 2)][None]                    # [1,Y,X,4]
    n = m.sum(-1)
    mean_row = np.where(n[..., None] > 0, m / np.maximum(n, 1)[..., None], 0.0)      # f_j for a non-matching j, as a row over k
    f = np.where(m[..., :, None], np.eye(4)[None, None, None], mean_row[..., None, :])   # [B,Y,X,j,k]
    return (w[..., :, None] * f).sum(-2)


def _blend(coef, taps):
    """out = sum_j coef_j tap_j over [B,Y,X,4(,C)]; the sum of absolute products and the number of non-zero coefficients with it"""
    p = coef[..., None] * taps
    n = np.broadcast_to((coef != 0).sum(-1)[..., None], p.shape[:3] + p.shape[4:])
    return SimpleNamespace(out=p.sum(3), S=np.abs(p).sum(3), n=n, coef=coef)


def guided_bilinear(x, mask):
    return _blend(guided_bilinear_coefficients(mask), up2(tap_values(np.asarray(x, np.float64))))


def _scatter_taps(coef, dy, h, w):
    """for every hi-res pixel and tap j: coef_j * dy added into low-res (Y // 2 + dy_j, X // 2 + dx_j); what lands on the padding is dropped.
    Returns dx, the sum of absolute products and the number of non-zero products per low-res pixel."""
    b, hh, ww, c = dy.shape
    dx = np.zeros((b * (h + 1) * (w + 1), c))
    s = np.zeros_like(dx)
    n = np.zeros(b * (h + 1) * (w + 1))
    bi, yy, xx = np.meshgrid(np.arange(b), np.arange(hh), np.arange(ww), indexing="ij")
    for j, (ty, tx) in enumerate(TAPS):
        flat = ((bi * (h + 1) + yy // 2 + ty) * (w + 1) + xx // 2 + tx).ravel()
        p = (coef[..., j, None] * dy).reshape(-1, c)
        np.add.at(dx, flat, p)
        np.add.at(s, flat, np.abs(p))
        np.add.at(n, flat, (coef[..., j] != 0).ravel().astype(np.float64))
    cut = lambda a: a.reshape((b, h + 1, w + 1) + a.shape[1:])[:, :h, :w]
    return SimpleNamespace(out=cut(dx), S=cut(s), n=np.broadcast_to(cut(n)[..., None], (b, h, w, c)))


def guided_bilinear_bwd(dy, mask):
    b, hh, ww, _ = dy.shape
    return _scatter_taps(guided_bilinear_coefficients(mask), np.asarray(dy, np.float64), hh // 2, ww // 2)


def _selected(sel, h, w):
    """low-res (row, column) that every hi-res pixel selects; a selection on the padding is a mistake of the caller"""
    _, hh, ww = sel.shape
    yy, xx = np.meshgrid(np.arange(hh), np.arange(ww), indexing="ij")
    sy, sx = yy[None] // 2 + sel // 2, xx[None] // 2 + sel % 2
    assert sel.max() <= 3 and sy.max() < h and sx.max() < w, "a selection points at the padding"
    return sy, sx


def guided_nearest(x, sel):
    b, h, w, _ = x.shape
    sy, sx = _selected(np.asarray(sel, np.int64), h, w)
    return x[np.arange(b)[:, None, None], sy, sx]


def guided_nearest_bwd(dy, sel):
    b, hh, ww, c = dy.shape
    h, w = hh // 2, ww // 2
    sy, sx = _selected(np.asarray(sel, np.int64), h, w)
    dx = np.zeros((b * h * w, c))
    np.add.at(dx, ((np.arange(b)[:, None, None] * h + sy) * w + sx).ravel(), np.asarray(dy, np.float64).reshape(-1, c))
    return dx.reshape(b, h, w, c)


def _half_pixel_taps(size):
    """per output index of one axis: the two source indices (edge clamped) and the fraction of the second"""
    src = (np.arange(2 * size) + 0.5) / 2.0 - 0.5
    i0 = np.floor(src).astype(np.int64)
    return np.clip(i0, 0, size - 1), np.clip(i0 + 1, 0, size - 1), src - i0


def _bilinear_terms(h, w):
    """the four (row index [2h], column index [2w], weight [2h,2w]) terms of every output pixel"""
    y0, y1, fy = _half_pixel_taps(h)
    x0, x1, fx = _half_pixel_taps(w)
    return [(ya, xa, np.outer(wy, wx)) for ya, wy in ((y0, 1 - fy), (y1, fy)) for xa, wx in ((x0, 1 - fx), (x1, fx))]


def bilinear_x2(x):
    x = np.asarray(x, np.float64)
    _, h, w, _ = x.shape
    p = np.stack([x[:, ya][:, :, xa] * wt[None, :, :, None] for ya, xa, wt in _bilinear_terms(h, w)], axis=3)
    return SimpleNamespace(out=p.sum(3), S=np.abs(p).sum(3), n=np.full(p.shape[:3] + p.shape[4:], 4))


def bilinear_x2_bwd(dy):
    dy = np.asarray(dy, np.float64)
    b, hh, ww, c = dy.shape
    h, w = hh // 2, ww // 2
    dx, s, n = np.zeros((b * h * w, c)), np.zeros((b * h * w, c)), np.zeros(b * h * w)
    bi = np.arange(b)[:, None, None]
    for ya, xa, wt in _bilinear_terms(h, w):
        flat = ((bi * h + ya[None, :, None]) * w + xa[None, None, :]).ravel()
        p = (dy * wt[None, :, :, None]).reshape(-1, c)
        np.add.at(dx, flat, p)
        np.add.at(s, flat, np.abs(p))
        np.add.at(n, flat, 1.0)
    return SimpleNamespace(out=dx.reshape(b, h, w, c), S=s.reshape(b, h, w, c), n=np.broadcast_to(n.reshape(b, h, w, 1), (b, h, w, c)))


def pool_size(n):
    return (n - 1) // 2 + 1


def _pool_windows(x):
    """[B,Ho,Wo,9,C] the 3x3 / stride 2 windows of x padded by one ring of zeros, tap = 3 ky + kx; [Ho,Wo,9] whether the tap lies in the image"""
    b, h, w, c = x.shape
    ho, wo = pool_size(h), pool_size(w)
    xp = np.zeros((b, 2 * ho + 1, 2 * wo + 1, c), x.dtype)
    xp[:, 1:h + 1, 1:w + 1] = x
    inside = np.zeros((2 * ho + 1, 2 * wo + 1), bool)
    inside[1:h + 1, 1:w + 1] = True
    win = np.stack([xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] for ky in range(3) for kx in range(3)], axis=3)
    return win, np.stack([inside[ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] for ky in range(3) for kx in range(3)], axis=-1)


def maxpool(x):
    """value and tap 0..8 of the first maximum in raster order; `pad_wins`: that tap is padding; `win` / `inside` for the cases' conditions"""
    win, inside = _pool_windows(np.asarray(x))
    idx = np.argmax(win, axis=3)                                   # the first maximum
    val = np.take_along_axis(win, idx[:, :, :, None], axis=3)[:, :, :, 0]
    pad_wins = ~np.take_along_axis(np.broadcast_to(inside[None, :, :, :, None], win.shape), idx[:, :, :, None], axis=3)[:, :, :, 0]
    return SimpleNamespace(val=val, idx=idx.astype(np.uint8), pad_wins=pad_wins, win=win, inside=inside)


def scale_shift(m, scale, shift, relu):
    """the fused consumer of the pooled value m: m * scale + shift (and ReLU), with the magnitude |m scale| + |shift| of the bound"""
    m = np.asarray(m, np.float64)
    y = m * scale + shift
    return SimpleNamespace(out=np.maximum(y, 0.0) if relu else y, mag=np.abs(m * scale) + np.abs(shift))


def maxpool_bwd(x, dy, dx_prev=None, pooled=None):
    """dy of every output element scattered to the input its window's first maximum sits on; dropped when that tap is padding
    (`pooled`: maxpool(x), where the caller has it already)"""
    b, h, w, c = x.shape
    r = maxpool(x) if pooled is None else pooled
    _, ho, wo, _ = r.idx.shape
    bi, oy, ox, ci = np.meshgrid(np.arange(b), np.arange(ho), np.arange(wo), np.arange(c), indexing="ij")
    iy, ix = 2 * oy - 1 + r.idx // 3, 2 * ox - 1 + r.idx % 3
    keep = ~r.pad_wins
    assert np.array_equal(keep, (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w))
    dx = np.zeros((b, h, w, c)) if dx_prev is None else np.array(dx_prev, np.float64)
    np.add.at(dx, (bi[keep], iy[keep], ix[keep], ci[keep]), np.asarray(dy, np.float64)[keep])
    return dx


def argmax_labels(x, classes):
    """index of the first maximum over x[..., :classes]"""
    return np.argmax(np.asarray(x)[..., :classes], axis=-1).astype(np.uint8)


def pad3to4(x):
    return np.concatenate([x, np.zeros(x.shape[:-1] + (1,), x.dtype)], axis=-1)


def gather(src, idx):
    return np.where(idx >= 0, src[np.maximum(idx, 0)], 0).astype(src.dtype)


def scatter(src, idx, dst, accumulate):
    """dst[idx[i]] (+)= src[i] for idx[i] >= 0, idx injective on those; every other target keeps what it held (compared as bits by the caller)"""
    used = idx[idx >= 0]
    assert len(np.unique(used)) == len(used)
    out = np.array(dst)
    out[used] = (dst[used] + src[idx >= 0]) if accumulate else src[idx >= 0]
    return out


def axpby(a, alpha, b, beta):
    pa = np.float64(alpha) * np.asarray(a, np.float64)
    pb = np.float64(beta) * np.asarray(b, np.float64) if b is not None else np.zeros_like(pa)
    return SimpleNamespace(out=pa + pb, S=np.abs(pa) + np.abs(pb), n=np.full(pa.shape, 2))
