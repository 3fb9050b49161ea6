"""NumPy / SciPy restatements of the input-pipeline ops with given parameters, used only by the tests (test_gpu_augment.py).  Borders are
OpenCV's as imgaug 0.4.0 calls it: reflect-101 (scipy's "mirror") for filter2D / blur / GaussianBlur / bilateralFilter, replicate
(scipy's "nearest") for medianBlur."""
import numpy as np
from scipy import ndimage


def apply_lut(img, lut):
    """img uint8 [h, w, 3], lut [3, 256]"""
    return np.stack([lut[c][img[..., c]] for c in range(3)], axis=-1)


def linear_blur(img, taps):
    """correlation with a k x k kernel anchored at k // 2 (also for even k), rounded half to even and clipped"""
    out = np.stack([ndimage.correlate(img[..., c].astype(np.float64), taps.astype(np.float64), mode="mirror") for c in range(3)], axis=-1)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def median_blur(img, k):
    return np.stack([ndimage.median_filter(img[..., c], size=k, mode="nearest") for c in range(3)], axis=-1)


def bilateral(img, radius, sigma_color, sigma_space):
    """OpenCV's bilateralFilter on 3 channels: taps within the disc of `radius`, weight exp(-r^2 / 2 ss^2) exp(-d^2 / 2 sc^2), d = sum of the
    absolute channel differences"""
    h, w, _ = img.shape
    src = np.pad(img.astype(np.float64), ((radius, radius), (radius, radius), (0, 0)), mode="reflect")
    acc, wsum = np.zeros((h, w, 3)), np.zeros((h, w, 1))
    center = img.astype(np.float64)
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            r = np.sqrt(i * i + j * j)
            if r > radius:
                continue
            p = src[radius + j:radius + j + h, radius + i:radius + i + w]
            d = np.abs(p - center).sum(-1, keepdims=True)
            wt = np.exp(-r * r / (2 * sigma_space ** 2)) * np.exp(-d * d / (2 * sigma_color ** 2))
            acc += wt * p
            wsum += wt
    return np.clip(np.rint(acc / wsum), 0, 255).astype(np.uint8)


def hue_saturation(img, dh, ds):
    """OpenCV 8-bit RGB -> HSV (hue 0..179, 12-bit fixed-point divisions), h = (h + dh) mod 180, s = clip(s + ds), float HSV -> RGB, rounded"""
    rgb = img.astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v, vmin = rgb.max(-1), rgb.min(-1)
    diff = v - vmin
    sdiv = np.where(v > 0, np.rint((255 << 12) / np.maximum(v, 1)), 0).astype(np.int64)
    hdiv = np.where(diff > 0, np.rint((180 << 12) / (6.0 * np.maximum(diff, 1))), 0).astype(np.int64)
    s = (diff * sdiv + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    h = np.mod(h + dh, 180)
    s = np.clip(s + ds, 0, 255)
    fh, fs, fv = (h * (6.0 / 180.0)).astype(np.float32), (s / 255.0).astype(np.float32), (v / 255.0).astype(np.float32)
    fh = np.where(fh >= 6, fh - 6, fh)
    sector = np.floor(fh).astype(np.int64)
    f = fh - sector
    tab = np.stack([fv, fv * (1 - fs), fv * (1 - fs * f), fv * (1 - fs * (1 - f))], axis=-1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    idx = sd[sector % 6]
    fb, fg, fr = [np.take_along_axis(tab, idx[..., k:k + 1], -1)[..., 0] for k in range(3)]
    out = np.stack([fr, fg, fb], -1)
    out = np.where((fs == 0)[..., None], fv[..., None], out)
    return np.clip(np.rint(out * 255), 0, 255).astype(np.uint8)
