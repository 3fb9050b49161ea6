"""The imgaug colour sequence of the reference (`seq`, casapose/data_handler/augmentation_model.py:43-110) restated as per-image parameter
draws, and the packing of one image's draws into the `cp_aug_image` program of the input-pipeline kernels (csrc/augment.hip).

These are RESTATEMENTS of imgaug 0.4.0 / OpenCV behaviour written from their documented algorithms; imgaug is not a dependency of this
project and nothing here has been checked against the library.  The distributions (group structure, ranges, per-channel and
Sometimes / SomeOf / OneOf rates) are imgaug's; the random stream is this project's (NumPy's default_rng, see below).  Faithful also means
keeping the oddities: Gaussian / Laplace noise with scale <= 0.05 intensity levels almost never moves a uint8 pixel, and that is what the
reference's sequence asks for.

Sequence (`random_order=True`: the five groups are permuted once per BATCH, from default_rng([seed, 3, epoch, batch]))
  0 blur        SomeOf((0, 2)) of GaussianBlur sigma U(0, 2), AverageBlur k [3, 7], MedianBlur k [3, 7], BilateralBlur d [1, 7], MotionBlur k [3, 7]
  1 colour      Sometimes(0.5, AddToHueAndSaturation((-15, 15)))
  2 brightness  OneOf(Add + Multiply, Add, Multiply, FrequencyNoiseAlpha(exponent (-4, 0), first=Multiply, second=ContrastNormalization))
  3 contrast    SomeOf((0, 2)) of GammaContrast, SigmoidContrast, LogContrast, LinearContrast
  4 arithmetic  SomeOf((0, 3)) of AdditiveGaussianNoise, AdditiveLaplaceNoise, AdditivePoissonNoise, Dropout, ImpulseNoise, SaltAndPepper,
                Salt, Pepper
SomeOf draws its count uniformly from {lo..hi}, then that many distinct children, applied in the listed order.  `per_channel=0.5`: with
probability 1/2 per image the op draws one value per channel, else one value shared by the channels.  Every per-image draw of image i in
epoch e comes from default_rng([seed, 2, e, i]) after the geometric draws of VectorfieldDataset, so a batch does not depend on the number of
replicas or on the shard that reads it.  Per-pixel randomness (noise, dropout, salt / pepper) is Philox4x32-10 on the device, keyed by a
64-bit seed drawn last from the same generator, counter (op slot, pixel, channel).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np

from .. import _lib

GROUPS = ("blur", "colour", "brightness", "contrast", "arithmetic")
_ARANGE = np.arange(256, dtype=np.float64)


class Op:
    """One op of a program: kind (_lib.AUG_*), per_channel, k, i0 / i1 / f0 / f1 as documented in include/casapose_hip.h, plus the host-built
    tables: lut [3][256] uint8 (AUG_LUT), luts (two of them, AUG_FREQ_BLEND), taps [k][k] float32 (AUG_BLUR_LINEAR)."""

    def __init__(self, kind, name, per_channel=0, k=0, i0=0, i1=0, f0=0.0, f1=0.0, lut=None, luts=None, taps=None):
        self.kind, self.name, self.per_channel, self.k, self.i0, self.i1, self.f0, self.f1 = kind, name, int(per_channel), int(k), int(i0), int(i1), \
            float(f0), float(f1)
        self.lut, self.luts, self.taps = lut, luts, taps

    def __repr__(self):
        return "Op(%s, pc=%d, k=%d, i=(%d, %d), f=(%.4g, %.4g))" % (self.name, self.per_channel, self.k, self.i0, self.i1, self.f0, self.f1)


# ------------------------------------------------------------------------------------------------------------------------------------
# lookup tables (uint8 in -> uint8 out, per channel)
def lut_add(v) -> np.ndarray:
    """Add: out = clip(x + v, 0, 255) with an integer v (imgaug samples Add's value from the discrete interval)."""
    return np.clip(_ARANGE[None, :] + np.asarray(v, np.float64).reshape(-1, 1), 0, 255).astype(np.uint8)


def lut_multiply(m) -> np.ndarray:
    """Multiply: out = clip(round(x * m), 0, 255) (round half to even, NumPy's)."""
    return np.clip(np.round(_ARANGE[None, :] * np.asarray(m, np.float64).reshape(-1, 1)), 0, 255).astype(np.uint8)


def lut_gamma(g) -> np.ndarray:
    """GammaContrast: out = trunc(255 * (x / 255) ** gamma) (imgaug builds the table in float32 and casts with astype)."""
    g = np.asarray(g, np.float32).reshape(-1, 1)
    t = (np.linspace(0, 1.0, 256, dtype=np.float32)[None, :] ** g) * np.float32(255)
    return np.clip(t, 0, 255).astype(np.uint8)


def lut_sigmoid(gain, cutoff) -> np.ndarray:
    """SigmoidContrast: out = trunc(255 / (1 + exp(gain * (cutoff - x / 255))))."""
    gain, cutoff = np.asarray(gain, np.float32).reshape(-1, 1), np.asarray(cutoff, np.float32).reshape(-1, 1)
    x = np.linspace(0, 1.0, 256, dtype=np.float32)[None, :]
    t = np.float32(255) / (1 + np.exp(gain * (cutoff - x)))
    return np.clip(t, 0, 255).astype(np.uint8)


def lut_log(gain) -> np.ndarray:
    """LogContrast: out = trunc(255 * gain * log2(1 + x / 255))."""
    gain = np.asarray(gain, np.float32).reshape(-1, 1)
    t = gain * np.log2(1 + np.linspace(0, 1.0, 256, dtype=np.float32)[None, :]) * np.float32(255)
    return np.clip(t, 0, 255).astype(np.uint8)


def lut_linear(alpha) -> np.ndarray:
    """LinearContrast / ContrastNormalization: out = trunc(127.5 + alpha * (x - 127.5)) (127.5 = the centre of uint8's value range)."""
    alpha = np.asarray(alpha, np.float32).reshape(-1, 1)
    t = np.float32(127.5) + alpha * (np.arange(256, dtype=np.float32)[None, :] - np.float32(127.5))
    return np.clip(t, 0, 255).astype(np.uint8)


def _three(lut: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.broadcast_to(lut, (3, 256)), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------------
# blur kernels
def gaussian_ksize(sigma: float) -> int:
    """imgaug's kernel size for cv2.GaussianBlur: 3.3 sigma below sigma 3 (2.9 below 5, else 2.6), at least 5, made odd -> 5 or 7 here."""
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = int(max(k, 5))
    return k + 1 if k % 2 == 0 else k


def gaussian_taps(sigma: float) -> np.ndarray:
    """cv2.getGaussianKernel(k, sigma) outer itself: g_i = exp(-(i - (k-1)/2)^2 / (2 sigma^2)), normalised to sum 1."""
    k = gaussian_ksize(sigma)
    g = np.exp(-((np.arange(k) - (k - 1) / 2.0) ** 2) / (2.0 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g).astype(np.float32)


def motion_taps(k: int, angle: float, direction: float) -> np.ndarray:
    """MotionBlur's kernel: k made odd; a vertical line through the centre column with weights linspace(d, 1 - d, k), d = (direction + 1) / 2;
    rotated by `angle` degrees about the kernel centre (bilinear, as uint8 x 255 then / 255, as imgaug's Affine does); normalised to sum 1."""
    k = k + 1 if k % 2 == 0 else k
    d = (float(np.clip(direction, -1.0, 1.0)) + 1.0) / 2.0
    m = np.zeros((k, k), np.float64)
    m[:, k // 2] = np.linspace(d, 1.0 - d, num=k)
    m8 = (m * 255).astype(np.uint8).astype(np.float64)
    c = (k - 1) / 2.0
    a, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    yy, xx = np.mgrid[0:k, 0:k].astype(np.float64)
    # output -> input: rotate the output pixel back about the centre
    xs = a * (xx - c) - s * (yy - c) + c
    ys = s * (xx - c) + a * (yy - c) + c
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    fx, fy = xs - x0, ys - y0

    def at(y, x):
        ok = (y >= 0) & (y < k) & (x >= 0) & (x < k)
        return np.where(ok, m8[np.clip(y, 0, k - 1), np.clip(x, 0, k - 1)], 0.0)

    r = (at(y0, x0) * (1 - fx) * (1 - fy) + at(y0, x0 + 1) * fx * (1 - fy) + at(y0 + 1, x0) * (1 - fx) * fy + at(y0 + 1, x0 + 1) * fx * fy)
    r = np.round(r).astype(np.uint8) / 255.0
    if r.sum() <= 0:
        r = m
    return (r / r.sum()).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# FrequencyNoise (the mask of FrequencyNoiseAlpha)
def frequency_noise_field(rng: np.random.Generator, h: int, w: int, exponent: float, size_px_max: int) -> np.ndarray:
    """imgaug's FrequencyNoise recipe at the small size: the field is (h, w) scaled so that its longer side is size_px_max (if the image is
    larger); random magnitudes U(0,1) times distance-from-DC ** exponent (DC removed) and random phases U(0, 2 pi); the real part of the
    inverse FFT, normalised to [0, 1]."""
    maxlen = max(h, w)
    if maxlen > size_px_max:
        hs, ws = max(int(h * size_px_max / maxlen), 1), max(int(w * size_px_max / maxlen), 1)
    else:
        hs, ws = h, w
    hs, ws = min(hs, _lib.AUG_NOISE_MAX), min(ws, _lib.AUG_NOISE_MAX)
    mag = rng.random((hs, ws))
    phase = rng.random((hs, ws)) * 2 * np.pi
    fy = np.minimum(np.arange(hs), hs - np.arange(hs)).astype(np.float64)
    fx = np.minimum(np.arange(ws), ws - np.arange(ws)).astype(np.float64)
    dist = np.sqrt(fy[:, None] ** 2 + fx[None, :] ** 2)
    dist[0, 0] = 1.0
    mag = mag * dist ** exponent
    mag[0, 0] = 0.0
    field = np.fft.ifft2(mag * np.exp(1j * phase)).real
    lo, hi = field.min(), field.max()
    field = (field - lo) / (hi - lo) if hi > lo else np.full_like(field, 0.5)
    return field.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
class ImageProgram:
    """The draws of one image: the op list in application order, and the FrequencyNoiseAlpha mask (fields + aggregation)."""

    def __init__(self):
        self.ops: List[Op] = []
        self.noise_fields: List[np.ndarray] = []
        self.noise_up: List[int] = []
        self.noise_aggregate = 0
        self.noise_sigmoid = 0
        self.noise_threshold = 0.0


def group_order(seed: int, epoch: int, batch: int) -> np.ndarray:
    """random_order=True of `seq`: the permutation of the five groups, one per batch."""
    return np.random.default_rng([int(seed), 3, int(epoch), int(batch)]).permutation(len(GROUPS))


def _per_channel_values(rng, draw):
    """per_channel=0.5: returns (per_channel flag, values [3])."""
    pc = rng.random() < 0.5
    v = draw(3) if pc else np.repeat(draw(1), 3)
    return int(pc), np.asarray(v)


def _some_of(rng, n_children: int, hi: int) -> List[int]:
    n = int(rng.integers(0, hi + 1))
    return sorted(rng.choice(n_children, size=n, replace=False).tolist()) if n else []


def sample_blur(rng, prog: ImageProgram):
    for c in _some_of(rng, 5, 2):
        if c == 0:   # GaussianBlur((0, 2)): skipped below sigma 1e-3 (imgaug's eps)
            sigma = float(rng.uniform(0.0, 2.0))
            if sigma >= 1e-3:
                t = gaussian_taps(sigma)
                prog.ops.append(Op(_lib.AUG_BLUR_LINEAR, "gaussian_blur", k=len(t), f0=sigma, taps=t))
        elif c == 1:   # AverageBlur(k=(3, 7)): cv2.blur with a k x k box, anchor k // 2 (also for even k)
            k = int(rng.integers(3, 8))
            prog.ops.append(Op(_lib.AUG_BLUR_LINEAR, "average_blur", k=k, taps=np.full((k, k), 1.0 / (k * k), np.float32)))
        elif c == 2:   # MedianBlur(k=(3, 7)): even k -> k + 1
            k = int(rng.integers(3, 8))
            prog.ops.append(Op(_lib.AUG_BLUR_MEDIAN, "median_blur", k=k + 1 if k % 2 == 0 else k))
        elif c == 3:   # BilateralBlur(d=(1, 7)), sigma_color = sigma_space = U(10, 250): OpenCV's radius max(d // 2, 1)
            d = int(rng.integers(1, 8))
            sc, ss = float(rng.uniform(10, 250)), float(rng.uniform(10, 250))
            prog.ops.append(Op(_lib.AUG_BLUR_BILATERAL, "bilateral_blur", k=max(d // 2, 1), i0=d, f0=sc, f1=ss))
        else:   # MotionBlur(k=(3, 7)), angle U(0, 360), direction U(-1, 1)
            k = int(rng.integers(3, 8))
            t = motion_taps(k, float(rng.uniform(0, 360)), float(rng.uniform(-1, 1)))
            prog.ops.append(Op(_lib.AUG_BLUR_LINEAR, "motion_blur", k=len(t), taps=t))


def sample_colour(rng, prog: ImageProgram):
    """Sometimes(0.5, AddToHueAndSaturation((-15, 15))): one integer v; saturation += v (clipped), hue (OpenCV's 0..179) += trunc(v * 180 / 255)
    modulo 180 -- imgaug projects its -255..255 hue value onto OpenCV's hue range."""
    if rng.random() < 0.5:
        v = int(rng.integers(-15, 16))
        prog.ops.append(Op(_lib.AUG_HUE_SAT, "add_to_hue_and_saturation", i0=int(v * 180 / 255), i1=v))


def _add(rng):
    pc, v = _per_channel_values(rng, lambda n: rng.integers(-10, 11, n))
    return Op(_lib.AUG_LUT, "add", per_channel=pc, lut=_three(lut_add(v)))


def _multiply(rng):
    pc, m = _per_channel_values(rng, lambda n: rng.uniform(0.75, 1.25, n))
    return Op(_lib.AUG_LUT, "multiply", per_channel=pc, lut=_three(lut_multiply(m)))


def sample_brightness(rng, prog: ImageProgram, h: int, w: int):
    choice = int(rng.integers(0, 4))
    if choice == 0:
        prog.ops += [_add(rng), _multiply(rng)]
    elif choice == 1:
        prog.ops.append(_add(rng))
    elif choice == 2:
        prog.ops.append(_multiply(rng))
    else:
        # FrequencyNoiseAlpha: mask a = aggregate over 1..3 iterations of a FrequencyNoise field (exponent U(-4, 0), size_px_max [4, 16],
        # upscaled to the crop with nearest / linear / cubic, p = 0.05 / 0.6 / 0.35) by max or average; then, with p 0.5, a sigmoid
        # 1 / (1 + exp(-(20 a - 10 - t))) with t ~ N(0, 5).  out = round(a * first(x) + (1 - a) * second(x)).
        first = _multiply(rng)
        pc, alpha = _per_channel_values(rng, lambda n: rng.uniform(0.7, 1.3, n))
        second = _three(lut_linear(alpha))
        iterations = int(rng.integers(1, 4))
        prog.noise_aggregate = int(rng.integers(0, 2))
        for _ in range(iterations):
            size_px_max = int(rng.integers(4, 17))
            exponent = float(rng.uniform(-4, 0))
            prog.noise_up.append(int(rng.choice(3, p=[0.05, 0.6, 0.35])))
            prog.noise_fields.append(frequency_noise_field(rng, h, w, exponent, size_px_max))
        if rng.random() < 0.5:
            prog.noise_sigmoid, prog.noise_threshold = 1, float(rng.normal(0.0, 5.0))
        prog.ops.append(Op(_lib.AUG_FREQ_BLEND, "frequency_noise_alpha", per_channel=pc, luts=(first.lut, second)))


def sample_contrast(rng, prog: ImageProgram):
    for c in _some_of(rng, 4, 2):
        if c == 0:   # GammaContrast((0.75, 1.25))
            pc, g = _per_channel_values(rng, lambda n: rng.uniform(0.75, 1.25, n))
            prog.ops.append(Op(_lib.AUG_LUT, "gamma_contrast", per_channel=pc, lut=_three(lut_gamma(g))))
        elif c == 1:   # SigmoidContrast(gain=(5, 10), cutoff=(0.25, 0.75))
            pc = int(rng.random() < 0.5)
            n = 3 if pc else 1
            gain, cutoff = rng.uniform(5, 10, n), rng.uniform(0.25, 0.75, n)
            prog.ops.append(Op(_lib.AUG_LUT, "sigmoid_contrast", per_channel=pc, lut=_three(lut_sigmoid(gain, cutoff))))
        elif c == 2:   # LogContrast(gain=(0.75, 1))
            pc, g = _per_channel_values(rng, lambda n: rng.uniform(0.75, 1.0, n))
            prog.ops.append(Op(_lib.AUG_LUT, "log_contrast", per_channel=pc, lut=_three(lut_log(g))))
        else:   # LinearContrast(alpha=(0.7, 1.3))
            pc, a = _per_channel_values(rng, lambda n: rng.uniform(0.7, 1.3, n))
            prog.ops.append(Op(_lib.AUG_LUT, "linear_contrast", per_channel=pc, lut=_three(lut_linear(a))))


def sample_arithmetic(rng, prog: ImageProgram):
    """Per pixel (Philox on the device): Gaussian N(0, s) / Laplace(0, s) noise with s U(0, 0.05), rounded; Poisson(lambda U(0, 8)) with a random
    sign; Dropout: 0 with probability p; ImpulseNoise (per channel), SaltAndPepper, Salt, Pepper: with probability p the value is replaced by
    round(255 r), r ~ Beta(0.5, 0.5) (both), 0.5 + |r - 0.5| (salt) or 0.5 - |r - 0.5| (pepper); p U(0, 0.05) for all of them."""
    for c in _some_of(rng, 8, 3):
        if c == 0:
            pc = int(rng.random() < 0.5)
            prog.ops.append(Op(_lib.AUG_GAUSS_NOISE, "additive_gaussian_noise", per_channel=pc, f0=rng.uniform(0, 0.05)))
        elif c == 1:
            pc = int(rng.random() < 0.5)
            prog.ops.append(Op(_lib.AUG_LAPLACE_NOISE, "additive_laplace_noise", per_channel=pc, f0=rng.uniform(0, 0.05)))
        elif c == 2:
            pc = int(rng.random() < 0.5)
            prog.ops.append(Op(_lib.AUG_POISSON_NOISE, "additive_poisson_noise", per_channel=pc, f0=rng.uniform(0, 8)))
        elif c == 3:
            pc = int(rng.random() < 0.5)
            prog.ops.append(Op(_lib.AUG_DROPOUT, "dropout", per_channel=pc, f0=rng.uniform(0, 0.05)))
        elif c == 4:
            prog.ops.append(Op(_lib.AUG_REPLACE, "impulse_noise", per_channel=1, i0=0, f0=rng.uniform(0, 0.05)))
        else:
            prog.ops.append(Op(_lib.AUG_REPLACE, ("salt_and_pepper", "salt", "pepper")[c - 5], per_channel=0, i0=c - 5, f0=rng.uniform(0, 0.05)))


def sample_program(rng: np.random.Generator, order: Sequence[int], h: int, w: int) -> ImageProgram:
    """The draws of one image for the five groups in `order` (group_order) on an h x w crop."""
    prog = ImageProgram()
    for g in order:
        g = int(g)
        if g == 0:
            sample_blur(rng, prog)
        elif g == 1:
            sample_colour(rng, prog)
        elif g == 2:
            sample_brightness(rng, prog, h, w)
        elif g == 3:
            sample_contrast(rng, prog)
        else:
            sample_arithmetic(rng, prog)
    return prog


# ------------------------------------------------------------------------------------------------------------------------------------
def pack_image(img: "_lib.AugImage", ops: Sequence[Op], prog: Optional[ImageProgram] = None) -> None:
    """Writes the op list (and the FrequencyNoise mask of `prog`) into the cp_aug_image `img`; Philox slot = op index."""
    if len(ops) > _lib.AUG_MAX_OPS:
        raise ValueError("%d ops exceed CP_AUG_MAX_OPS" % len(ops))
    blurs = [i for i, o in enumerate(ops) if o.kind >= _lib.AUG_BLUR_LINEAR]
    if len(blurs) > 2 or (blurs and blurs[-1] - blurs[0] != len(blurs) - 1):
        raise ValueError("at most two blurs, adjacent in the program")
    n_lut, n_taps = 0, 0
    for i, o in enumerate(ops):
        d = img.ops[i]
        d.kind, d.per_channel, d.slot, d.k, d.i0, d.i1, d.f0, d.f1 = o.kind, o.per_channel, i, o.k, o.i0, o.i1, o.f0, o.f1
        if o.kind == _lib.AUG_LUT or o.kind == _lib.AUG_FREQ_BLEND:
            tables = [o.lut] if o.kind == _lib.AUG_LUT else list(o.luts)
            if n_lut + len(tables) > _lib.AUG_MAX_LUTS:
                raise ValueError("more than CP_AUG_MAX_LUTS tables")
            for j, t in enumerate(tables):
                C.memmove(C.addressof(img.lut[n_lut + j]), np.ascontiguousarray(t, np.uint8).ctypes.data, 768)
            d.i0, d.i1 = n_lut, n_lut + len(tables) - 1
            n_lut += len(tables)
        if o.kind == _lib.AUG_BLUR_LINEAR:
            if o.k > 7:
                raise ValueError("linear blur wider than 7")
            t = np.ascontiguousarray(o.taps, np.float32).reshape(-1)
            C.memmove(C.addressof(img.taps[n_taps]), t.ctypes.data, 4 * t.size)
            d.i0 = n_taps
            n_taps += 1
        elif o.kind in (_lib.AUG_BLUR_MEDIAN, _lib.AUG_BLUR_BILATERAL) and (o.k > 7 if o.kind == _lib.AUG_BLUR_MEDIAN else o.k > 3):
            raise ValueError("blur wider than 7")
    img.n_ops = len(ops)
    if prog is not None and prog.noise_fields:
        img.noise_fields = len(prog.noise_fields)
        for f, (field, up) in enumerate(zip(prog.noise_fields, prog.noise_up)):
            hs, ws = field.shape
            img.noise_h[f], img.noise_w[f], img.noise_up[f] = hs, ws, up
            C.memmove(C.addressof(img.noise[f]), np.ascontiguousarray(field, np.float32).ctypes.data, 4 * field.size)
        img.noise_aggregate, img.noise_sigmoid, img.noise_threshold = prog.noise_aggregate, prog.noise_sigmoid, prog.noise_threshold
