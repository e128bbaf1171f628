"""Pillow's antialiased 8-bit resize (Resample.c, 8 bits per channel) and the app's min-max rule, stated as plain loops: the definition the
package's vectorised host form (ullsam_amd.utils.imageprep) and its kernels (csrc/imageprep.hip) are tested against.  Nothing here imports
the package.  DESIGN.md "7b, continued (image preprocessing)" has the same definition in words.

Per axis, in float64: scale = in / out, fs = max(scale, 1), support = support0 * fs, ksize = ceil(support) * 2 + 1; for output index xx:
center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in), n = xmax - xmin,
w[x] = f((x + xmin - center + 0.5) * (1 / fs)), normalised by their sum taken in index order, k[x] = int(w[x] * 2**22 +- 0.5) (truncating);
out = clamp((2**21 + sum src[xmin + x] * k[x]) >> 22, 0, 255).  Horizontal first, rounded to uint8, then vertical; a pass with out == in is skipped.
"""
import math

import numpy as np

BITS = 22
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}
PIL_FILTER = {"bilinear": 2, "bicubic": 3}          # PIL.Image.Resampling values

# (h, w) -> (oh, ow)
SHAPES = [
    ((37, 53), (16, 16)),
    ((64, 64), (32, 32)),
    ((50, 31), (64, 64)),       # upscale, taps clipped at both edges
    ((129, 257), (32, 64)),     # get_preprocess_shape(129, 257, 64)
    ((17, 1), (5, 9)),          # one-pixel-wide source
    ((300, 200), (64, 43)),
    ((64, 64), (64, 20)),       # vertical pass skipped
    ((64, 64), (64, 64)),       # both passes skipped
    ((2, 3), (7, 5)),
    ((100, 100), (1, 1)),       # 101 taps
    ((65, 63), (33, 31)),       # odd sizes around any block width
]
CHANNELS = (1, 3, 4)
FILTERS = ("bilinear", "bicubic")
LAYOUTS = ("interleaved", "planar")
# every (index of SHAPES, C, filter); the device tests cross these with LAYOUTS
CASES = [(i, c, f) for i in range(len(SHAPES)) for c in CHANNELS for f in FILTERS]
PREPROCESS_CASE = ((45, 70, 3), 32)                 # uint8 [45, 70, 3] -> padded to 70 x 70 -> 32 x 32 -> float32 [1, 3, 32, 32]


def case_id(case):
    i, c, f = case
    (h, w), (oh, ow) = SHAPES[i]
    return f"{h}x{w}-{oh}x{ow}-c{c}-{f}"


def make_image(h, w, c, seed=0):
    """Seeded random uint8 [h, w, c]; the top half is forced to 0 or 255 per pixel, so bicubic overshoot reaches the clamp on both sides."""
    rng = np.random.default_rng(1000 * seed + 100 * h + 10 * w + c)
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if h // 2:
        img[: h // 2] = np.where(rng.random((h // 2, w, 1)) < 0.5, 0, 255).astype(np.uint8)
    return img


def case_image(case):
    i, c, _ = case
    (h, w), _ = SHAPES[i]
    return make_image(h, w, c, seed=i)


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_F = {"bilinear": _bilinear, "bicubic": _bicubic}


def coeffs(in_size, out_size, filt):
    """-> (list of (xmin, n), list of n integer coefficients) per output index."""
    f = _F[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ss = 1.0 / fs
    bounds, ks = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        ks.append([int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5) for v in w])
        bounds.append((xmin, n))
    return bounds, ks


def _pass_axis1(img, out_size, filt):
    h, w, c = img.shape
    if out_size == w:
        return img
    bounds, ks = coeffs(w, out_size, filt)
    out = np.empty((h, out_size, c), np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = np.full((h, c), 1 << (BITS - 1), np.int64)
        for x in range(n):
            acc += img[:, xmin + x, :].astype(np.int64) * ks[xx][x]
        assert np.abs(acc).max() < 2 ** 31
        out[:, xx, :] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(img, out_hw, filt="bilinear"):
    """uint8 [H, W, C] -> uint8 [OH, OW, C]."""
    t = _pass_axis1(img, out_hw[1], filt)
    return np.ascontiguousarray(_pass_axis1(t.transpose(1, 0, 2), out_hw[0], filt).transpose(1, 0, 2))


def pad_to_square(img):
    """The app's centred zero pad (app.py:111-143)."""
    h, w = img.shape[:2]
    size = max(h, w)
    top, left = (size - h) // 2, (size - w) // 2
    return np.pad(img, ((top, size - h - top), (left, size - w - left), (0, 0)))


def minmax_u8(a):
    """app.py:191 as numpy evaluates it."""
    return ((a - a.min()) / (a.max() - a.min() + 1e-8) * 255).astype(np.uint8)


def to_uint8_inputs():
    """name -> array: the inputs of the to_uint8 / normalize_to_u8 tests."""
    rng = np.random.default_rng(7)
    return {
        "u16_range1": rng.integers(1000, 1002, (33, 47), dtype=np.uint16),
        "u16_range65535": np.concatenate([np.array([0, 65535], np.uint16), rng.integers(0, 65536, 1502, dtype=np.uint16)]).reshape(32, 47),
        "u16_constant": np.full((9, 11), 777, np.uint16),
        "f32_negative": (rng.standard_normal((41, 29)) * 37.5).astype(np.float32),
        "f32_unit": rng.random((35, 18, 3), dtype=np.float32),
    }
