"""The interactive loop's display tail on the host: what ops.click_finish (csrc/interactive.hip) computes, as vectorised numpy written from the
same definitions (DESIGN.md "7b, continued: the interactive loop").  It is what the kernel is tested against and what a CPU caller gets.
Also the app's palette (app.py:84-95), the blend tables of its overlay (app.py:748-772) and its click-coordinate mapping (app.py:536-537).
"""
from __future__ import annotations

import colorsys

import numpy as np

from .amg import nearest_source_index

INSTANCE_ALPHA = 0.5                 # app.py:758
CURRENT_ALPHA = 0.7                  # app.py:768
CURRENT_COLOR = (0, 255, 0)          # app.py:767


def default_palette(n: int = 64) -> np.ndarray:
    """generate_colors(64) (app.py:84-95): uint8 [n, 3], hue i / n at saturation 0.8 and value 0.9, each channel int(c * 255)."""
    return np.array([[int(c * 255) for c in colorsys.hsv_to_rgb(i / n, 0.8, 0.9)] for i in range(n)], np.uint8)


def _blend_table(colour, alpha: float) -> np.ndarray:
    v = np.arange(256, dtype=np.uint8)
    return np.stack([((1 - alpha) * v + alpha * np.array(colour)[k]).astype(np.uint8) for k in range(3)])


def blend_luts(palette=None):
    """The overlay's two blends over the 256 byte values, by the app's own expression ((1 - a) * v + a * colour).astype(np.uint8) in float64
    (app.py:759-762, 769-772): (lut_inst uint8 [K, 3, 256] at a = 0.5, lut_cur uint8 [3, 256] at a = 0.7 towards (0, 255, 0))."""
    pal = default_palette() if palette is None else np.asarray(palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError(f"palette must be uint8 [K, 3] with K >= 1, got {pal.dtype} {pal.shape}")
    lut_inst = np.stack([_blend_table(pal[i].astype(np.int64), INSTANCE_ALPHA) for i in range(pal.shape[0])])
    return np.ascontiguousarray(lut_inst), np.ascontiguousarray(_blend_table(CURRENT_COLOR, CURRENT_ALPHA))


def frame_coords(xy, frame: int, side: int, top: int = 0, left: int = 0) -> np.ndarray:
    """Display-pixel coordinates [..., 2] (x, y) -> model-frame coordinates, as the app maps a click (app.py:536-537) extended by the centred pad:
    x' = int((x + left) * frame / side), y' = int((y + top) * frame / side) in Python floats, truncated by int().  float32 [..., 2]."""
    a = np.asarray(xy, dtype=np.float64)
    out = np.empty(a.shape, np.float32)
    flat_in, flat_out = a.reshape(-1, 2), out.reshape(-1, 2)
    for i in range(flat_in.shape[0]):
        flat_out[i, 0] = int((float(flat_in[i, 0]) + left) * frame / side)
        flat_out[i, 1] = int((float(flat_in[i, 1]) + top) * frame / side)
    return out


def _taps(src: np.ndarray, n_in: int, n_out: int):
    """tap_of (csrc/common.h) for output indices src of an n_in -> n_out resize, align_corners=False, in float32 with its rounding order."""
    scale = np.float32(n_in) / np.float32(n_out)
    f = (src.astype(np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    f = np.maximum(f, np.float32(0))
    i0 = np.minimum(f.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (f - i0.astype(np.float32)).astype(np.float32)


def _lerp(a, b, l):
    """lerp_rn (csrc/common.h): a (1 - l) + b l, two products and a sum, each rounded to float32 once."""
    return (a * (np.float32(1) - l) + b * l).astype(np.float32)


def click_finish_host(low, frame: int, hw, side=None, top: int = 0, left: int = 0, thr: float = 0.0, image=None, canvas=None, first_id: int = 1,
                      paint: bool = False, highlight: bool = False, lut_inst=None, lut_cur=None, want_overlay: bool = False):
    """ops.click_finish on numpy arrays: low float32 [P, LH, LW] -> (mask uint8 [P, H, W], overlay uint8 [H, W, 3] or None, stats int32 [P, 5]).
    canvas int32 [H, W] is updated in place when paint is set."""
    low = np.ascontiguousarray(low, dtype=np.float32)
    if low.ndim != 3 or low.shape[0] < 1:
        raise ValueError(f"low must be float32 [P, LH, LW] with P >= 1, got {low.shape}")
    P, LH, LW = low.shape
    H, W = (int(v) for v in hw)
    S = int(frame)
    side = max(H, W) if side is None else int(side)
    top, left = int(top), int(left)
    if min(H, W, S, side) < 1 or top < 0 or left < 0 or top + H > side or left + W > side:
        raise ValueError(f"the window {(top, left, H, W)} must lie inside the square of side {side}")
    if paint and canvas is None:
        raise ValueError("paint needs a canvas")
    fy = nearest_source_index(side, S)[top:top + H]
    fx = nearest_source_index(side, S)[left:left + W]
    y0, y1, ly = _taps(fy, LH, S)
    x0, x1, lx = _taps(fx, LW, S)
    lx, ly = lx[None, None, :], ly[None, :, None]
    rows0, rows1 = low[:, y0, :], low[:, y1, :]
    v = _lerp(_lerp(rows0[:, :, x0], rows0[:, :, x1], lx), _lerp(rows1[:, :, x0], rows1[:, :, x1], lx), ly)
    m = v > np.float32(thr)
    ids = np.zeros((H, W), np.int32) if canvas is None else canvas
    if paint:
        for p in range(P):
            ids[m[p]] = first_id + p
    overlay = None
    if want_overlay:
        if image is None or lut_inst is None or lut_cur is None:
            raise ValueError("an overlay needs image, lut_inst and lut_cur")
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.shape != (H, W, 3):
            raise ValueError(f"image must be uint8 {(H, W, 3)}, got {img.dtype} {img.shape}")
        K = lut_inst.shape[0]
        ch = np.arange(3)[None, None, :]
        sel = (np.maximum(ids, 1) - 1) % K
        overlay = np.where((ids > 0)[:, :, None], lut_inst[sel[:, :, None], ch, img], img)
        if highlight:
            overlay = np.where(m[P - 1][:, :, None], lut_cur[ch, overlay], overlay)
        overlay = np.ascontiguousarray(overlay, dtype=np.uint8)
    stats = np.zeros((P, 5), np.int32)
    for p in range(P):
        ys, xs = np.nonzero(m[p])
        if ys.size:
            stats[p] = (ys.size, xs.min(), ys.min(), xs.max(), ys.max())
    return m.astype(np.uint8), overlay, stats
