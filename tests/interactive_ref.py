"""Plain-loop definitions of the interactive loop's display tail (ops.click_finish / utils.interactive.click_finish_host), written from the
reference's app.py, one display pixel at a time:

  frame pixel   export_mask's "Image.NEAREST to the padded size, then cut the pad off" (app.py:807-820; on a square image postprocess_mask,
                app.py:283-287): PIL's nearest rule src = floor((dst + 0.5) * n_in / n_out), in integers
  logit         F.interpolate(low, (S, S), mode="bilinear", align_corners=False) (app.py:635-640) at that frame pixel, in float32 with the
                rounding order of csrc/common.h tap_of / lerp_rn
  mask          sigmoid(x) > 0.5 (app.py:643-645) = x > 0; in general x > thr
  canvas        final_mask_state[mask] = instance_count (app.py:692-707), one mask after the other
  overlay       visualize_masks (app.py:748-772): the app's float64 expression per pixel -- NOT a table
  area, box     pixel count and XYXY box with inclusive maxima, zeros for an empty mask (amg.py:303-346 batched_mask_to_box)

`click_finish_loops` visits every pixel with scalar arithmetic (the small shapes); `click_finish_rows` is the same definition with one numpy row
per step (the 1024-sized shapes, where a scalar loop would take minutes); the CPU test holds the two equal on the small shapes.
"""
import numpy as np

F32 = np.float32


def frame_index(d: int, off: int, S: int, side: int) -> int:
    return min(((2 * (d + off) + 1) * S) // (2 * side), S - 1)


def tap(o, n_in: int, n_out: int):
    """Source taps of output index o (scalar or integer array) for an n_in -> n_out resize, align_corners=False, float32."""
    scale = F32(n_in) / F32(n_out)
    f = (np.asarray(o).astype(F32) + F32(0.5)) * scale - F32(0.5)
    f = np.where(f < F32(0), F32(0), f).astype(F32)
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (f - i0.astype(F32)).astype(F32)


def lerp(a, b, l):
    one_minus = F32(1) - l
    return F32(F32(a * one_minus) + F32(b * l)) if np.ndim(a) == 0 else ((a * one_minus).astype(F32) + (b * l).astype(F32)).astype(F32)


def bilinear_at(low2, fy: int, fx: int, S: int):
    LH, LW = low2.shape
    y0, y1, ly = tap(fy, LH, S)
    x0, x1, lx = tap(fx, LW, S)
    ly, lx = F32(ly), F32(lx)
    top = lerp(F32(low2[y0, x0]), F32(low2[y0, x1]), lx)
    bot = lerp(F32(low2[y1, x0]), F32(low2[y1, x1]), lx)
    return lerp(top, bot, ly)


def blend(rgb, colour, alpha):
    """app.py:759-762 / 769-772 on one pixel: ((1 - alpha) * overlay[mask] + alpha * np.array(color)).astype(np.uint8)."""
    return ((1 - alpha) * np.asarray(rgb, np.uint8) + alpha * np.array(colour)).astype(np.uint8)


def stats_of(masks):
    P = masks.shape[0]
    out = np.zeros((P, 5), np.int32)
    for p in range(P):
        area, x0, y0, x1, y1 = 0, None, None, None, None
        for y in range(masks.shape[1]):
            for x in np.flatnonzero(masks[p, y]):
                area += 1
                x0 = x if x0 is None else min(x0, x); x1 = x if x1 is None else max(x1, x)
                y0 = y if y0 is None else min(y0, y); y1 = y if y1 is None else max(y1, y)
        if area:
            out[p] = (area, x0, y0, x1, y1)
    return out


def click_finish_loops(low, S, hw, side, top, left, thr, image, canvas, first_id, paint, highlight, palette):
    """Returns (mask u8 [P, H, W], canvas i32 [H, W] (a copy), overlay u8 [H, W, 3] or None when image is None, stats i32 [P, 5])."""
    P = low.shape[0]
    H, W = hw
    K = len(palette)
    mask = np.zeros((P, H, W), np.uint8)
    ids = np.zeros((H, W), np.int32) if canvas is None else canvas.copy()
    overlay = None if image is None else image.copy()
    for y in range(H):
        fy = frame_index(y, top, S, side)
        for x in range(W):
            fx = frame_index(x, left, S, side)
            for p in range(P):
                mask[p, y, x] = bilinear_at(low[p], fy, fx, S) > F32(thr)
                if paint and mask[p, y, x]:
                    ids[y, x] = first_id + p
            if overlay is not None:
                if ids[y, x] > 0:
                    overlay[y, x] = blend(overlay[y, x], tuple(int(c) for c in palette[(ids[y, x] - 1) % K]), 0.5)
                if highlight and mask[P - 1, y, x]:
                    overlay[y, x] = blend(overlay[y, x], (0, 255, 0), 0.7)
    return mask, ids, overlay, stats_of(mask)


def click_finish_rows(low, S, hw, side, top, left, thr, image, canvas, first_id, paint, highlight, palette):
    """The same definition, one display row per step."""
    P, LH, LW = low.shape
    H, W = hw
    K = len(palette)
    mask = np.zeros((P, H, W), np.uint8)
    ids = np.zeros((H, W), np.int32) if canvas is None else canvas.copy()
    overlay = None if image is None else image.copy()
    fx = np.array([frame_index(x, left, S, side) for x in range(W)])
    x0, x1, lx = tap(fx, LW, S)
    for y in range(H):
        y0, y1, ly = tap(frame_index(y, top, S, side), LH, S)
        ly = F32(ly)
        for p in range(P):
            v = lerp(lerp(low[p, y0, x0], low[p, y0, x1], lx), lerp(low[p, y1, x0], low[p, y1, x1], lx), ly)
            mask[p, y] = v > F32(thr)
            if paint:
                ids[y, mask[p, y] > 0] = first_id + p
        if overlay is not None:
            for i in np.unique(ids[y]):
                if i > 0:
                    sel = ids[y] == i
                    overlay[y, sel] = ((1 - 0.5) * overlay[y, sel] + 0.5 * np.array(tuple(int(c) for c in palette[(i - 1) % K]))).astype(np.uint8)
            if highlight:
                sel = mask[P - 1, y] > 0
                overlay[y, sel] = ((1 - 0.7) * overlay[y, sel] + 0.7 * np.array((0, 255, 0))).astype(np.uint8)
    stats = np.zeros((P, 5), np.int32)
    for p in range(P):
        ys, xs = np.nonzero(mask[p])
        if ys.size:
            stats[p] = (ys.size, xs.min(), ys.min(), xs.max(), ys.max())
    return mask, ids, overlay, stats


# ---- the shapes and inputs the CPU and GPU tests share -------------------------------------------------------------------------------
# name -> (low side, frame S, display (H, W), side, top, left): the smallest shapes at which each index rule can go wrong
SHAPES = {
    "identity": (8, 32, (32, 32), 32, 0, 0),
    "down": (8, 32, (5, 7), 7, 1, 0),
    "up_beyond_frame": (16, 64, (61, 47), 61, 0, 7),
    "portrait_pad": (16, 64, (47, 61), 61, 7, 0),
    "degenerate": (16, 64, (1, 1), 1, 0, 0),
    "sam": (256, 1024, (1024, 1024), 1024, 0, 0),
    "off_size": (256, 1024, (1000, 1333), 1333, 166, 0),
}
SMALL = ("identity", "down", "up_beyond_frame", "portrait_pad", "degenerate")
FLAGS = ((False, False), (True, False), (False, True), (True, True))          # (paint, highlight)
TEST_PALETTE = np.array([[230, 46, 46], [46, 230, 92], [12, 0, 255], [255, 255, 255], [0, 0, 0], [7, 130, 201], [99, 98, 97]], np.uint8)


def _blob(rng, n, cy, cx, r):
    """Smooth logits, positive inside a disc of radius r * n around (cy, cx) * n, plus noise that roughens the zero crossing."""
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    d = np.hypot(yy - cy * n, xx - cx * n)
    return ((r * n - d) * (8.0 / n) + rng.normal(0, 0.3, (n, n))).astype(F32)


def lows(n: int, seed: int = 0):
    """name -> low f32 [P, n, n]: one mask; three overlapping masks whose middle one carries patches of exactly 0.0 and of +-1e-30; and
    (full, empty, blob) -- the last mask is the one a highlight shows."""
    rng = np.random.default_rng(seed + n)
    a, b, c = _blob(rng, n, 0.45, 0.40, 0.30), _blob(rng, n, 0.55, 0.55, 0.28), _blob(rng, n, 0.35, 0.60, 0.22)
    q = max(n // 8, 1)
    b[:q, :] = 0.0                         # exactly on the threshold: not in the mask
    b[-q:, :q] = F32(1e-30)                # just above it
    b[-q:, -q:] = F32(-1e-30)              # just below it
    b[n // 2, n // 2] = 0.0
    return {"p1": a[None].copy(), "p3": np.stack([a, b, c]), "p3_full_empty": np.stack([np.full((n, n), 5, F32), np.full((n, n), -5, F32), c])}


def display_inputs(hw, seed: int = 1):
    """(image u8 [H, W, 3], canvas i32 [H, W] with ids far beyond the palette's length and about a third background)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    canvas = rng.integers(0, 41, (H, W)).astype(np.int32) * (rng.random((H, W)) > 0.33)
    return image, canvas.astype(np.int32)
