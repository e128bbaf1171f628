"""Definitions for the mask-generation kernels of csrc/amg.hip (utils/amg.py), numpy and torch on the CPU, nothing from ullsam_amd.

  post64         Sam.postprocess_masks (sam.py:154-162) as float64 F.interpolate(mode="bilinear", align_corners=False) twice with the cut to
                 input_size in between: the MEANING of the fused launch's virtual logits
  post32         the same composition in float32 with the rounding order amg_postprocess_kernel declares (csrc/common.h tap_of / lerp_rn): the BITS
  expected       everything ullsam_amg_postprocess writes, from post32 plus the integer oracle (oracle/amg_oracle.py)
  change_words   the [ceil(FH/64), FW] uint64 words of the frame mask's column-major change positions, and the way back to runs
  nms_bits32     the upper-triangle suppression matrix of ullsam_nms_mask in float32, in the kernel's order of operations
  nms_bits_exact the same matrix in Python integers (integer boxes, rational threshold)

and the case tables and input builders that tests/test_amg_ref_cpu.py and tests/test_amg_kernels_gpu.py share.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import amg_oracle as AO
from tests.interactive_ref import F32, lerp, tap


# ---- the two resizes --------------------------------------------------------------------------------------------------------------
def _resize32(x, out_hw, clamp_hw):
    """One bilinear stage in float32 on [..., H, W]: x first, then y; taps clamped at clamp_hw (the valid part of x), each product and sum rounded once."""
    x0, x1, lx = tap(np.arange(out_hw[1]), clamp_hw[1], out_hw[1])
    y0, y1, ly = tap(np.arange(out_hw[0]), clamp_hw[0], out_hw[0])
    rows = lerp(x[..., :, x0], x[..., :, x1], lx)
    return lerp(rows[..., y0, :], rows[..., y1, :], ly[:, None])


def post32(low, S1, inp, crop_hw):
    """low f32 [M, LH, LW] -> f32 [M, CH, CW], bit for bit what amg_postprocess_kernel evaluates per pixel.  NaN and +-inf flow through as IEEE does."""
    low = np.ascontiguousarray(low, dtype=F32)
    with np.errstate(all="ignore"):
        up = _resize32(low, (S1, S1), low.shape[-2:])
        cut = up[..., :inp[0], :inp[1]]
        return _resize32(cut, crop_hw, inp)


def post64(low, S1, inp, crop_hw):
    """The meaning: float64 F.interpolate twice."""
    x = torch.from_numpy(np.ascontiguousarray(low, dtype=np.float64))[None]
    up = F.interpolate(x, (S1, S1), mode="bilinear", align_corners=False)[..., :inp[0], :inp[1]]
    return F.interpolate(up, tuple(crop_hw), mode="bilinear", align_corners=False)[0].numpy()


def band_of(low):
    """The kernel's own footprint margin, 1e-4 * max(1, max|low|), taken over the finite cells of the whole stack (an upper bound of every block's margin)."""
    fin = np.abs(low[np.isfinite(low)])
    return 1e-4 * max(1.0, float(fin.max()) if fin.size else 0.0)


def thresholds(thr, off):
    """(t, hi, lo) as the reference compares them: the double sum, rounded to float32 once."""
    return F32(thr), F32(float(thr) + float(off)), F32(float(thr) - float(off))


def thresholds_two_floats(thr, off):
    """(hi, lo) built from two float32 values, the deviation the entries had before they took doubles."""
    return F32(F32(thr) + F32(off)), F32(F32(thr) - F32(off))


# ---- change words ------------------------------------------------------------------------------------------------------------------
def change_words(frame_mask):
    """bool [M, FH, FW] -> uint64 [M, ceil(FH/64), FW]: bit i of words[yb][x] set iff t[f] != t[f+1] for f = x*FH + 64*yb + i in the
    column-major flattening t, never for the last f."""
    m = np.asarray(frame_mask).astype(bool)
    M, FH, FW = m.shape
    nyb = (FH + 63) // 64
    t = m.transpose(0, 2, 1).reshape(M, FW * FH)
    ch = np.zeros((M, FW * FH), bool)
    ch[:, :-1] = t[:, 1:] != t[:, :-1]
    pad = np.zeros((M, FW, nyb * 64), bool)
    pad[:, :, :FH] = ch.reshape(M, FW, FH)
    out = np.empty((M, nyb, FW), np.uint64)
    for i in range(M):                                             # (one mask at a time: the 64 shifted copies of a whole stack are large)
        bits = pad[i].reshape(FW, nyb, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
        out[i] = np.bitwise_or.reduce(bits, axis=-1).T
    return out


def words_to_positions(words, FH):
    """uint64 [nyb, FW] of ONE mask -> the ordered change positions f (int64)."""
    nyb, FW = words.shape
    bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    yb, x, i = np.nonzero(bits)
    return np.sort(x.astype(np.int64) * FH + yb.astype(np.int64) * 64 + i.astype(np.int64))


def positions_to_runs(pos, first, FH, FW):
    """Change positions + the first element -> the counts of the uncompressed RLE (they start with the 0-run)."""
    edges = np.concatenate([[0, 0] if first else [0], np.asarray(pos, np.int64) + 1, [FH * FW]])
    return (edges[1:] - edges[:-1]).tolist()


def runs_to_mask(counts, FH, FW):
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, np.asarray(counts, np.int64))
    return flat.reshape(FW, FH).transpose()


# ---- geometries and inputs ---------------------------------------------------------------------------------------------------------
# name -> (low (h, w), S1, input_size, crop_box [x0, y0, x1, y1], orig (h, w)): the smallest shapes that reach each branch of the fused launch
GEOMS = {
    "full_nc1": ((16, 16), 64, (64, 64), (0, 0, 70, 70), (70, 70)),            # one-column lanes, ragged last column block, 6-row last block
    "full_nc4": ((16, 16), 64, (48, 64), (0, 0, 300, 225), (225, 300)),        # four-column lanes, ragged, 4 live waves
    "tall": ((16, 16), 64, (64, 17), (0, 0, 70, 300), (300, 70)),              # 5 row blocks: a second workgroup with 3 idle waves
    "inside": ((16, 16), 64, (48, 64), (70, 37, 270, 187), (230, 300)),        # crop starts and ends mid-block, blocks outside the crop
    "flush": ((24, 20), 64, (61, 37), (29, 64, 129, 193), (193, 129)),         # non-integer ratios, crop top on a block boundary, flush bottom-right
    "exact64": ((16, 16), 64, (64, 32), (0, 0, 64, 128), (128, 64)),           # r = 64 at the column end, FW = 64
    "down3": ((16, 16), 64, (64, 64), (100, 66, 121, 86), (90, 140)),          # stage 2 down by more than 3: memo rows are skipped
    "stage1_down": ((32, 32), 16, (16, 13), (0, 0, 135, 140), (140, 135)),     # stage 1 down, stage 2 up about 10x: memo rows are reused
    "identity": ((32, 32), 32, (32, 32), (0, 0, 32, 32), (32, 32)),            # every l = 0: the mask is low > thr
    "one_pixel_crop": ((16, 16), 64, (64, 64), (5, 3, 6, 4), (7, 9)),          # CH = CW = 1
    "one_pixel_frame": ((16, 16), 64, (64, 64), (0, 0, 1, 1), (1, 1)),
    "column": ((16, 16), 64, (64, 64), (0, 2, 1, 130), (130, 1)),              # FW = 1, cy0 != 0
    "row": ((16, 16), 64, (64, 64), (0, 0, 130, 1), (1, 130)),                 # every element is a column end
    "wide": ((16, 16), 64, (7, 64), (0, 0, 2100, 200), (200, 2100)),           # 8400 words: three emission trips
    "row_after": ((16, 16), 64, (64, 64), (0, 5, 70, 75), (75, 70)),           # the row after block 0 takes 11 % of a low-res row that no row of the block touches
}
PAIRS = ((0.0, 1.0), (0.25, 0.5), (-0.5, 0.75), (0.25, 0.0), (0.0, -1.0))       # float and double sums agree on all of these
FIX_PAIR = (-1.0, 0.6)                                                          # they do not here: hi = -0.40000001 (double sum) vs -0.39999998
N_SMOOTH = 6
M_PLANES = 12


def crop_hw(geom):
    x0, y0, x1, y1 = geom[3]
    return (y1 - y0, x1 - x0)


def smooth_planes(n, lh, lw, seed, cells=6):
    """Low-frequency random fields (blobs and long borders instead of salt and pepper): coarse normals * 3, resized in float64, plus 0.05 noise."""
    rng = np.random.default_rng(seed)
    coarse = torch.from_numpy(rng.standard_normal((1, n, cells, cells)) * 3)
    up = F.interpolate(coarse, (lh, lw), mode="bilinear", align_corners=False)[0].numpy()
    return (up + rng.standard_normal((n, lh, lw)) * 0.05).astype(F32)


def planes(name, thr, off, seed=0):
    """The M = 12 low-res planes of a geometry at a threshold pair: six smooth, all -5, all +5, constant thr, constant hi, a +-3 checkerboard of
    cells, and a smooth plane with one NaN, one +inf and one -inf cell."""
    (lh, lw) = GEOMS[name][0]
    t, hi, _ = thresholds(thr, off)
    seed = seed + sum(name.encode()) * 101                        # (by the name alone: a geometry added to the table leaves the others' planes alone)
    sm = smooth_planes(N_SMOOTH + 1, lh, lw, seed)
    yy, xx = np.mgrid[0:lh, 0:lw]
    special = sm[N_SMOOTH].copy()
    rng = np.random.default_rng(seed + 1)
    cells = rng.choice(lh * lw, 3, replace=False)
    special.reshape(-1)[cells] = [np.nan, np.inf, -np.inf]
    out = np.concatenate([sm[:N_SMOOTH], np.stack([np.full((lh, lw), -5, F32), np.full((lh, lw), 5, F32), np.full((lh, lw), t, F32),
                                                   np.full((lh, lw), hi, F32), np.where((yy + xx) % 2 == 0, 3, -3).astype(F32), special])])
    assert out.shape == (M_PLANES, lh, lw) and out.dtype == F32
    return out


def fix_pair_planes(name, seed=0):
    """planes() at FIX_PAIR plus four constant planes at both candidate values of hi and lo (double sum / two floats), and the same four
    values planted in cells of smooth plane 0: where every l is 0 (`identity`) the kernel sees them exactly."""
    thr, off = FIX_PAIR
    base = planes(name, thr, off, seed)
    _, hi, lo = thresholds(thr, off)
    hi2, lo2 = thresholds_two_floats(thr, off)
    assert hi != hi2 or lo != lo2
    vals = [hi, hi2, lo, lo2]
    lh, lw = base.shape[1:]
    rng = np.random.default_rng(seed + 5)
    cells = rng.choice(lh * lw, 16, replace=False)
    base[0].reshape(-1)[cells] = np.tile(np.asarray(vals, F32), 4)
    return np.concatenate([base, np.stack([np.full((lh, lw), v, F32) for v in vals])])


def expected(low, geom, thr, off):
    """Everything the fused launch writes, from post32 and the integer oracle.  -> dict: mask bool [M, FH, FW] (the crop pasted into zeros),
    first u8 [M], stab int64 [M, 2] = #(v > hi), #(v > lo), score f32 [M], boxes int64 [M, 4] (crop coordinates), rles, rle_counts, words."""
    _, S1, inp, (x0, y0, x1, y1), (FH, FW) = geom
    v = post32(low, S1, inp, (y1 - y0, x1 - x0))
    t, hi, lo = thresholds(thr, off)
    crop = v > t
    mask = np.zeros((low.shape[0], FH, FW), bool)
    mask[:, y0:y1, x0:x1] = crop
    stab = np.stack([(v > hi).sum((-1, -2)), (v > lo).sum((-1, -2))], -1).astype(np.int64)
    words = change_words(mask)
    t_flat = mask.transpose(0, 2, 1).reshape(low.shape[0], -1)
    return dict(v=v, mask=mask, first=mask[:, 0, 0].astype(np.uint8), stab=stab, score=AO.calculate_stability_score(v, thr, off),
                boxes=AO.batched_mask_to_box(crop), rles=AO.mask_to_rle(mask), words=words,
                rle_counts=(t_flat[:, 1:] != t_flat[:, :-1]).sum(-1).astype(np.int64))


def band_share(v64, band, thr, off):
    """Share of pixels within `band` of any of the three thresholds, and the mask of pixels outside it."""
    near = np.zeros(v64.shape, bool)
    for t in thresholds(thr, off):
        near |= np.abs(v64 - float(t)) <= band
    return float(near.mean()), ~near


# ---- footprint-shortcut inputs ------------------------------------------------------------------------------------------------------
def spike_planes(lh, lw, base, spike, cells=None):
    """One plane per cell: constant `base` with that cell at `spike`."""
    cells = range(lh * lw) if cells is None else cells
    out = np.full((len(cells), lh * lw), base, F32)
    out[np.arange(len(cells)), list(cells)] = F32(spike)
    return out.reshape(len(cells), lh, lw)


def straddle_planes(lh, lw, thr, off, seed=3):
    """Constants on both sides of the footprint margin m = 1e-4 * max(1, |c|): top + 0.5m and bot - 0.5m must be evaluated, top + 2m and bot - 2m
    are decided without a pixel; 1e-6 of noise keeps the planes from being exactly constant."""
    th = [float(x) for x in thresholds(thr, off)]
    top, bot = max(th), min(th)
    rng = np.random.default_rng(seed)
    out = []
    for c, k in ((top, 0.5), (top, 2.0), (bot, -0.5), (bot, -2.0)):
        m = 1e-4 * max(1.0, abs(c))
        out.append((c + k * m + rng.uniform(-1e-6, 1e-6, (lh, lw))).astype(F32))
    return np.stack(out)


def footprint_decision(low2, geom, thr, off, ys, bx0, ncols):
    """The kernel's footprint rule for ONE plane and the block of 64 frame rows from ys and `ncols` frame columns from bx0, restated with scalar taps:
    -> 0 (evaluate), 1 (all above), 2 (all below)."""
    (LH, LW), S1, (nh, nw), (cx0, cy0, cx1, cy1), (FH, FW) = geom
    CH, CW = cy1 - cy0, cx1 - cx0
    r = min(64, FH - ys)
    cl = lambda a, n: min(max(a, 0), n - 1)
    xl, xh = cl(bx0 - cx0, CW), cl(bx0 + ncols - 1 - cx0, CW)
    yl, yh = cl(ys - cy0, CH), cl(ys + r - cy0, CH)
    lc0 = int(tap(int(tap(xl, nw, CW)[0]), LW, S1)[0]); lc1 = int(tap(int(tap(xh, nw, CW)[1]), LW, S1)[1])
    lr0 = int(tap(int(tap(yl, nh, CH)[0]), LH, S1)[0]); lr1 = int(tap(int(tap(yh, nh, CH)[1]), LH, S1)[1])
    cells = low2[lr0:lr1 + 1, lc0:lc1 + 1]
    if np.isnan(cells).any():
        return 0
    mn, mx = F32(cells.min()), F32(cells.max())
    with np.errstate(all="ignore"):
        margin = F32(1e-4) * max(F32(1), max(abs(mn), abs(mx)))
        t, hi, lo = thresholds(thr, off)
        if mn > F32(max(hi, lo, t) + margin):
            return 1
        if mx < F32(min(hi, lo, t) - margin):
            return 2
    return 0


# ---- NMS ----------------------------------------------------------------------------------------------------------------------------
def _pack_upper(gt):
    """bool [N, N] -> uint64 [N, ceil(N/64)], upper triangle only (bit j of word w of row i = column 64w + j)."""
    n = gt.shape[0]
    nw = (n + 63) // 64
    up = np.triu(gt, 1)
    pad = np.zeros((n, nw * 64), bool)
    pad[:, :n] = up
    return np.bitwise_or.reduce(pad.reshape(n, nw, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64), axis=-1)


def nms_bits32(boxes, thr):
    """The suppression matrix in float32, in nms_mask_kernel's order: inter / ((ai + aj) - inter) > thr (0 / 0 is NaN: false)."""
    b = np.asarray(boxes, F32)
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    w = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), F32(0))
    h = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), F32(0))
    inter = (w * h).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / ((area[:, None] + area[None, :]).astype(F32) - inter).astype(F32)
    return _pack_upper(iou > F32(thr))


def nms_bits_exact(boxes, thr_num, thr_den):
    """The same matrix in Python integers for integer boxes: IoU > num / den  <=>  inter * den > num * union, false when union == 0."""
    b = [[int(v) for v in row] for row in np.asarray(boxes).tolist()]
    n = len(b)
    gt = np.zeros((n, n), bool)
    for i in range(n):
        x1, y1, x2, y2 = b[i]
        ai = (x2 - x1) * (y2 - y1)
        for j in range(i + 1, n):
            u1, v1, u2, v2 = b[j]
            inter = max(min(x2, u2) - max(x1, u1), 0) * max(min(y2, v2) - max(y1, v1), 0)
            union = ai + (u2 - u1) * (v2 - v1) - inter
            gt[i, j] = union != 0 and inter * thr_den > thr_num * union
    return _pack_upper(gt)


NMS_SIZES = (1, 64, 65, 128, 129, 200)
NMS_THRESHOLDS = ((1, 4), (1, 2), (3, 4))


@functools.lru_cache(maxsize=None)
def _nms_boxes(n, seed):
    rng = np.random.default_rng(seed + n)
    xy = rng.integers(0, 700, (n, 2))
    wh = rng.integers(1, 325, (n, 2))
    b = np.concatenate([xy, xy + wh], 1).astype(np.int64)                       # coordinates in [0, 1024]
    plant = [                                                                   # rows planted over the random ones, as far as n allows
        [0, 0, 1024, 1024], [0, 0, 1024, 1024],                                 # duplicates (IoU 1)
        [100, 100, 140, 120], [100, 100, 120, 120],                             # nested, IoU exactly 1/2
        [200, 200, 240, 240], [200, 200, 220, 220],                             # nested, IoU exactly 1/4
        [300, 300, 300, 340], [300, 300, 300, 340],                             # zero area and its duplicate: union 0
        [50, 60, 50, 60], [50, 60, 50, 60],                                     # a point, twice
        [400, 400, 450, 450], [450, 400, 500, 450], [400, 450, 450, 500],       # boxes that only touch (edge, edge)
        [450, 450, 500, 500],                                                   # ... and at a corner
        [600, 600, 640, 630], [600, 600, 640, 610],                             # nested, IoU exactly 1/3 (between the thresholds)
        [700, 100, 740, 140], [700, 100, 730, 140],                             # nested, IoU exactly 3/4
    ]
    pos = rng.permutation(n)[:min(n, len(plant))]                               # scattered, so pairs straddle the 64-box blocks
    for p, row in zip(pos, plant):
        b[p] = row
    if n >= 129:                                                                # a duplicate pair across the first and the last block
        b[1] = b[n - 1] = [10, 20, 300, 400]
    return b


def nms_int_boxes(n, seed=0):
    return _nms_boxes(n, seed).copy()


def nms_float_boxes(n):
    """The seeded float boxes of tests/test_amg_gpu.py::test_box_nms_matches_oracle."""
    rng = np.random.default_rng(n)
    xy = rng.uniform(0, 900, (n, 2)).astype(F32)
    wh = rng.uniform(5, 300, (n, 2)).astype(F32)
    return np.concatenate([xy, xy + wh], 1)


# ---- helper inputs -------------------------------------------------------------------------------------------------------------------
def stability_values(n, per, thr, off, seed=0):
    """f32 [n, per]: seeded normals around the thresholds, planted with hi, lo, nextafter of each in both directions, NaN, +-inf and +-0; the
    LAST plane lies entirely below every threshold (0 / 0: its score is NaN)."""
    t, hi, lo = thresholds(thr, off)
    rng = np.random.default_rng(seed + per)
    x = (rng.standard_normal((n, per)) * 1.5 + float(t)).astype(F32)
    planted = [hi, lo, np.nextafter(hi, F32(np.inf)), np.nextafter(hi, F32(-np.inf)), np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf)),
               F32(np.nan), F32(np.inf), F32(-np.inf), F32(0.0), F32(-0.0)]
    hi2, lo2 = thresholds_two_floats(thr, off)
    planted += [hi2, lo2]                                                        # differ from hi / lo only where the float and double sums do
    flat = x[:n - 1].reshape(-1)
    reps = max(1, min(8, flat.size // len(planted)))
    pos = rng.choice(flat.size, min(flat.size, reps * len(planted)), replace=False)
    flat[pos] = np.resize(np.asarray(planted, F32), len(pos))
    x[n - 1] = F32(min(float(hi), float(lo), float(t)) - 1.0) - np.abs(x[n - 1])
    return x
