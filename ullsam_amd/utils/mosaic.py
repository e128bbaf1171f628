"""Tiled segment-everything: a frame far larger than the model's input is cut into overlapping tiles, every tile is segmented at its native
resolution, and the per-tile instance label maps are stitched into ONE label image.  This module is the definition (numpy, integers only)
and the driver of the device route (csrc/mosaic.hip); the two are equal bit for bit (tests/test_mosaic_*.py).  DESIGN.md "7b, continued
(mosaic)" states the definition and why it is what it is.

    grid = tile_grid(H, W, tile=2048, overlap=256)
    labels, label_of_global, areas, boxes = stitch_label_maps(tiles, counts, grid, device="cuda")

The result has the types and conventions of utils.amg.paint_label_map (labels int32 [H, W], ids 1..K, areas int32 [K], boxes int32 [K, 4]
inclusive XYXY), so it goes straight into instance_scores, prompts_from_labels and resize_labels_nearest.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

MAX_IDS = 2 ** 31 - 2


def _axis_starts(extent: int, tile: int, overlap: int) -> Tuple[int, List[int]]:
    """Intervals of length t = min(tile, extent): 0, stride, 2 * stride, ... (stride = tile - overlap) for as long as the interval ends before the
    border AND the closing interval [extent - t, extent) would not start inside the one BEFORE it; then the closing interval.  The second
    condition only ever removes the last regular start (never the start 0): without it the closing interval, which is pushed back to end at
    the border, can reach into the last two regular intervals at once -- e.g. extent 170, tile 64, overlap 16: [48, 112), [96, 160), [106, 170)
    all hold 106..111 -- and the definition below rests on a coordinate lying in at most two intervals."""
    t = min(tile, extent)
    stride = tile - overlap
    starts: List[int] = []
    s = 0
    while s + t < extent and (s == 0 or s + overlap <= extent - t):
        starts.append(s)
        s += stride
    starts.append(extent - t)
    return t, starts


def _cuts(starts: Sequence[int], t: int, extent: int) -> List[int]:
    """cut i = the middle of the overlap of the intervals i and i + 1; interval i owns [cut i-1, cut i), cut -1 = 0 and the last cut = extent."""
    return [0] + [(starts[i + 1] + starts[i] + t) // 2 for i in range(len(starts) - 1)] + [extent]


@dataclass(frozen=True)
class TileGrid:
    """The tiles of an [H, W] frame: all of size (th, tw), numbered row-major t = r * ncols + c, tile (r, c) at (row_starts[r], col_starts[c]).
    row_cuts / col_cuts have one entry more than there are rows / columns: tile (r, c) owns -- its CORE -- the rows [row_cuts[r], row_cuts[r + 1])
    and the columns [col_cuts[c], col_cuts[c + 1]).  The cores partition the frame."""
    H: int
    W: int
    th: int
    tw: int
    row_starts: Tuple[int, ...]
    col_starts: Tuple[int, ...]
    row_cuts: Tuple[int, ...]
    col_cuts: Tuple[int, ...]

    @property
    def nrows(self) -> int:
        return len(self.row_starts)

    @property
    def ncols(self) -> int:
        return len(self.col_starts)

    @property
    def ntiles(self) -> int:
        return self.nrows * self.ncols

    def boxes(self) -> List[Tuple[int, int, int, int]]:
        """(top, left, h, w) of every tile, in tile order."""
        return [(r, c, self.th, self.tw) for r in self.row_starts for c in self.col_starts]

    def cores(self) -> List[Tuple[int, int, int, int]]:
        """(top, left, h, w) of every tile's core, in tile order."""
        return [(self.row_cuts[r], self.col_cuts[c], self.row_cuts[r + 1] - self.row_cuts[r], self.col_cuts[c + 1] - self.col_cuts[c])
                for r in range(self.nrows) for c in range(self.ncols)]

    def seams(self) -> List[Tuple[int, int, int, Tuple[int, int, int, int]]]:
        """(s, t, dir, (top, left, h, w)): every tile s with its right (dir 0) and its lower (dir 1) neighbour t and the intersection of their boxes,
        in tile order of s.  An empty intersection (overlap 0) is no seam."""
        out = []
        for r in range(self.nrows):
            for c in range(self.ncols):
                s = r * self.ncols + c
                top, left = self.row_starts[r], self.col_starts[c]
                if c + 1 < self.ncols:
                    l2 = self.col_starts[c + 1]
                    if left + self.tw > l2:
                        out.append((s, s + 1, 0, (top, l2, self.th, left + self.tw - l2)))
                if r + 1 < self.nrows:
                    t2 = self.row_starts[r + 1]
                    if top + self.th > t2:
                        out.append((s, s + self.ncols, 1, (t2, left, top + self.th - t2, self.tw)))
        return out


def tile_grid(H: int, W: int, tile: int, overlap: int) -> TileGrid:
    """The tile grid of an [H, W] frame for square tiles of side `tile` that share `overlap` pixels with their neighbours (the last row / column
    is pushed back to end at the border, so it may share more; where that would make three intervals meet, the regular interval before it is
    left out and the last pair shares less -- see _axis_starts).  Requires 0 <= overlap <= tile // 2."""
    H, W, tile, overlap = int(H), int(W), int(tile), int(overlap)
    if H < 1 or W < 1 or tile < 1:
        raise ValueError(f"tile_grid: H, W and tile must be positive, got {(H, W, tile)}")
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f"tile_grid: overlap {overlap} must lie in 0..tile // 2 = {tile // 2}")
    th, rows = _axis_starts(H, tile, overlap)
    tw, cols = _axis_starts(W, tile, overlap)
    return TileGrid(H, W, th, tw, tuple(rows), tuple(cols), tuple(_cuts(rows, th, H)), tuple(_cuts(cols, tw, W)))


def _check_iou(iou) -> Tuple[int, int]:
    num, den = (int(v) for v in iou)
    if not 0 < num <= den < 2 ** 31:
        raise ValueError(f"stitch_label_maps: iou = (num, den) needs 0 < num <= den < 2^31, got {iou}")
    return num, den


def _bases(counts, ntiles: int) -> np.ndarray:
    k = (counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).astype(np.int64).reshape(-1)
    if len(k) != ntiles or (k < 0).any():
        raise ValueError(f"stitch_label_maps: {len(k)} counts for {ntiles} tiles (each >= 0)")
    base = np.concatenate([[0], np.cumsum(k)])
    if int(base[-1]) > MAX_IDS:
        raise _lib.UllsamError(f"stitch_label_maps: {int(base[-1])} ids in all (at most 2^31 - 2)")
    return base


def _merge_components(a: np.ndarray, b: np.ndarray, g: int) -> np.ndarray:
    """rep int64 [g + 1]: the smallest id of the connected component of every id under the edges (a[i], b[i])."""
    rep = np.arange(g + 1, dtype=np.int64)
    while len(a):
        ra, rb = rep[a], rep[b]
        if np.array_equal(ra, rb):
            break
        m = np.minimum(ra, rb)
        np.minimum.at(rep, ra, m)                       # hook the two current representatives (and the ends) under the smaller one ...
        np.minimum.at(rep, rb, m)
        np.minimum.at(rep, a, m)
        np.minimum.at(rep, b, m)
        while True:                                      # ... and jump: rep becomes idempotent again
            nxt = rep[rep]
            if np.array_equal(nxt, rep):
                break
            rep = nxt
    return rep


def _stitch_host(tiles: np.ndarray, base: np.ndarray, grid: TileGrid, num: int, den: int, mva: int, max_pairs: int):
    T = grid.ntiles
    g = int(base[-1])
    k = np.diff(base)
    if tiles.size and ((tiles < 0).any() or (tiles > k[:, None, None]).any()):
        t = int(np.nonzero(((tiles < 0) | (tiles > k[:, None, None])).reshape(T, -1).any(1))[0][0])
        raise _lib.UllsamError(f"stitch_label_maps: tile {t} holds an id outside 0..{int(k[t])}")
    glob = np.where(tiles > 0, tiles.astype(np.int64) + base[:-1, None, None], 0)
    boxes_t = grid.boxes()
    ea, eb, npairs = [], [], 0
    for s, t, _, (top, left, h, w) in grid.seams():
        ps = glob[s, top - boxes_t[s][0]:top - boxes_t[s][0] + h, left - boxes_t[s][1]:left - boxes_t[s][1] + w].reshape(-1)
        pt = glob[t, top - boxes_t[t][0]:top - boxes_t[t][0] + h, left - boxes_t[t][1]:left - boxes_t[t][1] + w].reshape(-1)
        both = (ps > 0) & (pt > 0)
        if not both.any():
            continue
        area_s = np.bincount(np.where(ps > 0, ps - base[s], 0), minlength=int(k[s]) + 1)     # in-seam areas by LOCAL id
        area_t = np.bincount(np.where(pt > 0, pt - base[t], 0), minlength=int(k[t]) + 1)
        key, n = np.unique(ps[both] * (g + 1) + pt[both], return_counts=True)
        a, b = key // (g + 1), key % (g + 1)
        npairs += len(key)
        if npairs > max_pairs:
            raise _lib.UllsamError(f"stitch_label_maps: more than max_pairs = {max_pairs} distinct label pairs in the seams")
        n = n.astype(np.int64)
        merge = n * den >= num * (area_s[a - base[s]] + area_t[b - base[t]] - n)
        ea.append(a[merge])
        eb.append(b[merge])
    rep = _merge_components(np.concatenate(ea) if ea else np.zeros(0, np.int64), np.concatenate(eb) if eb else np.zeros(0, np.int64), g)
    raw = np.zeros((grid.H, grid.W), np.int64)
    for t, (top, left, h, w) in enumerate(grid.cores()):
        oy, ox = boxes_t[t][0], boxes_t[t][1]
        raw[top:top + h, left:left + w] = rep[glob[t, top - oy:top - oy + h, left - ox:left - ox + w]]
    area_raw = np.bincount(raw.reshape(-1), minlength=g + 1)
    keep = (area_raw != 0) & (area_raw >= mva)
    keep[0] = False
    lmap = (np.cumsum(keep) * keep).astype(np.int32)
    labels = lmap[raw]
    kk = int(keep.sum())
    boxes = np.zeros((kk, 4), np.int32)
    ys, xs = np.nonzero(labels)
    lab = labels[ys, xs] - 1
    for col, vals, fn in ((0, xs, np.minimum), (1, ys, np.minimum), (2, xs, np.maximum), (3, ys, np.maximum)):
        acc = np.full((kk,), np.iinfo(np.int32).max if fn is np.minimum else -1, np.int64)
        fn.at(acc, lab, vals)
        boxes[:, col] = acc
    return labels, lmap[rep], area_raw[keep].astype(np.int32), boxes


def seam_table(grid: TileGrid) -> np.ndarray:
    """The seams as the kernels read them: int32 [S, 9] = (s, t, sy, sx, ty, tx, h, w, dir), the region as a window of each of the two tiles."""
    b = grid.boxes()
    rows = [(s, t, top - b[s][0], left - b[s][1], top - b[t][0], left - b[t][1], h, w, d) for s, t, d, (top, left, h, w) in grid.seams()]
    return np.asarray(rows, np.int32).reshape(-1, 9)


def core_table(grid: TileGrid) -> np.ndarray:
    """The cores as the kernels read them: int32 [T, 6] = (top, left, h, w of the core in the frame, the tile's origin oy, ox)."""
    return np.asarray([c + b[:2] for c, b in zip(grid.cores(), grid.boxes())], np.int32).reshape(-1, 6)


def stitch_label_maps(tiles, counts, grid: TileGrid, iou=(1, 2), min_visible_area: int = 0, max_pairs: int = 1 << 20, device=None):
    """Per-tile instance label maps -> one label image of the frame.  tiles int32 [T, th, tw] (the tiles of `grid`, in its order), counts[t] = K_t:
    tile t uses the ids 0..K_t, 0 = background.  The global id of (t, l > 0) is base_t + l, base_t = sum of K_s over s < t; G = the sum of all K_t.

    1. Seams: for every tile s and its right / lower neighbour t, over the intersection R of their boxes, n(a, b) = #{p in R: s(p) = a, t(p) = b}
       for a, b > 0, A_s(a) = #{p in R: s(p) = a}, A_t(b) = #{p in R: t(p) = b}.
    2. (a, b) is MERGED iff n > 0 and n * den >= num * (A_s(a) + A_t(b) - n), iou = (num, den): the IoU of the two labels INSIDE the seam, where
       both tiles see the same pixels, is at least num / den.  Equality merges; background never does.
    3. Components of the merge graph over 1..G; a component is represented by its SMALLEST global id.
    4. Paint: a pixel p of the core of tile t gets the representative of g(t, tile_t[p - origin_t]); only the owner tile speaks.
    5. A component whose visible area (its pixels in that image) is 0 or below min_visible_area is dropped (its pixels become 0); the others are
       renumbered 1..K by ascending representative.

    -> (labels int32 [H, W], label_of_global int32 [G + 1] (0 for the background and for members of dropped components), areas int32 [K],
    boxes int32 [K, 4] inclusive XYXY).  More than max_pairs distinct (a, b) pairs in the seams, G > 2^31 - 2 or an id outside 0..K_t raise UllsamError.
    device None / "cpu": this definition in numpy.  A GPU device: csrc/mosaic.hip on the tiles where they are (five launches of kernels, ONE
    read-back: the status words and K); `counts` is host data there (a GPU tensor costs a second read-back)."""
    num, den = _check_iou(iou)
    mva = int(min(max(int(min_visible_area), 0), 2 ** 31 - 1))
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise ValueError(f"stitch_label_maps: max_pairs must lie in 1..2^30, got {max_pairs}")
    T = grid.ntiles
    if tuple(tiles.shape) != (T, grid.th, grid.tw):
        raise ValueError(f"stitch_label_maps: tiles {tuple(tiles.shape)} for a grid of [{T}, {grid.th}, {grid.tw}]")
    base = _bases(counts, T)
    dev = torch.device("cpu" if device is None else device)
    if dev.type != "cuda":
        tl = tiles.detach().cpu().numpy() if isinstance(tiles, torch.Tensor) else np.asarray(tiles)
        return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in _stitch_host(tl.astype(np.int32), base, grid, num, den, mva, max_pairs))
    from .. import ops
    if T > ops.MOSAIC_MAX_TILES:
        raise _lib.UllsamError(f"stitch_label_maps: {T} tiles (at most {ops.MOSAIC_MAX_TILES})")
    tl = torch.as_tensor(tiles, device=dev).to(torch.int32).contiguous()
    g = int(base[-1])
    seams, cores = seam_table(grid), core_table(grid)
    # one upload: base | seams | cores
    up = torch.from_numpy(np.concatenate([base.astype(np.int32), seams.reshape(-1), cores.reshape(-1)])).to(dev)
    base_d, seams_d, cores_d = up[:T + 1], up[T + 1:T + 1 + seams.size].view(-1, 9), up[T + 1 + seams.size:].view(-1, 6)
    flags = torch.empty((ops.MOSAIC_FLAGS,), dtype=torch.int32, device=dev)            # bad id | overflow | pairs | K: the one read-back
    seam_rows = int(seams[:, 6].max()) if len(seams) else 0
    core_rows = int(cores[:, 2].max())
    keys, cnt, areas_seam, _ = ops.mosaic_seams(tl, base_d, g, seams_d, seam_rows, max_pairs, flags=flags)
    parent, _ = ops.mosaic_union(keys, g, cnt, areas_seam, (num, den), flags=flags)
    areas_raw, boxes_raw, _ = ops.mosaic_stats(tl, base_d, g, cores_d, core_rows, parent, grid.H, grid.W, flags=flags)
    log, areas, boxes, _ = ops.mosaic_compact(areas_raw, boxes_raw, parent, mva, k_out=flags[3:])
    labels = ops.mosaic_paste(tl, base_d, g, cores_d, core_rows, log, grid.H, grid.W)
    fl = flags.cpu().numpy()
    if fl[0]:
        raise _lib.UllsamError("stitch_label_maps: a tile holds an id outside 0..K_t")
    if fl[1] or fl[2] > max_pairs:
        raise _lib.UllsamError(f"stitch_label_maps: more than max_pairs = {max_pairs} distinct label pairs in the seams")
    k = int(fl[3])
    return labels, log, areas[:k], boxes[:k]
