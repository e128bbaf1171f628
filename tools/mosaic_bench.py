"""Time the label-map stitch (utils.mosaic.stitch_label_maps) on a synthetic mosaic, in one process, the two routes alternating:

  (a) the host form: the numpy definition, tiles in host memory;
  (b) the device route (csrc/mosaic.hip): tiles resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call.

The frame is a grid x grid mosaic of tile^2 tiles with the given overlap (default 4 x 4 of 2048^2, overlap 256: 7424^2 = 55 M pixels).  Discs of
utils.synthetic.label_tile's geometry are drawn on the FULL frame (synthetic.label_frame) and the frame is cut into the tiles, every tile
renumbering the instances it sees 1..K_t -- what sixteen generate_label_map calls would leave behind.

    python tools/mosaic_bench.py [--tile 2048] [--overlap 256] [--grid 4] [--cells-per-mpx 14] [--reps 3]

Prints every run, the medians and the spread (max - min), whether the two routes give identical outputs, and the stitch time beside the time of
the tile^2 segment-everything calls it follows (the README's measured 2048^2 tile; no model runs here).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ullsam_amd.utils import mosaic as M  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

TILE_SECONDS = 0.097     # one 2048^2 tile of segment-everything (README, configs[4]); a tile's generate_label_map adds the paint to it


def cut(frame: np.ndarray, grid: M.TileGrid):
    tiles = np.zeros((grid.ntiles, grid.th, grid.tw), np.int32)
    counts = []
    lut = np.zeros(int(frame.max()) + 1, np.int32)
    for t, (top, left, h, w) in enumerate(grid.boxes()):
        win = frame[top:top + h, left:left + w]
        ids = np.unique(win)
        ids = ids[ids > 0]
        lut[:] = 0
        lut[ids] = np.arange(1, len(ids) + 1)
        tiles[t] = lut[win]
        counts.append(len(ids))
    return tiles, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=int, default=256)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--cells-per-mpx", type=float, default=14.0, help="discs per 2^20 pixels (label_tile's default density on a 1024^2 tile)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    side = a.tile + (a.grid - 1) * (a.tile - a.overlap)
    grid = M.tile_grid(side, side, a.tile, a.overlap)
    assert grid.nrows == grid.ncols == a.grid
    n_cells = int(round(a.cells_per_mpx * side * side / 2 ** 20))
    t0 = time.perf_counter()
    frame = S.label_frame(1, side, side, n_cells)
    tiles, counts = cut(frame, grid)
    print(f"{a.grid} x {a.grid} tiles of {a.tile}^2, overlap {a.overlap}: a {side}^2 frame ({side * side / 1e6:.1f} M pixels), {n_cells} discs drawn, "
          f"{sum(counts)} per-tile labels in all (built in {time.perf_counter() - t0:.1f} s)")
    tiles_d = torch.from_numpy(tiles).cuda()
    dev = M.stitch_label_maps(tiles_d, counts, grid, device="cuda")                 # warm-up: allocator, code objects
    torch.cuda.synchronize()
    ta, tb = [], []
    host = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        host = M.stitch_label_maps(tiles, counts, grid, device="cpu")
        ta.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = M.stitch_label_maps(tiles_d, counts, grid, device="cuda")
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t0)
    same = [bool(torch.equal(d.cpu(), h)) for d, h in zip(dev, host)]
    med = lambda t: statistics.median(t)
    spread = lambda t: max(t) - min(t)
    fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)
    k = int(dev[0].max())
    print(f"{k} instances in the mosaic ({len(np.unique(frame)) - 1} visible discs in the frame it was cut from)")
    print(f"(a) host form    numpy definition, tiles in host memory:        runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
    print(f"(b) device       stitch_label_maps, tiles resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s")
    print(f"identical outputs (labels, label_of_global, areas, boxes): {same} -> {'IDENTICAL' if all(same) else 'DIFFERENT'}")
    print(f"(a) / (b) = {med(ta) / med(tb):.1f}x; (a) - (b) = {med(ta) - med(tb):.4f} s against (a)'s spread {spread(ta):.4f} s")
    px = side * side
    seam_px = sum(h * w for _, _, _, (_, _, h, w) in grid.seams())
    nbytes = 8 * seam_px + 4 * px + 8 * px
    print(f"algorithmic bytes of (b): 8 B x {seam_px / 1e6:.1f} M seam pixels (two tiles read) + 4 B x H*W (stats read of the cores) + 8 B x H*W (paste read + write) "
          f"= {nbytes / 1e6:.0f} MB = {nbytes / 8e12 * 1e6:.0f} us at 8 TB/s; measured {med(tb) * 1e6:.0f} us (upload of the tables, launches and the read-back included)")
    tile_s = TILE_SECONDS * (a.tile / 2048) ** 2
    print(f"(b) beside the {grid.ntiles} tile calls it follows ({grid.ntiles} x {tile_s:.3f} s = {grid.ntiles * tile_s:.2f} s, README's 2048^2 tile scaled by area; not measured here): "
          f"{med(tb) / (grid.ntiles * tile_s) * 100:.2f} % of their time; the host form would be {med(ta) / (grid.ntiles * tile_s) * 100:.0f} %")


if __name__ == "__main__":
    main()
