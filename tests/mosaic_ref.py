"""Plain-loop definitions of the label-map mosaic (ullsam_amd/utils/mosaic.py), and the cases the CPU and the GPU tests share.

Everything here is written the slow, obvious way on purpose: per-pixel Python loops for the seam counts, a dictionary union-find, and a
pixel's owner found by testing every core.  Of the grid only boxes(), cores() and the row-major numbering are used."""
import numpy as np


# ---- the definition, in loops --------------------------------------------------------------------------------------------------------
class DictUnionFind:
    def __init__(self):
        self.parent = {}

    def find(self, x):
        self.parent.setdefault(x, x)
        while self.parent[x] != x:
            x = self.parent[x]
        return x

    def union(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            self.parent[max(ra, rb)] = min(ra, rb)       # the smaller root stays a root: a component's root is its smallest member


def representatives(pairs, g):
    """rep[0..g] under the edges `pairs`: the smallest id of every id's component."""
    uf = DictUnionFind()
    for a, b in pairs:
        uf.union(int(a), int(b))
    return np.asarray([uf.find(i) for i in range(g + 1)], np.int64)


def seam_list(grid):
    """(s, t, dir, top, left, h, w): 4-neighbour pairs (right: dir 0, down: dir 1) and the intersection of their boxes, empty ones left out."""
    boxes = grid.boxes()
    out = []
    for r in range(grid.nrows):
        for c in range(grid.ncols):
            s = r * grid.ncols + c
            for t, d in ((s + 1, 0), (s + grid.ncols, 1)):
                if (d == 0 and c + 1 >= grid.ncols) or (d == 1 and r + 1 >= grid.nrows):
                    continue
                top, left = max(boxes[s][0], boxes[t][0]), max(boxes[s][1], boxes[t][1])
                bot = min(boxes[s][0] + boxes[s][2], boxes[t][0] + boxes[t][2])
                right = min(boxes[s][1] + boxes[s][3], boxes[t][1] + boxes[t][3])
                if bot > top and right > left:
                    out.append((s, t, d, top, left, bot - top, right - left))
    return out


def seam_counts(tiles, base, grid):
    """-> (pairs {(dir, g_a, g_b): n}, areas {(g, side): pixels of g inside the seam on that side of its tile}; side 0 left, 1 right, 2 up, 3 down)."""
    boxes = grid.boxes()
    pairs, areas = {}, {}
    for s, t, d, top, left, h, w in seam_list(grid):
        for y in range(top, top + h):
            for x in range(left, left + w):
                a = int(tiles[s][y - boxes[s][0]][x - boxes[s][1]])
                b = int(tiles[t][y - boxes[t][0]][x - boxes[t][1]])
                if a > 0:
                    ka = (int(base[s]) + a, 3 if d else 1)
                    areas[ka] = areas.get(ka, 0) + 1
                if b > 0:
                    kb = (int(base[t]) + b, 2 if d else 0)
                    areas[kb] = areas.get(kb, 0) + 1
                if a > 0 and b > 0:
                    k = (d, int(base[s]) + a, int(base[t]) + b)
                    pairs[k] = pairs.get(k, 0) + 1
    return pairs, areas


def stitch(tiles, counts, grid, iou=(1, 2), min_visible_area=0):
    """-> (labels int32 [H, W], label_of_global int32 [G + 1], areas int32 [K], boxes int32 [K, 4])"""
    tiles = np.asarray(tiles)
    base = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    g = int(base[-1])
    num, den = iou
    pairs, areas = seam_counts(tiles, base, grid)
    merged = []
    for (d, a, b), n in pairs.items():
        union = areas[(a, 3 if d else 1)] + areas[(b, 2 if d else 0)] - n
        if n > 0 and n * den >= num * union:
            merged.append((a, b))
    rep = representatives(merged, g)
    boxes, cores = grid.boxes(), grid.cores()
    raw = np.zeros((grid.H, grid.W), np.int64)
    for y in range(grid.H):
        for x in range(grid.W):
            owners = [t for t, (top, left, h, w) in enumerate(cores) if top <= y < top + h and left <= x < left + w]
            assert len(owners) == 1, "the cores partition the frame"
            t = owners[0]
            l = int(tiles[t][y - boxes[t][0]][x - boxes[t][1]])
            raw[y, x] = rep[int(base[t]) + l] if l > 0 else 0
    visible = {}
    for y in range(grid.H):
        for x in range(grid.W):
            v = int(raw[y, x])
            if v:
                bx = visible.setdefault(v, [0, x, y, x, y])
                bx[0] += 1
                bx[1], bx[2], bx[3], bx[4] = min(bx[1], x), min(bx[2], y), max(bx[3], x), max(bx[4], y)
    kept = [v for v in sorted(visible) if visible[v][0] >= min_visible_area]
    final = {v: i + 1 for i, v in enumerate(kept)}
    labels = np.zeros((grid.H, grid.W), np.int32)
    for y in range(grid.H):
        for x in range(grid.W):
            labels[y, x] = final.get(int(raw[y, x]), 0)
    log = np.asarray([final.get(int(rep[i]), 0) if i else 0 for i in range(g + 1)], np.int32)
    return (labels, log, np.asarray([visible[v][0] for v in kept], np.int32).reshape(-1),
            np.asarray([visible[v][1:] for v in kept], np.int32).reshape(-1, 4))


def paste(tiles, grid):
    """The slicing expression: every tile's core copied as it is."""
    out = np.zeros((grid.H, grid.W), np.int32)
    for t, ((top, left, h, w), (oy, ox, _, _)) in enumerate(zip(grid.cores(), grid.boxes())):
        out[top:top + h, left:left + w] = tiles[t][top - oy:top - oy + h, left - ox:left - ox + w]
    return out


def same_up_to_a_bijection(a, b):
    """Two label images describe the same partition: the pairs (a[p], b[p]) form a bijection that fixes 0."""
    pairs = np.unique(np.stack([a.reshape(-1), b.reshape(-1)], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])) and all((x == 0) == (y == 0) for x, y in pairs)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
GRIDS = [(150, 170, 64, 16), (33, 200, 64, 32), (64, 64, 64, 0), (65, 64, 64, 7), (40, 50, 64, 16), (129, 131, 33, 7), (200, 96, 64, 0)]
LARGE = (600, 520, 256, 64)      # many workgroups: the GPU tests only (the loops above would take minutes)


def cut(truth, grid, seed):
    """A ground-truth label image cut into the grid's tiles; every tile renumbers the instances it sees 1..K_t in a seeded shuffled order."""
    rng = np.random.default_rng(seed)
    tiles = np.zeros((grid.ntiles, grid.th, grid.tw), np.int32)
    counts = []
    for t, (top, left, h, w) in enumerate(grid.boxes()):
        win = truth[top:top + h, left:left + w]
        ids = np.unique(win[win > 0])
        lut = np.zeros(int(truth.max()) + 1, np.int32)
        lut[rng.permutation(ids)] = np.arange(1, len(ids) + 1)
        tiles[t] = lut[win]
        counts.append(len(ids))
    return tiles, counts


def add_discs(truth, n, r_range, seed):
    """Discs of label_tile's geometry (uniform centres, (x - cx)^2 + (y - cy)^2 < r^2) that are drawn only where nothing is drawn yet and only
    whole: an instance stays one connected piece, so the tiles' views of it can be told to be one instance."""
    rng = np.random.default_rng([seed, 0x5EED])
    h, w = truth.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    nxt = int(truth.max()) + 1
    for _ in range(n):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(*r_range)
        disc = (xx - np.float32(cx)) ** 2 + (yy - np.float32(cy)) ** 2 < np.float32(r) ** 2
        if disc.any() and not truth[disc].any():
            truth[disc] = nxt
            nxt += 1
    return truth


def hand_placed(grid):
    """Instances placed by the grid's cuts (needs >= 2 rows and >= 3 columns of tiles): one spanning 2 tiles, one spanning 3, one spanning 4, one
    wholly inside the seam of tiles 0 and 1, and one that reaches across a cut by a single pixel."""
    assert grid.nrows >= 2 and grid.ncols >= 3
    truth = np.zeros((grid.H, grid.W), np.int32)
    rc, cc = grid.row_cuts, grid.col_cuts
    truth[2:5, cc[1] - 4:cc[1] + 4] = 1                                         # 2 tiles, across the first column cut
    truth[7:9, cc[1] - 3:cc[2] + 3] = 2                                         # 3 tiles of the first row
    truth[rc[1] - 3:rc[1] + 3, cc[2] - 3:cc[2] + 3] = 3                         # 4 tiles, around a corner of cuts
    s1, e0 = grid.col_starts[1], grid.col_starts[0] + grid.tw
    truth[12:15, s1:min(s1 + 3, e0)] = 4                                        # inside the seam of tiles 0 and 1 (both see all of it)
    truth[18:21, cc[1] - 5:cc[1]] = 5                                           # left of the cut ...
    truth[19, cc[1]] = 5                                                        # ... and one pixel across it
    return truth


def truth_case(name, H, W, tile, overlap, seed, n_discs, r_range, hand=False, iou=(1, 2), mva=0):
    from ullsam_amd.utils.mosaic import tile_grid
    grid = tile_grid(H, W, tile, overlap)
    truth = hand_placed(grid) if hand else np.zeros((H, W), np.int32)
    add_discs(truth, n_discs, r_range, seed)
    tiles, counts = cut(truth, grid, seed + 1)
    return dict(name=name, grid=(H, W, tile, overlap), tiles=tiles, counts=counts, iou=iou, mva=mva, truth=truth)


def threshold_case(iou):
    """1 x 2 tiles of 8 x 16 over an 8 x 24 frame, seam = columns 8..15.  Tile 0: label 1 fills the seam's rows 0..3 (32 pixels there) and reaches
    left of it; label 2 is the seam's rows 4..7, columns 8..11.  Tile 1: labels 1 and 2 are the two halves (16 pixels each) of label 1's seam part
    -- IoU 16 / (32 + 16 - 16) = 1 / 2 with each --, label 3 has exactly label 2's footprint, label 4 lies outside the seam."""
    s = np.zeros((8, 16), np.int32)
    t = np.zeros((8, 16), np.int32)
    s[0:4, 5:16] = 1
    s[4:8, 8:12] = 2
    t[0:4, 0:4] = 1
    t[0:4, 4:8] = 2
    t[4:8, 0:4] = 3
    t[5:7, 10:14] = 4
    return dict(name=f"threshold{iou}", grid=(8, 24, 16, 8), tiles=np.stack([s, t]), counts=[2, 4], iou=iou, mva=0, truth=None)


def chain_truth():
    """1 x 5 tiles of 6 x 16 (overlap 8) over a 6 x 48 frame: a bar through all five tiles, an instance across the LAST cut only (its smallest id
    lies in tile 3), a one-pixel instance, and an instance wholly inside the seam of tiles 1 and 2 on tile 2's side of the cut (tile 1's label
    for it is visible nowhere in tile 1's core)."""
    truth = np.zeros((6, 48), np.int32)
    truth[0, 1:47] = 1
    truth[2:4, 34:38] = 2        # cut between tiles 3 and 4 is at column 36
    truth[5, 2] = 3
    truth[2:4, 21:23] = 4        # seam of tiles 1 and 2 = columns 16..23, cut at 20
    return truth


def chain_case(mva=0, empty_tile=False):
    from ullsam_amd.utils.mosaic import tile_grid
    grid = tile_grid(6, 48, 16, 8)
    assert grid.ntiles == 5 and grid.col_cuts == (0, 12, 20, 28, 36, 48)
    truth = chain_truth()
    if empty_tile:
        truth[:, 24:48] = 0      # nothing right of column 24: tiles 3 (24..39) and 4 (32..47) are empty
        truth[5, 2] = 0
    tiles, counts = cut(truth, grid, 7)
    return dict(name=f"chain mva={mva} empty={empty_tile}", grid=(6, 48, 16, 8), tiles=tiles, counts=counts, iou=(1, 2), mva=mva, truth=truth)


def cases():
    """Every case of the CPU tests; the GPU tests run the device route on the same ones."""
    out = [
        truth_case("3x3 hand-placed + discs", 150, 170, 64, 16, 1, 40, (3.0, 14.0), hand=True),
        truth_case("5x5 odd tile", 129, 131, 33, 7, 2, 60, (2.0, 9.0), hand=True),
        truth_case("wide overlap", 33, 200, 64, 32, 3, 25, (3.0, 12.0)),
        truth_case("overlap 0, whole tiles", 128, 192, 64, 0, 4, 30, (3.0, 14.0)),
        truth_case("overlap 0, closing tiles pushed back", 200, 96, 64, 0, 9, 30, (3.0, 14.0)),
        truth_case("single tile", 40, 50, 64, 16, 5, 12, (3.0, 9.0)),
        truth_case("single tile, exact", 64, 64, 64, 0, 6, 12, (3.0, 9.0)),
        truth_case("one row more than a tile", 65, 64, 64, 7, 7, 14, (3.0, 9.0)),
        truth_case("min_visible_area", 150, 170, 64, 16, 8, 40, (2.0, 10.0), mva=60),
        threshold_case((1, 2)), threshold_case((501, 1000)), threshold_case((1, 1)),
        chain_case(), chain_case(mva=5), chain_case(empty_tile=True),
    ]
    return out
