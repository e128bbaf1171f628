"""The stack linking of utils.stack as plain loops: per-pixel counting into dictionaries, fractions.Fraction for the ranking, a dictionary
union-find -- no code shared with ullsam_amd/utils/stack.py -- and the case list of tests/test_stack_cpu.py and tests/test_stack_gpu.py."""
from fractions import Fraction

import numpy as np

INT_MAX = 2 ** 31 - 1


def bases(counts):
    base = [0]
    for k in counts:
        base.append(base[-1] + int(k))
    return base


def pixel_counts(planes, counts):
    """One pass over the pixels: (areas {g: pixels}, pairs {(g_a, g_b): pixels} over consecutive planes, boxes {g: [x0, y0, x1, y1]})."""
    base = bases(counts)
    rows = np.asarray(planes).tolist()
    areas, pairs, boxes = {}, {}, {}
    for z, plane in enumerate(rows):
        nxt = rows[z + 1] if z + 1 < len(rows) else None
        for y, row in enumerate(plane):
            nrow = nxt[y] if nxt is not None else None
            for x, a in enumerate(row):
                if not a:
                    continue
                assert 0 < a <= counts[z]
                ga = base[z] + a
                areas[ga] = areas.get(ga, 0) + 1
                bx = boxes.get(ga)
                if bx is None:
                    boxes[ga] = [x, y, x, y]
                else:
                    if x < bx[0]: bx[0] = x
                    if x > bx[2]: bx[2] = x
                    bx[3] = y                            # (rows ascend)
                if nrow is not None and nrow[x]:
                    key = (ga, base[z + 1] + nrow[x])
                    pairs[key] = pairs.get(key, 0) + 1
    return areas, pairs, boxes


def plane_of(g, base):
    z = 0
    while base[z + 1] < g:
        z += 1
    return z


def rank_key(n, u, partner):
    """Larger is better: the IoU as an exact fraction, then the SMALLER partner id."""
    return (Fraction(n, u), -partner)


def link(planes, counts, iou, mode="mutual", min_planes=1, min_volume=0, stats=None):
    """-> (volume, label_of_global, voxels, zrange, boxes, info): the definition of utils.stack.link_label_stack, step by step."""
    planes = np.asarray(planes)
    Z, H, W = planes.shape
    base = bases(counts)
    G = base[-1]
    areas, pairs, boxes_g = stats if stats is not None else pixel_counts(planes, counts)
    num, den = iou
    cands = {}
    for (a, b), n in pairs.items():
        u = areas[a] + areas[b] - n
        if n > 0 and n * den >= num * u:
            cands[(a, b)] = (n, u)
    succ, pred = {}, {}
    for (a, b), (n, u) in cands.items():
        if a not in succ or rank_key(n, u, b) > rank_key(*cands[(a, succ[a])], succ[a]):
            succ[a] = b
        if b not in pred or rank_key(n, u, a) > rank_key(*cands[(pred[b], b)], pred[b]):
            pred[b] = a
    if mode == "mutual":
        links = [(a, b) for (a, b) in cands if succ[a] == b and pred[b] == a]
    else:
        assert mode == "all"
        links = list(cands)
    parent = {g: g for g in range(1, G + 1)}

    def find(g):
        while parent[g] != g:
            g = parent[g]
        return g

    for a, b in links:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    rep = {g: find(g) for g in range(1, G + 1)}
    vox, zr, bx = {}, {}, {}
    for g, n in areas.items():
        r, z = rep[g], plane_of(g, base)
        vox[r] = vox.get(r, 0) + n
        lo, hi = zr.get(r, (z, z))
        zr[r] = (min(lo, z), max(hi, z))
        b = bx.get(r, [INT_MAX, INT_MAX, -1, -1])
        g_box = boxes_g[g]
        bx[r] = [min(b[0], g_box[0]), min(b[1], g_box[1]), max(b[2], g_box[2]), max(b[3], g_box[3])]
    final = {}
    for r in sorted(vox):
        if vox[r] != 0 and vox[r] >= min_volume and zr[r][1] - zr[r][0] + 1 >= min_planes:
            final[r] = len(final) + 1
    log = np.zeros(G + 1, np.int32)
    for g in range(1, G + 1):
        log[g] = final.get(rep[g], 0)
    volume = np.zeros((Z, H, W), np.int32)
    for z, plane in enumerate(planes.tolist()):
        lut = [0] + [int(log[base[z] + l]) for l in range(1, counts[z] + 1)]
        volume[z] = np.asarray([[lut[v] for v in row] for row in plane], np.int32).reshape(H, W)
    order = sorted(final, key=final.get)
    voxels = np.asarray([vox[r] for r in order], np.int64).reshape(-1)
    zrange = np.asarray([zr[r] for r in order], np.int32).reshape(-1, 2)
    boxes = np.asarray([bx[r] for r in order], np.int32).reshape(-1, 4)
    info = {"G": G, "candidates": len(cands), "links": len(links), "succ": succ, "pred": pred, "rep": rep, "K": len(final)}
    return volume, log, voxels, zrange, boxes, info


def table(log, counts):
    """track_table by loops: [K, Z]."""
    base = bases(counts)
    K = int(max(log)) if len(log) else 0
    out = np.zeros((K, len(counts)), np.int32)
    for z, k in enumerate(counts):
        for l in range(1, k + 1):
            o = int(log[base[z] + l])
            if o:
                assert out[o - 1, z] == 0
                out[o - 1, z] = l
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def case(name, planes, counts, iou=(1, 4), min_planes=1, min_volume=0):
    planes = np.ascontiguousarray(np.asarray(planes, np.int32))
    assert planes.ndim == 3 and len(counts) == planes.shape[0]
    return {"name": name, "planes": planes, "counts": [int(k) for k in counts], "iou": iou, "min_planes": min_planes, "min_volume": min_volume}


def _row_case(name, rows, counts, iou, width=None, **kw):
    """Planes of ONE row each, given as lists of (first column, length, id)."""
    width = width or max(x + n for row in rows for x, n, _ in row)
    planes = np.zeros((len(rows), 1, width), np.int32)
    for z, row in enumerate(rows):
        for x, n, v in row:
            planes[z, 0, x:x + n] = v
    return case(name, planes, counts, iou, **kw)


# (n, u) of the two candidates of one label: the cross-products differ by 1 -- 3000 * 10864 - 3833 * 8503 = 1, so 3000 / 8503 is the LARGER
# IoU -- and the float32 quotients coincide.  The exact winner carries the larger id, so equal floats broken by the smaller id pick the loser.
EXACT = ((3833, 10864), (3000, 8503))
# a pair of this kind just above 1 / 2, (4096, 8191) against (4097, 8193): 4096 * 8193 - 4097 * 8191 = 1.  Both lie above 1 / 2, so no image holds them
# as two candidates of one label (n1 + n2 <= A <= u1); the ranking is tested with them on hand-made tables.
EXACT_TABLE = ((4096, 8191), (4097, 8193))


def exact_ranking_case(swap=False):
    """128 x 192: plane 0 holds one label a on the first A pixels in raster order; plane 1 holds b1 on a's first n1 pixels and b2 on its next n2
    pixels, both continued outside a up to the unions of EXACT.  swap: the same plane 1 under plane 0 (the ranking on the predecessor side)."""
    (n1, u1), (n2, u2) = EXACT
    A = n1 + n2
    e1, e2 = u1 - A, u2 - A
    H, W = 128, 192
    assert A + e1 + e2 <= H * W
    p0, p1 = np.zeros(H * W, np.int32), np.zeros(H * W, np.int32)
    p0[:A] = 1
    p1[:n1] = 1
    p1[n1:A] = 2
    p1[A:A + e1] = 1
    p1[A + e1:A + e1 + e2] = 2
    planes = [p1.reshape(H, W), p0.reshape(H, W)] if swap else [p0.reshape(H, W), p1.reshape(H, W)]
    return case("exact ranking" + (" (predecessor side)" if swap else ""), planes, [2, 1] if swap else [1, 2], (1, 4))


def hand_cases():
    out = []
    # ties: both IoUs are exactly 2 / 4
    out.append(_row_case("tie on the successor side", [[(0, 4, 1)], [(0, 2, 1), (2, 2, 2)]], [1, 2], (1, 2)))
    out.append(_row_case("tie on the predecessor side", [[(0, 2, 1), (2, 2, 2)], [(0, 4, 1)]], [2, 1], (1, 2)))
    # threshold (1, 3): 6 and 6 pixels sharing 3 -> n * den = 9 = num * u; one shared pixel fewer in b -> 2 * 3 = 6 < 9
    out.append(_row_case("threshold equality", [[(0, 6, 1)], [(3, 6, 1)]], [1, 1], (1, 3)))
    out.append(_row_case("threshold one pixel below", [[(0, 6, 1)], [(4, 5, 1)]], [1, 1], (1, 3)))
    # no second choice.  plane 0: a = 1 on 0..19, a2 = 2 on 20..59; plane 1: b' = 2 on 0..11, b = 1 on 12..27.  IoUs: (a, b') 12 / 20, (a, b) 8 / 28,
    # (a2, b) 8 / 48, all >= 1 / 8.  b's best is a, a's best is b', a2's only candidate is b: b stays unlinked, a2 too.
    out.append(_row_case("no second choice", [[(0, 20, 1), (20, 40, 2)], [(0, 12, 2), (12, 16, 1)]], [2, 2], (1, 8), width=64))
    out.append(exact_ranking_case())
    out.append(exact_ranking_case(swap=True))
    # vanish and reappear: the same footprint in planes 0 and 2, nothing in plane 1 (which still declares an id)
    blob = np.zeros((3, 5, 9), np.int32)
    blob[0, 1:4, 2:6] = 1
    blob[2, 1:4, 2:6] = 1
    out.append(case("vanish and reappear", blob, [1, 1, 1], (1, 2)))
    # degenerate shapes
    one = np.zeros((1, 7, 70), np.int32)
    one[0, 1:3, 5:69] = 3
    one[0, 4:6, 0:9] = 1
    out.append(case("Z = 1, absent ids", one, [4], (1, 4)))
    mid = np.zeros((3, 6, 10), np.int32)
    mid[0, 1:4, 1:5] = 2
    mid[2, 1:4, 1:5] = 1
    out.append(case("an empty plane with K = 0 in the middle", mid, [2, 0, 1], (1, 4)))
    out.append(case("nothing at all", np.zeros((2, 3, 5), np.int32), [0, 0], (1, 4)))
    for w in (63, 64, 65, 130):                          # one label filling whole rows: runs that go on over 64-pixel segments and end with the row
        full = np.zeros((3, 4, w), np.int32)
        full[0, 0:3] = 1
        full[1, 1:4] = 2
        full[2, 2:3] = 1
        full[2, 3, : w // 2] = 2
        out.append(case(f"whole rows, width {w}", full, [1, 2, 2], (1, 4)))
    cross = np.zeros((2, 3, 130), np.int32)              # runs that cross a segment end and run into the row's end, the next row starting with another id
    cross.reshape(2, -1)[0, 50:150] = 1
    cross.reshape(2, -1)[0, 150:280] = 2
    cross.reshape(2, -1)[1, 60:200] = 2
    cross.reshape(2, -1)[1, 200:390] = 1
    out.append(case("runs crossing segment and row ends", cross, [2, 3], (1, 4)))
    # min_planes / min_volume: A = 3 planes x 3 pixels, B = 1 plane x 20 pixels, C = 2 planes x 3 pixels
    drop = np.zeros((4, 6, 12), np.int32)
    for z in (0, 1, 2):
        drop[z, 0, 0:3] = z + 1                          # A (ids 1, 2, 3 in the three planes)
    drop[1, 2:4, 0:10] = 1                               # B
    drop[2, 5, 4:7] = 1                                  # C
    drop[3, 5, 4:7] = 2
    counts = [1, 2, 3, 2]
    out.append(case("drops: none", drop, counts, (1, 2)))
    out.append(case("drops: min_planes", drop, counts, (1, 2), min_planes=2))
    out.append(case("drops: min_volume", drop, counts, (1, 2), min_volume=7))
    out.append(case("drops: both", drop, counts, (1, 2), min_planes=2, min_volume=7))
    return out


# (seed, Z, H, W, n, r_range, dz, iou).  What the loops above find in them (tests/test_stack_cpu.py asserts the two conditions the list has to meet:
# some candidate that mutual leaves unlinked, and some case with fewer objects under "all" than under "mutual"):
#   seed 3, 5 x 96 x 130, (1, 2):   G = 168,  98 candidates,  98 links,                K =  63 under mutual and under all (at 1 / 2 nothing competes)
#   seed 4, 6 x 70 x 200, (1, 4):   G = 308, 223 candidates, 217 links,  6 unlinked,   K =  74 under mutual,  69 under all
#   seed 4, 9 x 200 x 300, (1, 3):  G = 912, 570 candidates, 563 links,  7 unlinked,   K = 220 under mutual, 214 under all
#   seed 1, 6 x 300 x 520, (1, 4):  G = 1372, 980 candidates, 972 links, 8 unlinked,   K = 286 under mutual, 280 under all
SPHERES = ((3, 5, 96, 130, 40, (6.0, 18.0), 3.0, (1, 2)),
           (4, 6, 70, 200, 60, (5.0, 16.0), 2.5, (1, 4)),
           (4, 9, 200, 300, 150, (4.0, 30.0), 4.0, (1, 3)))
LARGE = (1, 6, 300, 520, 260, (4.0, 26.0), 3.0, (1, 4))      # the GPU's "many workgroups" case: 75 x 6 workgroups per pass


def sphere_case(seed, Z, H, W, n, r_range, dz, iou, **kw):
    from ullsam_amd.utils import synthetic as S
    planes, counts = S.label_stack(seed, Z, H, W, n, r_range, dz)
    return case(f"spheres seed {seed} {Z} x {H} x {W}", planes, counts, iou, **kw)


def cases():
    out = hand_cases() + [sphere_case(*s) for s in SPHERES]
    out.append(dict(out[-2], name=out[-2]["name"] + ", min_planes 2, min_volume 150", min_planes=2, min_volume=150))
    return out
