"""The definition of utils.raster as plain loops (DESIGN.md "7b, continued (rasterising)"): coordinates snapped with fractions.Fraction, every edge
tested against every row, the crossing point an exact Fraction compared with every pixel centre of the row, one counter per (label, pixel); a
pixel is covered where its counter is odd.  It shares nothing with the numpy form (no A / B, no sort, no spans).  Also the polygon inputs the
tests share.  tests/test_raster_cpu.py holds the numpy form to these loops, tests/test_raster_gpu.py the kernels' raw outputs."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

INT_MAX = 2 ** 31 - 1


def snap(vertices):
    """[(qx, qy)] in 1/256 pixel: floor(v * 256 + 1/2), exactly"""
    return [tuple(math.floor(Fraction(c) * 256 + Fraction(1, 2)) for c in v) for v in np.asarray(vertices).reshape(-1, 2).tolist()]


def ring_edges(start):
    """[(ring, i, j)]: edge i runs from vertex i to vertex j, the last vertex of a ring back to its first"""
    out = []
    for r in range(len(start) - 1):
        s0, s1 = int(start[r]), int(start[r + 1])
        for i in range(s0, s1):
            out.append((r, i, i + 1 if i + 1 < s1 else s0))
    return out


def crossings(q, start, ring_label, h, w):
    """[(edge, label, row, xc, xs)] in edge order, rows ascending: xc = the crossing point (1/256 pixel, a Fraction), xs = the first column whose
    centre is at or right of it (W: none)"""
    out = []
    for r, i, j in ring_edges(start):
        (x0, y0), (x1, y1) = q[i], q[j]
        for y in range(h):
            cy = 256 * y + 128
            if min(y0, y1) <= cy < max(y0, y1):
                xc = x0 + Fraction((cy - y0) * (x1 - x0), y1 - y0)
                xs = w
                for x in range(w):
                    if 256 * x + 128 >= xc:
                        xs = x
                        break
                out.append((i, int(ring_label[r]), y, xc, xs))
    return out


def edge_rows(q, start, h):
    """(row0, cnt) per edge: the first and the number of the rows 0..h - 1 it crosses (row0 = 0 where there is none)"""
    row0, cnt = [], []
    for _, i, j in ring_edges(start):
        rows = [y for y in range(h) if min(q[i][1], q[j][1]) <= 256 * y + 128 < max(q[i][1], q[j][1])]
        assert rows == list(range(rows[0], rows[0] + len(rows))) if rows else True
        row0.append(rows[0] if rows else 0)
        cnt.append(len(rows))
    return row0, cnt


def rasterize(vertices, start, ring_label, size, order="label", num=None):
    """-> SimpleNamespace(labels [H, W], covered [K], area [K], box [K, 4], raw [H, W], rank [K], keys [C] in edge order) of int64 arrays"""
    h, w = size
    q = snap(vertices)
    k = int(max(list(ring_label) + [0])) if num is None else int(num)
    count = np.zeros((k, h, w), np.int64)
    keys = []
    for _, label, y, xc, xs in crossings(q, start, ring_label, h, w):
        keys.append(label << 32 | y << 16 | xs)
        for x in range(w):
            if 256 * x + 128 >= xc:                                   # the centre is at or right of the crossing
                count[label - 1, y, x] += 1
    inside = count % 2 == 1
    covered = inside.sum((1, 2))
    if order == "label":
        rank = list(range(k))
    else:
        rank = [0] * k
        for place, i in enumerate(sorted(range(k), key=lambda i: (-int(covered[i]), i))):
            rank[i] = place
    raw = np.zeros((h, w), np.int64)
    labels = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            on = [i for i in range(k) if inside[i, y, x]]
            if on:
                top = max(on, key=lambda i: rank[i])
                raw[y, x] = rank[top] + 1
                labels[y, x] = top + 1
    area = np.zeros(k, np.int64)
    box = np.tile(np.array([INT_MAX, INT_MAX, -1, -1], np.int64), (k, 1))
    for y in range(h):
        for x in range(w):
            l = labels[y, x] - 1
            if l >= 0:
                area[l] += 1
                box[l] = (min(box[l, 0], x), min(box[l, 1], y), max(box[l, 2], x), max(box[l, 3], y))
    return SimpleNamespace(labels=labels, covered=covered, area=area, box=box, raw=raw, rank=np.array(rank, np.int64).reshape(-1),
                           keys=np.array(keys, np.int64).reshape(-1))


FIELDS = ("labels", "covered", "area", "box")


# ---- polygon inputs -----------------------------------------------------------------------------------------------------------------------------
def rings(*polys):
    """[(label, [(x, y), ...]), ...] -> (vertices float64 [N, 2], start int32 [R + 1], ring_label int32 [R])"""
    verts = [np.asarray(p, np.float64).reshape(-1, 2) for _, p in polys]
    start = np.concatenate([[0], np.cumsum([len(v) for v in verts])]).astype(np.int32)
    return (np.concatenate(verts) if verts else np.zeros((0, 2), np.float64)), start, np.array([l for l, _ in polys], np.int32)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def case(polys, size, order="label", num=None):
    v, s, l = rings(*polys)
    return dict(vertices=v, start=s, ring_label=l, size=size, order=order, num=num)


DIAMOND = [(4.5, .5), (8.5, 4.5), (4.5, 8.5), (.5, 4.5)]


def cut_rectangle(seed=3, h=37, w=41, n=40):
    """The frame cut into two labels by a random polyline of n non-lattice vertices from its top side to its bottom side: every pixel gets exactly one"""
    rng = np.random.default_rng(seed)
    line = np.stack([rng.uniform(1.0, w - 1.0, n), rng.uniform(0.5, h - 0.5, n)], 1)
    line[0, 1], line[-1, 1] = 0.0, float(h)
    left = [(0.0, 0.0)] + [tuple(p) for p in line] + [(0.0, float(h))]
    right = [(float(w), 0.0), (float(w), float(h))] + [tuple(p) for p in line[::-1]]
    return case([(1, left), (2, right)], (h, w))


def cases():
    """{name: dict(vertices, start, ring_label, size, order, num)}: small enough for the loops"""
    out = {}
    out["diamond"] = case([(1, DIAMOND)], (10, 10))
    out["integer rectangle"] = case([(1, rect(2, 3, 7, 8))], (11, 9))
    out["triangle: a vertex on a scanline, one on a centre"] = case([(1, [(1.5, 2.5), (8.0, 4.5), (3.25, 9.0)])], (11, 10))
    hole = rect(4, 4, 8, 9)
    out["hole, same orientation"] = case([(1, rect(1, 1, 12, 12)), (1, hole)], (13, 14))
    out["hole, other orientation"] = case([(1, rect(1, 1, 12, 12)), (1, hole[::-1])], (13, 14))
    out["bow-tie"] = case([(1, [(1, 1), (9, 8), (9, 1), (1, 8)])], (9, 10))
    out["a ring twice cancels"] = case([(1, DIAMOND), (2, rect(1, 1, 4, 3)), (1, DIAMOND)], (10, 10))
    out["out of every side, and outside"] = case([(1, rect(-3.5, 2, 2.5, 5)), (2, rect(4, -4, 7, 2.25)), (3, rect(9.5, 3, 20, 6)), (4, rect(5, 8.5, 8, 15)),
                                                  (5, rect(20, 20, 25, 25)), (6, rect(-9, -9, -2, 40))], (10, 12))
    three = [(1, rect(1, 1, 6, 6)), (2, rect(4, 4, 9, 9)), (3, rect(2, 2, 10, 8))]                  # 1 and 2 cover 25 pixels each: a tie
    out["overlaps, by label"] = case(three, (11, 12), "label")
    out["overlaps, by area"] = case(three, (11, 12), "area")
    out["absent ids"] = case([(2, rect(1, 1, 5, 4)), (5, [(6.2, 6.1), (11.0, 6.4), (10.7, 9.3), (6.5, 8.8)])], (10, 12), num=7)
    out["1 x 1"] = case([(1, rect(-.25, -.25, .75, .75))], (1, 1))
    out["1 x 17"] = case([(1, rect(2, 0, 9, 1)), (2, rect(8.5, -1, 12.5, 3)), (1, [(15.6, 0), (17, 0.2), (16.2, 1)])], (1, 17))
    out["23 x 1"] = case([(2, rect(0, 0, 1, 5)), (1, [(0.1, 7.2), (0.9, 6.9), (0.6, 22.0)])], (23, 1))
    out["no rings"] = case([], (6, 5))
    out["no rings, num = 3"] = case([], (4, 7), num=3)
    out["cut rectangle"] = cut_rectangle()
    return out


def ngon(n, h=48, w=52):
    """A regular n-gon: n edges, most of them shorter than a pixel"""
    t = 2 * np.pi * np.arange(n) / n
    return case([(1, np.stack([w / 2 + (w / 2 - 2.3) * np.cos(t), h / 2 + (h / 2 - 1.7) * np.sin(t)], 1))], (h, w))


def comb(spans, h=300):
    """Teeth two pixels wide over h rows each (the last one shorter), labels 1 and 2 in turn: `spans` spans, 2 * spans crossings"""
    polys, t = [], 0
    while spans > 0:
        rows = min(h, spans)
        polys.append((1 + t % 2, rect(2 * t + .3, 0, 2 * t + 1.7, rows)))
        spans -= rows
        t += 1
    return case(polys, (h, 2 * t + 1))


def long_edge(h=300, w=517, short=500):
    """One edge that spans all h rows next to `short` short ones"""
    i = np.arange(short + 1)
    back = np.stack([200.0 + 30.0 * np.sin(i * 0.7) + 0.37, (h + 3.0) - i * ((h + 5.0) / short)], 1)
    return case([(1, [(5.3, -2.0), (40.7, h + 3.0)] + [tuple(p) for p in back])], (h, w))


def span_cases():
    """Spans of the widths at which a wave of 64 lanes takes one more turn, inside a row and as whole rows"""
    out = {}
    for wd in (63, 64, 65, 130):
        out[f"spans of width {wd}"] = case([(1, rect(3, 1, 3 + wd, 4))], (5, wd + 7))
        out[f"whole rows of width {wd}"] = case([(1, rect(-2, -1, wd + 2, 7))], (5, wd))
    return out
