"""The definition of utils.simplify as plain loops (DESIGN.md "7b, continued (simplifying)"): the loops of tests/outline_ref.py walked edge by edge,
fixed points and candidates pixel by pixel, recursive Douglas-Peucker per arc on fractions.Fraction.  Also the checks of the three facts (tolerance
0, the guarantee, watertightness) and the label images the tests share.  tests/test_simplify_cpu.py holds the host form to these."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from tests import outline_ref as R


def _val(lab, x, y):
    h, w = lab.shape
    return int(lab[y, x]) if 0 <= x < w and 0 <= y < h else 0        # the frame's outside counts as 0


def is_fixed(lab, x, y):
    """At least three of the four pixel sides that meet at the lattice point (x, y) separate different values."""
    a, b, c, d = _val(lab, x - 1, y - 1), _val(lab, x, y - 1), _val(lab, x - 1, y), _val(lab, x, y)
    return (a != b) + (c != d) + (a != c) + (b != d) >= 3


def dist2(p, a, b):
    """The squared distance of p to the segment a b, a Fraction."""
    ux, uy, vx, vy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    length, t = ux * ux + uy * uy, vx * ux + vy * uy
    if length == 0 or t <= 0:
        return Fraction(vx * vx + vy * vy)
    if t >= length:
        return Fraction((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2)
    return Fraction((ux * vy - uy * vx) ** 2, length)


def _peucker(pts, i, j, tol2, keep):
    """pts[i], pts[j] are kept; the candidates strictly between them (j may run past the end: indices are taken modulo len(pts))"""
    n = len(pts)
    best, at = None, None
    for m in range(i + 1, j):
        p = pts[m % n]
        d = dist2(p, pts[i % n], pts[j % n])
        if best is None or d > best or (d == best and (p[1], p[0]) < (pts[at % n][1], pts[at % n][0])):
            best, at = d, m
    if best is not None and best > tol2:
        keep.add(at % n)
        _peucker(pts, i, at, tol2, keep)
        _peucker(pts, at, j, tol2, keep)


def loops(lab, connectivity=8):
    """[(label, candidates [(x, y)], fixed [bool], arcs)] per loop of R.cycles; arcs[j] = the values across the edges from candidate j to the next
    one (cyclic; 0 for the background and the frame's outside), each with its crack: (value, frozenset of the two end points)"""
    ed = R.edges(lab)
    w = lab.shape[1]
    other = ((0, -1), (1, 0), (0, 1), (-1, 0))                         # side -> the pixel across it
    across = lambda e: _val(lab, (e // 4) % w + other[e % 4][0], (e // 4) // w + other[e % 4][1])
    out = []
    for k, cyc in R.cycles(lab, connectivity):
        n = len(cyc)
        fx = [is_fixed(lab, *ed[e][1]) for e in cyc]
        pos = [i for i, e in enumerate(cyc) if cyc[i - 1] % 4 != e % 4 or fx[i]]
        crack = lambda e: (across(e), frozenset(ed[e][1:]))
        arcs = [[crack(cyc[m % n]) for m in range(a, b)] for a, b in zip(pos, pos[1:] + [pos[0] + n])]
        out.append((k, [ed[cyc[i]][1] for i in pos], [fx[i] for i in pos], arcs))
    return out


def simplify(lab, t, connectivity=8, num=None):
    """-> SimpleNamespace(label, start, edges, area2, parent, vertices, loops_of, source: int64 arrays; rings: per SOURCE loop the kept candidate
    indices, before any loop is dropped; cands: per source loop its candidates; arcs).  t = the tolerance in 1/256 pixel."""
    lab = np.asarray(lab)
    src = R.outlines(lab, connectivity, num)
    tol2 = Fraction(t * t, 65536)
    rings, cands, arcs_of = [], [], []
    for k, cand, fixed, arcs in loops(lab, connectivity):
        n = len(cand)
        keep = {i for i in range(n) if fixed[i]}
        if not keep:
            first = min(range(n), key=lambda i: (cand[i][1], cand[i][0]))
            far = max(range(n), key=lambda i: ((cand[i][0] - cand[first][0]) ** 2 + (cand[i][1] - cand[first][1]) ** 2, -cand[i][1], -cand[i][0]))
            keep = {first, far}
        base = sorted(keep)
        for a, b in zip(base, base[1:] + [base[0] + n]):
            _peucker(cand, a, b, tol2, keep)
        rings.append(sorted(keep))
        cands.append(cand)
        arcs_of.append(arcs)
    area2 = []
    for cand, ring in zip(cands, rings):
        pts = [cand[i] for i in ring]
        area2.append(sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(pts, pts[1:] + pts[:1])))
    ok = [len(r) >= 3 and a != 0 and (a > 0) == (s > 0) for r, a, s in zip(rings, area2, src.area2)]
    ok = [o and ok[int(src.parent[i])] for i, o in enumerate(ok)]
    source = [i for i, o in enumerate(ok) if o]
    new = {i: j for j, i in enumerate(source)}
    verts, start = [], [0]
    for i in source:
        verts += [cands[i][j] for j in rings[i]]
        start.append(len(verts))
    loops_of = np.zeros(len(src.loops_of), np.int64)
    for i in source:
        loops_of[src.label[i] - 1] += 1
    i64 = lambda v, *s: np.array(v, np.int64).reshape(*s)
    return SimpleNamespace(label=src.label[source] if source else i64([], -1), start=i64(start, -1), edges=src.edges[source] if source else i64([], -1),
                           area2=i64([area2[i] for i in source], -1), parent=i64([new[int(src.parent[i])] for i in source], -1),
                           vertices=i64(verts, -1, 2), loops_of=loops_of, source=i64(source, -1), rings=rings, cands=cands, arcs=arcs_of, src=src)


# ---- the facts ----------------------------------------------------------------------------------------------------------------------------------
def _rows(out):
    a = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.int64)
    start, verts = a(out.start), a(out.vertices).reshape(-1, 2)
    return [[tuple(int(c) for c in v) for v in verts[start[i]:start[i + 1]]] for i in range(len(start) - 1)]


def without_collinear(ring):
    n = len(ring)
    cross = lambda p, q, r: (q[0] - p[0]) * (r[1] - q[1]) - (q[1] - p[1]) * (r[0] - q[0])
    return [ring[i] for i in range(n) if cross(ring[i - 1], ring[i], ring[(i + 1) % n]) != 0]


def check_tolerance_zero(res, lab, connectivity):
    """Fact 1: nothing is dropped, and without the collinear vertices every ring is label_outlines' ring."""
    src = R.outlines(lab, connectivity)
    got, want = _rows(res.outlines), _rows(src)
    assert len(got) == len(want) and [without_collinear(r) for r in got] == want
    assert np.asarray(res.source.cpu() if hasattr(res.source, "cpu") else res.source).tolist() == list(range(len(want)))
    a = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.int64)
    for f in ("label", "edges", "area2", "parent", "loops_of"):
        assert np.array_equal(a(getattr(res.outlines, f)), getattr(src, f)), f


def check_guarantee(res, ref, t):
    """Fact 2: every candidate of a surviving source loop lies within the tolerance of its simplified ring."""
    tol2 = Fraction(t * t, 65536)
    source = np.asarray(res.source.cpu() if hasattr(res.source, "cpu") else res.source).tolist()
    for ring, s in zip(_rows(res.outlines), source):
        segs = list(zip(ring, ring[1:] + ring[:1]))
        for p in ref.cands[s]:
            assert min(dist2(p, a, b) for a, b in segs) <= tol2, (s, p)


def check_watertight(ref, lab):
    """Fact 3, on the rings before any loop is dropped: a ring segment whose source arc borders a label (not the background, not the frame's outside)
    has exactly one partner, in another ring: the segment with the same cracks as its source arc, and that one is the same chord reversed.  -> the
    number of such segments."""
    held, need = {}, []
    for i, (cand, ring, arcs) in enumerate(zip(ref.cands, ref.rings, ref.arcs)):
        n = len(cand)
        for a, b in zip(ring, ring[1:] + [ring[0] + n]):
            arc = [v for m in range(a, b) for v in arcs[m % n]]
            cracks, seg = frozenset(c for _, c in arc), (cand[a], cand[b % n])
            held.setdefault(cracks, []).append((i, seg))
            assert len({v for v, _ in arc}) == 1, "an arc between two kept candidates borders one value"
            if arc[0][0] != 0:
                need.append((i, seg, cracks))
    for i, (p, q), cracks in need:
        assert len(held[cracks]) == 2 and [s for j, s in held[cracks] if j != i] == [(q, p)], (i, p, q)
    return len(need)


def segments_of(res):
    """{directed segment: how many rings hold it} of an Outlines-like result"""
    count = {}
    for ring in _rows(res):
        for seg in zip(ring, ring[1:] + ring[:1]):
            count[seg] = count.get(seg, 0) + 1
    return count


def check_reversal(res, h, w):
    """Fact 3 on a label image without background: every directed segment of a ring that does not lie on the frame's border occurs reversed in exactly
    one other ring."""
    count = segments_of(res)
    on_border = lambda p, q: (p[0] == q[0] and p[0] in (0, w)) or (p[1] == q[1] and p[1] in (0, h))
    inner = 0
    for (p, q), c in count.items():
        if not on_border(p, q):
            assert c == 1 and count.get((q, p), 0) == 1, (p, q)
            inner += 1
    return inner


# ---- label images -------------------------------------------------------------------------------------------------------------------------------
def images():
    """{name: labels int32 [H, W]}: the cases the simplifier adds to outline_ref.shapes()"""
    out = {}
    a = np.zeros((9, 12), np.int32)                       # label 1 runs straight through the junction of 2 and 3 below it
    a[1:4, 1:11] = 1
    a[4:8, 1:6] = 2
    a[4:8, 6:11] = 3
    out["a T-junction passed straight"] = a
    a = np.zeros((14, 44), np.int32)
    for x in range(2, 42):
        top = 6 + (1 if (x // 3) % 2 else 0) + (2 if 18 <= x < 24 else 0)
        a[1:top, x] = 1
        a[top:13, x] = 2
    out["two labels on a wavy border"] = a
    rng = np.random.default_rng(21)
    seeds = rng.integers(0, 40, (7, 2))
    ys, xs = np.mgrid[0:41, 0:39]
    d = (ys[..., None] - seeds[:, 0]) ** 2 + (xs[..., None] - seeds[:, 1]) ** 2 + rng.integers(0, 12, (41, 39, 7))    # (wavy borders, every label in one piece)
    out["a tiling without background 41 x 39"] = (np.argmin(d, -1) + 1).astype(np.int32)
    a = np.zeros((9, 9), np.int32)                        # corners (8, 2), (6, 6), (2, 8) are equally far (50) from the first anchor (1, 1)
    a[1, 1:8] = 1
    a[1:6, 1:6] = 1
    a[1:8, 1] = 1
    out["tied farthest anchors"] = a
    a = np.zeros((8, 8), np.int32)                        # two squares of one label that touch at a corner: with connectivity 4 each loop has the
    a[1:4, 1:4] = 1                                       # saddle as its single fixed point (L = 0)
    a[4:7, 4:7] = 1
    out["loops with one fixed point"] = a
    a = np.zeros((6, 14), np.int32)                       # a bump of height 1 on a long side
    a[1:4, 1:13] = 1
    a[4, 6:8] = 1
    out["a bump at distance 1"] = a
    a = np.zeros((8, 16), np.int32)                       # two bumps of the same height on the border of 1 and 2
    a[1:4, 1:15] = 1
    a[4:7, 1:15] = 2
    a[4, 4:6] = 1
    a[4, 10:12] = 1
    out["two equal bumps on a shared border"] = a
    a = np.zeros((10, 12), np.int32)                      # an L whose arm ends lie beyond the chord's ends
    a[1:9, 1:3] = 1
    a[7:9, 1:11] = 1
    a[4:6, 3:5] = 1
    out["candidates beyond the chord's ends"] = a
    a = np.zeros((5, 6), np.int32)
    a[2, 2:4] = 1
    out["a 2 x 1 cell"] = a
    a = np.zeros((9, 10), np.int32)                       # a thin ring: at tolerance 2 the outer loop collapses and takes the hole along
    a[2:5, 2:8] = 1
    a[3, 3:7] = 0
    out["a hole whose parent drops"] = a
    a = np.zeros((12, 16), np.int32)                      # label 1 sits on the straight border of 2 and 3 and holds 4, 5, 6 in its hole: at 7 px its
    a[8:10, 0:8], a[8:10, 8:16] = 2, 3                    # outer ring is three collinear fixed points (area2 = 0), while the hole keeps its three
    a[2:8, 3:13] = 1                                      # junctions (7, 5), (8, 6), (9, 5), a valid ring: only the parent rule removes it
    a[4, 7:9], a[5, 7], a[5, 8] = 4, 5, 6
    out["a valid hole whose parent drops"] = a
    return out


def three_collinear():
    """A bump of label 1 on the straight border of 2 and 3: its loop has three fixed points, all on that line; at a tolerance of 2 pixels the ring
    is those three (area2 = 0)."""
    a = np.zeros((6, 12), np.int32)
    a[3:5, 0:6] = 2
    a[3:5, 6:12] = 3
    a[2, 3:9] = 1
    return a


def all_images():
    out = dict(R.shapes())
    out.update(images())
    out["three collinear fixed points"] = three_collinear()
    return out
