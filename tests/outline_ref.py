"""The definition of utils.outline as plain loops (DESIGN.md "7b, continued (outlines)"): a dict of directed unit edges, the successor of an edge
by "the edges of k that start at its head", the cycles walked one by one, parents by the walk to the left.  Also fill(), the inverse operation
(polygon loops -> label image; tests only), and the label images the tests share.  tests/test_outline_cpu.py holds the host form to these,
tests/test_outline_gpu.py the kernels' raw outputs."""
from types import SimpleNamespace

import numpy as np

# side -> (tail, head) offsets from the pixel's top-left corner; the instance lies on the right of travel (y points down)
TAIL = ((0, 0), (1, 0), (1, 1), (0, 1))
HEAD = ((1, 0), (1, 1), (0, 1), (0, 0))


def _lab(lab, x, y):
    h, w = lab.shape
    return int(lab[y, x]) if 0 <= x < w and 0 <= y < h else -1       # the frame's outside is "not k"


def side_masks(lab):
    """mask [H, W]: bit s is set where side s of a labelled pixel faces a pixel that is not of its label."""
    h, w = lab.shape
    mask = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            k = int(lab[y, x])
            if k > 0:
                for s, (dx, dy) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0))):
                    if _lab(lab, x + dx, y + dy) != k:
                        mask[y, x] |= 1 << s
    return mask


def edges(lab):
    """{edge id: (label, tail, head)} in id order"""
    h, w = lab.shape
    mask = side_masks(lab)
    out = {}
    for y in range(h):
        for x in range(w):
            for s in range(4):
                if mask[y, x] >> s & 1:
                    out[4 * (y * w + x) + s] = (int(lab[y, x]), (x + TAIL[s][0], y + TAIL[s][1]), (x + HEAD[s][0], y + HEAD[s][1]))
    return out


def successors(lab, connectivity):
    """{edge id: the id of its successor}"""
    ed = edges(lab)
    starts = {}
    for e, (k, t, _) in ed.items():
        starts.setdefault((k, t), []).append(e)
    succ = {}
    for e, (k, _, hd) in ed.items():
        cand = starts[(k, hd)]
        if len(cand) == 1:
            succ[e] = cand[0]
        else:                                                         # a saddle: the left turn (8) or the right turn (4)
            assert len(cand) == 2
            want = (e % 4 + (3 if connectivity == 8 else 1)) % 4
            (succ[e],) = [c for c in cand if c % 4 == want]
    assert sorted(succ.values()) == sorted(ed)                        # a permutation
    return succ


def cycles(lab, connectivity):
    """[(label, [edge ids from the leader on])] ordered by (label, leader)"""
    ed = edges(lab)
    succ = successors(lab, connectivity)
    seen, out = set(), []
    for e in sorted(ed):                                              # the first edge met of a cycle is its smallest: the leader
        if e in seen:
            continue
        cyc, c = [], e
        while c not in seen:
            seen.add(c)
            cyc.append(c)
            c = succ[c]
        assert c == e
        out.append((ed[e][0], cyc))
    out.sort(key=lambda t: (t[0], t[1][0]))
    return out


def leader_rank(lab, connectivity):
    """({edge id: leader id}, {edge id: steps from the leader})"""
    lead, rank = {}, {}
    for _, cyc in cycles(lab, connectivity):
        for i, e in enumerate(cyc):
            lead[e], rank[e] = cyc[0], i
    return lead, rank


def outlines(lab, connectivity=8, num=None):
    """-> SimpleNamespace(label [L], start [L + 1], edges [L], area2 [L], parent [L], vertices [N, 2], loops_of [K]) of int64 arrays"""
    lab = np.asarray(lab)
    h, w = lab.shape
    k_max = int(max(lab.max(), 0)) if num is None else int(num)
    ed = edges(lab)
    cyc = cycles(lab, connectivity)
    loop_of_edge = {e: i for i, (_, c) in enumerate(cyc) for e in c}
    label, start, count, area2, verts = [], [0], [], [], []
    for k, c in cyc:
        a = 0
        for e in c:
            (xt, yt), (xh, yh) = ed[e][1], ed[e][2]
            a += xt * yh - xh * yt
        n = len(c)
        for i, e in enumerate(c):                                     # corners: the predecessor runs in another direction
            if c[i - 1] % 4 != e % 4:
                verts.append(ed[e][1])
        label.append(k)
        count.append(n)
        area2.append(a)
        start.append(len(verts))
    parent = []
    for i, (k, c) in enumerate(cyc):
        j = i
        while area2[j] <= 0:
            p = cyc[j][1][0] // 4
            x, y = p % w, p // w
            while x > 0 and lab[y, x - 1] == k:
                x -= 1
            j = loop_of_edge[4 * (y * w + x) + 3]
        parent.append(j)
    loops_of = np.zeros(k_max, np.int64)
    for k in label:
        loops_of[k - 1] += 1
    i64 = lambda v, *s: np.array(v, np.int64).reshape(*s)
    return SimpleNamespace(label=i64(label, -1), start=i64(start, -1), edges=i64(count, -1), area2=i64(area2, -1), parent=i64(parent, -1),
                           vertices=i64(verts, -1, 2), loops_of=loops_of)


FIELDS = ("label", "start", "edges", "area2", "parent", "vertices", "loops_of")


def fill(out, h, w):
    """The label image of polygon loops: every vertical segment adds +label at its column over the rows it spans when it runs north and -label
    when it runs south; a cumulative sum along each row does the rest."""
    a = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v).astype(np.int64)
    label, start, verts = a(out.label), a(out.start), a(out.vertices)
    d = np.zeros((h, w + 1), np.int64)
    for i, k in enumerate(label):
        ring = verts[start[i]:start[i + 1]]
        for j in range(len(ring)):
            (x0, y0), (x1, y1) = ring[j], ring[(j + 1) % len(ring)]
            if x0 == x1 and y1 < y0:
                d[y1:y0, x0] += k
            elif x0 == x1 and y1 > y0:
                d[y0:y1, x0] -= k
    return np.cumsum(d, 1)[:, :w]


# ---- label images -------------------------------------------------------------------------------------------------------------------------------
def spiral(n=64):
    """A one-pixel corridor that winds inwards, walls of one pixel between its turns: one loop of several thousand edges."""
    lab = np.zeros((n, n), np.int32)
    x, y, dx, dy = 1, 1, 1, 0
    lab[y, x] = 1
    while True:
        moved = False
        for _ in range(2):
            nx, ny = x + dx, y + dy
            ax, ay = x + 2 * dx, y + 2 * dy                          # the pixel after the next one: stop one short of an older turn
            ok = 1 <= nx < n - 1 and 1 <= ny < n - 1 and lab[ny, nx] == 0 and not (0 <= ax < n and 0 <= ay < n and lab[ay, ax] == 1)
            if ok:
                x, y = nx, ny
                lab[y, x] = 1
                moved = True
                break
            dx, dy = -dy, dx                                          # turn right
        if not moved:
            return lab


def shapes():
    """{name: labels int32 [H, W]}"""
    out = {}
    ys, xs = np.mgrid[0:33, 0:31]
    out["checkerboard 33 x 31"] = ((ys + xs) % 2 == 0).astype(np.int32)
    out["noise 24 x 31"] = np.random.default_rng(5).integers(0, 3, (24, 31)).astype(np.int32)
    out["noise 9 x 11"] = np.random.default_rng(6).integers(0, 3, (9, 11)).astype(np.int32)
    a = np.zeros((9, 9), np.int32)
    a[1:8, 1:8] = 1
    a[2:7, 2:7] = 0
    a[3:6, 3:6] = 1
    a[4, 4] = 2
    out["nested rings 9 x 9"] = a
    out["spiral 64 x 64"] = spiral(64)
    a = np.zeros((12, 40), np.int32)
    a[1:6, 2:38] = 1
    a[6:11, 2:38] = 2
    out["two labels on one long border"] = a
    a = np.zeros((15, 14), np.int32)
    a[2:13, 2:12] = 3
    a[5:10, 5:12] = 0
    out["a C shape"] = a
    out["a frame-filling instance 7 x 10"] = np.full((7, 10), 1, np.int32)
    out["1 x 1"] = np.ones((1, 1), np.int32)
    a = np.zeros((1, 17), np.int32)
    a[0, 2:9] = 1
    a[0, 9:12] = 2
    a[0, 16] = 1
    out["1 x 17"] = a
    a = np.zeros((23, 1), np.int32)
    a[0:5, 0] = 2
    a[7:22, 0] = 1
    out["23 x 1"] = a
    out["an empty frame"] = np.zeros((6, 5), np.int32)
    a = np.zeros((10, 12), np.int32)
    a[1:4, 1:5] = 2
    a[6:9, 6:11] = 5
    out["absent ids"] = a
    a = np.random.default_rng(8).integers(0, 4, (7, 9)).astype(np.int32)
    assert a.size % 4 != 0
    out["H * W no multiple of 4"] = a
    return out
