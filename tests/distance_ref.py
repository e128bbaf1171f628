"""The definitions of utils.distance as per-pixel loops: every value is a brute-force minimum over ALL pixels of the frame, nothing is separated into
columns and rows.  Shared by tests/test_distance_cpu.py (the host form against these) and tests/test_distance_gpu.py (the kernels' raw outputs)."""
import numpy as np

INF = 2 ** 31 - 1


def _grid(lab):
    h, w = lab.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return ys.reshape(-1).astype(np.int64), xs.reshape(-1).astype(np.int64), lab.reshape(-1).astype(np.int64)


def inner_distance(lab, edge):
    h, w = lab.shape
    ys, xs, ls = _grid(lab)
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            i = int(lab[y, x])
            if i <= 0:
                continue
            d = ((xs - x) ** 2 + (ys - y) ** 2)[ls != i]
            best = int(d.min()) if d.size else INF
            if edge:
                best = min(best, (x + 1) ** 2, (w - x) ** 2, (y + 1) ** 2, (h - y) ** 2)
            out[y, x] = best
    return out


def background_feature(lab, max_distance2=None):
    h, w = lab.shape
    ys, xs, ls = _grid(lab)
    on = ls > 0
    d2 = np.full((h, w), INF, np.int64)
    near = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            d = ((xs - x) ** 2 + (ys - y) ** 2)[on]
            if not d.size:
                continue
            m = int(d.min())
            if max_distance2 is not None and m > max_distance2:
                continue
            d2[y, x] = m
            near[y, x] = int(ls[on][d == m].min())         # the smallest id among ALL minimisers
    return d2, near


def expand_labels(lab, r2):
    d2, near = background_feature(lab)
    out = lab.astype(np.int64).copy()
    for y in range(lab.shape[0]):
        for x in range(lab.shape[1]):
            if lab[y, x] <= 0:
                out[y, x] = near[y, x] if d2[y, x] <= r2 else 0
    return out


def shrink_labels(lab, r2, edge):
    d2 = inner_distance(lab, edge)
    out = np.zeros(lab.shape, np.int64)
    for y in range(lab.shape[0]):
        for x in range(lab.shape[1]):
            if lab[y, x] > 0 and d2[y, x] > r2:
                out[y, x] = lab[y, x]
    return out


def instance_depth(lab, k, edge):
    d2 = inner_distance(lab, edge)
    r2 = np.zeros(k, np.int64)
    xy = np.full((k, 2), -1, np.int64)
    for y in range(lab.shape[0]):                          # row-major: the first pixel that attains the maximum stays
        for x in range(lab.shape[1]):
            i = int(lab[y, x])
            if i > 0 and d2[y, x] > r2[i - 1]:
                r2[i - 1] = d2[y, x]
                xy[i - 1] = (x, y)
    return r2, xy


def column_inner(lab, edge):
    """g [H, W]: the vertical distance of a labelled pixel to the nearest pixel of its column with another label (0xFFFF: none; 0 on the background)."""
    h, w = lab.shape
    g = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            i = lab[y, x]
            if i <= 0:
                continue
            d = [abs(k - y) for k in range(h) if lab[k, x] != i]
            if edge:
                d += [y + 1, h - y]
            g[y, x] = min(d) if d else 0xFFFF
    return g


def column_feature(lab):
    """(g, nearest) [H, W]: the vertical distance to the nearest labelled pixel of the column (0xFFFF: none) and the smallest label at that distance."""
    h, w = lab.shape
    g = np.full((h, w), 0xFFFF, np.int64)
    near = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            d = [(abs(k - y), int(lab[k, x])) for k in range(h) if lab[k, x] > 0]
            if d:
                g[y, x], near[y, x] = min(d)
    return g, near


# ---- label images -------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 17), (23, 1), (2, 2), (5, 40), (40, 7), (13, 13), (23, 23), (31, 18), (40, 40), (17, 33), (8, 9), (3, 29), (36, 25)]


def blobs(seed, h, w, n=None, ids=None):
    """Random discs and bars, later ones on top; ids are drawn from 1..ids with repeats (disconnected instances) and gaps (absent ids)."""
    rng = np.random.default_rng([seed, 0xD157])
    n = int(rng.integers(1, 7)) if n is None else n
    ids = n + 2 if ids is None else ids
    lab = np.zeros((h, w), np.int32)
    ys, xs = np.mgrid[0:h, 0:w]
    for _ in range(n):
        i = int(rng.integers(1, ids + 1))
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        if rng.integers(0, 3) == 0:
            m = (abs(ys - cy) <= rng.uniform(0.5, 3)) & (abs(xs - cx) <= rng.uniform(1, max(w, 2) / 2))
        else:
            m = (ys - cy) ** 2 + (xs - cx) ** 2 <= rng.uniform(0.7, max(min(h, w), 3) / 2.5) ** 2
        lab[m] = i
    return lab


def named_cases():
    """[(name, labels int32 [H, W])]"""
    out = []
    a = np.zeros((9, 11), np.int32)
    a[4, 6] = 1
    out.append(("a one-pixel instance", a))
    out.append(("a frame-filling instance", np.full((7, 10), 1, np.int32)))
    a = np.zeros((7, 16), np.int32)
    a[2:5, 1:5] = 2
    a[2:5, 5:9] = 1
    a[2:5, 9:15] = 2
    out.append(("two pieces of one instance on a row, another label between them", a))
    a = np.zeros((15, 14), np.int32)
    a[2:13, 2:12] = 3
    a[5:10, 5:12] = 0
    out.append(("a C-shaped instance", a))
    out.append(("no labelled pixel", np.zeros((6, 5), np.int32)))
    a = np.zeros((10, 12), np.int32)
    a[1:4, 1:5] = 2
    a[6:9, 6:11] = 5
    out.append(("absent ids", a))
    return out


def cases():
    return [(f"blobs seed {s} {h} x {w}", blobs(s, h, w)) for s, (h, w) in enumerate(SHAPES)] + named_cases()
