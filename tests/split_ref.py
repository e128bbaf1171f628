"""The definition of utils.split.split_labels as plain per-pixel loops over Python integers: nothing is vectorised, the distance map is the brute-force
one of tests/distance_ref.py.  Shared by tests/test_split_cpu.py (the host form against these) and tests/test_split_gpu.py (the kernels' raw outputs)."""
import numpy as np

from tests import distance_ref as R

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
FORWARD = [(0, 1), (1, -1), (1, 0), (1, 1)]               # every 8-adjacent pixel pair once


def shallow(p, s, h):
    """sqrt(p) - sqrt(s) <= h, exactly."""
    t = p - s - h * h
    return t <= 0 or t * t <= 4 * h * h * s


def ascent(lab, d2):
    """up [H * W] (Python ints): the pixel of greatest (d2, -index) among p and its 8 neighbours with p's label; p itself on the background."""
    h, w = lab.shape
    up = list(range(h * w))
    for y in range(h):
        for x in range(w):
            if lab[y, x] <= 0:
                continue
            best = (int(d2[y, x]), -(y * w + x))
            for dy, dx in NEIGHBOURS:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and lab[yy, xx] == lab[y, x]:
                    best = max(best, (int(d2[yy, xx]), -(yy * w + xx)))
            up[y * w + x] = -best[1]
    return up


def roots(up):
    """[H * W]: the root every chain reaches."""
    out = []
    for p in range(len(up)):
        while up[p] != p:
            p = up[p]
        out.append(p)
    return out


def passes(lab, d2, root):
    """{(a, b): S} for the basins a < b of one label that touch."""
    h, w = lab.shape
    out = {}
    for y in range(h):
        for x in range(w):
            if lab[y, x] <= 0:
                continue
            for dy, dx in FORWARD:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and lab[yy, xx] == lab[y, x]:
                    a, b = root[y * w + x], root[yy * w + xx]
                    if a != b:
                        k = (min(a, b), max(a, b))
                        out[k] = max(out.get(k, 0), min(int(d2[y, x]), int(d2[yy, xx])))
    return out


def merge_round(edges, d2f, rep, h):
    """edges {(a, b): S}, rep[p] = the representative of p's component at the round's start -> {X: Y}: the absorptions of one round."""
    best = {}
    for (a, b), s in edges.items():
        x, y = rep[a], rep[b]
        if x != y:
            best[x] = max(best.get(x, (-1, 0)), (s, -y))
            best[y] = max(best.get(y, (-1, 0)), (s, -x))
    out = {}
    for x, (s, ny) in best.items():
        y = -ny
        if (int(d2f[x]), -x) < (int(d2f[y]), -y) and shallow(int(d2f[x]), s, h):
            out[x] = y
    return out


def split(lab, h, edge=False, k=None):
    """-> (labels [H, W], parent [K'], peak_r2 [K'], peak_xy [K', 2], parts_of [K], rounds), all int64."""
    hh, w = lab.shape
    k = max(int(lab.max()), 0) if k is None else k
    d2 = R.inner_distance(lab, edge)
    d2f = [int(v) for v in d2.reshape(-1)]
    labf = [int(v) for v in lab.reshape(-1)]
    rep = roots(ascent(lab, d2))
    edges = passes(lab, d2, rep)
    rounds = 0
    while True:
        move = merge_round(edges, d2f, rep, h)
        if not move:
            break
        up = list(rep)
        for x, y in move.items():
            up[x] = y
        rep = roots(up)
        rounds += 1
    reps = sorted({rep[p] for p in range(hh * w) if labf[p] > 0}, key=lambda r: (labf[r], r))
    newid = {r: i + 1 for i, r in enumerate(reps)}
    out = np.array([newid[rep[p]] if labf[p] > 0 else 0 for p in range(hh * w)], np.int64).reshape(hh, w)
    parent = np.array([labf[r] for r in reps], np.int64)
    parts_of = np.zeros(k, np.int64)
    for r in reps:
        parts_of[labf[r] - 1] += 1
    return (out, parent, np.array([d2f[r] for r in reps], np.int64), np.array([(r % w, r // w) for r in reps], np.int64).reshape(-1, 2), parts_of, rounds)


# ---- label images -------------------------------------------------------------------------------------------------------------------------------
def disc(h, w, cy, cx, r):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys - cy) ** 2 + (xs - cx) ** 2 <= r * r


def ellipse(h, w, cy, cx, a, b, c, s):
    """Half axes a, b; (c, s) = the cosine and sine of the tilt as exact small fractions' values."""
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs - cx) * c + (ys - cy) * s
    v = -(xs - cx) * s + (ys - cy) * c
    return (u / a) ** 2 + (v / b) ** 2 <= 1


def shapes():
    """{name: labels int32 [H, W]}: the hand-made objects of the tests, small enough for the brute-force distance map."""
    out = {}
    out["two overlapping discs"] = (disc(28, 46, 13, 13, 10) | disc(28, 46, 13, 30, 10)).astype(np.int32)
    out["one disc"] = disc(27, 29, 13, 14, 11).astype(np.int32)
    a = np.zeros((20, 30), np.int32)
    a[3:17, 4:26] = 1
    out["a rectangle"] = a
    out["a tilted ellipse"] = ellipse(36, 44, 18, 22, 18, 7, 0.8, 0.6).astype(np.int32)
    a = np.zeros((13, 15), np.int32)                       # three bars of width 3: D2 = 4 along the whole centre line, one plateau
    a[1:12, 2:5] = 1
    a[1:12, 10:13] = 1
    a[9:12, 2:13] = 1
    out["a U-shaped plateau"] = a
    a = (disc(25, 60, 12, 11, 9) | disc(25, 60, 12, 47, 8)).astype(np.int32)
    a[11:14, 11:47] = 1
    out["a dumbbell"] = a
    a = np.zeros((14, 30), np.int32)
    a[2:11, 2:11] = 3
    a[4:12, 17:27] = 3
    out["one id in two pieces"] = a
    a = np.zeros((16, 26), np.int32)
    a[2:14, 2:13] = 1
    a[2:14, 13:24] = 2
    out["two labels side by side"] = a
    return out


# ---- one merge round on a hand-made edge list ---------------------------------------------------------------------------------------------------
INF = R.INF
# (P, S, h, absorbed): sqrt(P) - sqrt(S) <= h at equality, one above it, and where the products leave 32 and 63 bits
THRESHOLDS = [(9, 4, 1, True), (10, 4, 1, False), (4, 4, 0, True), (5, 4, 0, False), (4, 4, 1, True),
              (46340 ** 2, 46339 ** 2, 1, True), (46340 ** 2 + 1, 46339 ** 2, 1, False),           # t^2 = 4 h^2 S = 8 589 420 484 > 2^32
              (INF, 2 * 32766 ** 2, 32767, True), (INF, 2 * 32766 ** 2, 0, False),                 # S at the top of the finite range; 4 h^2 S = 2^63 - 1.8e15
              (INF, 2 ** 28, 32767, True), (INF, 1, 32767, False), (INF, 49151 ** 2 - INF - 1, 16384, False),
              (INF, INF, 0, True), (65 ** 2, 33 ** 2, 32, True), (65 ** 2 + 1, 33 ** 2, 32, False)]


def round_case(h):
    """-> (d2 [n] ints, edges {(a, b): S}, want {X: Y}) for the threshold triples with this h and a few orderings.  Pixels 2 i (Y, D2 = INF) and
    2 i + 1 (X, D2 = P) carry triple i; the tail holds: a component that takes the greater S of two passes, one that takes the smaller
    representative at equal S, one that is the higher end of its only pass (it stays), and a pair of equal peaks (the larger index moves)."""
    d2, edges, want = [], {}, {}
    for p, s, hh, fires in THRESHOLDS:
        if hh == h:
            y = len(d2)
            d2 += [INF, p]
            edges[(y, y + 1)] = s
            if fires:
                want[y + 1] = y
    b = len(d2)
    d2 += [50, 60, 70, 80, 90, 90, 20]
    edges.update({(b, b + 1): 45, (b, b + 2): 48,         # b: best is b + 2 (S = 48), shallow for h >= 1: 50 - 48 - h^2 <= 0
                  (b + 1, b + 3): 58, (b + 2, b + 3): 58,
                  (b + 4, b + 5): 90,                     # equal peaks: b + 5 moves to b + 4 (P = S)
                  (b + 3, b + 6): 20})                    # b + 6: its only pass leads up to b + 3, P = S
    rep = list(range(len(d2)))
    return d2, edges, merge_round(edges, d2, rep, h)
