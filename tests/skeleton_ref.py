"""The definitions of utils.skeleton as plain per-pixel loops: the two tables of Guo and Hall's rule built from its formulas bit by bit, one
sub-iteration as a double loop over a copy, links and degrees as loops over pixel pairs.  Imports nothing from the package.  Shared by
tests/test_skeleton_cpu.py (the host form against these) and tests/test_skeleton_gpu.py (the kernels' raw outputs)."""
import numpy as np

# neighbour bit i of the code: N, NE, E, SE, S, SW, W, NW (y grows downwards) = p2..p9 of the paper
OFFSETS = [(-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)]      # (dy, dx)


def deletable(code, parity):
    p2, p3, p4, p5, p6, p7, p8, p9 = [(code >> i) & 1 for i in range(8)]
    c = ((1 - p2) & (p3 | p4)) + ((1 - p4) & (p5 | p6)) + ((1 - p6) & (p7 | p8)) + ((1 - p8) & (p9 | p2))
    n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8)
    n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9)
    n = min(n1, n2)
    m = ((p2 | p3 | (1 - p5)) & p4) if parity == 0 else ((p6 | p7 | (1 - p9)) & p8)
    return c == 1 and 2 <= n <= 3 and m == 0


def table(parity):
    return [bool(deletable(code, parity)) for code in range(256)]


TABLES = [table(0), table(1)]


def code_at(img, y, x):
    """The 8-bit code of pixel (y, x) of the current image: a neighbour is on when it is in the frame and carries the pixel's (positive) label."""
    h, w = img.shape
    l = int(img[y, x])
    code = 0
    for i, (dy, dx) in enumerate(OFFSETS):
        yy, xx = y + dy, x + dx
        if 0 <= yy < h and 0 <= xx < w and int(img[yy, xx]) == l:
            code |= 1 << i
    return code


def subiteration(img, index):
    """-> (the image after sub-iteration `index`, the pixels it deleted): every pixel is judged on the state at the start."""
    out = img.copy()
    deleted = 0
    tab = TABLES[index & 1]
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            if img[y, x] > 0 and tab[code_at(img, y, x)]:
                out[y, x] = 0
                deleted += 1
    return out, deleted


def skeletonize(lab, steps=None):
    """-> (skeleton int64 [H, W], subiterations, [the image after every sub-iteration run]); steps: run exactly that many sub-iterations."""
    img = np.asarray(lab).astype(np.int64).copy()
    trail, last, quiet, i = [], 0, 0, 0
    while (steps is None and quiet < 2) or (steps is not None and i < steps):
        img, d = subiteration(img, i)
        trail.append(img)
        if d:
            last, quiet = i + 1, 0
        else:
            quiet += 1
        i += 1
    return img, last, trail


def linked(img, y, x, dy, dx):
    """Is (y, x) linked to (y + dy, x + dx)?  4-adjacent pixels of one label are; diagonal ones are when neither pixel 4-adjacent to both has it."""
    h, w = img.shape
    l = int(img[y, x])
    yy, xx = y + dy, x + dx
    if l <= 0 or not (0 <= yy < h and 0 <= xx < w) or int(img[yy, xx]) != l:
        return False
    if dy == 0 or dx == 0:
        return True
    return int(img[y, xx]) != l and int(img[yy, x]) != l


def degrees(img):
    img = np.asarray(img).astype(np.int64)
    deg = np.zeros(img.shape, np.int64)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            deg[y, x] = sum(linked(img, y, x, dy, dx) for dy, dx in OFFSETS)
    return deg


def node_image(img):
    img = np.asarray(img).astype(np.int64)
    deg = degrees(img)
    out = np.zeros(img.shape, np.uint8)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            if img[y, x] > 0:
                d = int(deg[y, x])
                out[y, x] = 4 if d == 0 else 1 if d == 1 else 2 if d == 2 else 3
    return out


FIELDS = ("pixels", "end_points", "junctions", "isolated", "links_orth", "links_diag", "degree_sum")


def measure(img, k, d2=None):
    """{field: [k] Python integers}; with d2 also d2_sum, d2_min (2^31 - 1 for an absent id), d2_max (-1)."""
    img = np.asarray(img).astype(np.int64)
    deg = degrees(img)
    t = {f: [0] * k for f in FIELDS}
    if d2 is not None:
        t.update(d2_sum=[0] * k, d2_min=[2 ** 31 - 1] * k, d2_max=[-1] * k)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            l = int(img[y, x])
            if l <= 0:
                continue
            d = int(deg[y, x])
            t["pixels"][l - 1] += 1
            t["end_points"][l - 1] += d == 1
            t["junctions"][l - 1] += d >= 3
            t["isolated"][l - 1] += d == 0
            t["degree_sum"][l - 1] += d
            t["links_orth"][l - 1] += linked(img, y, x, 0, 1) + linked(img, y, x, 1, 0)          # every link once: right, down,
            t["links_diag"][l - 1] += linked(img, y, x, 1, 1) + linked(img, y, x, 1, -1)         # down-right, down-left
            if d2 is not None:
                v = int(d2[y, x])
                t["d2_sum"][l - 1] += v
                t["d2_min"][l - 1] = min(t["d2_min"][l - 1], v)
                t["d2_max"][l - 1] = max(t["d2_max"][l - 1], v)
    return t


# ---- label images -------------------------------------------------------------------------------------------------------------------------------
def disc(h, w, cy, cx, r, label=1):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where((ys - cy) ** 2 + (xs - cx) ** 2 <= r * r, label, 0).astype(np.int32)


def small_cases():
    """[(name, labels, the pixels (row, column) left, subiterations)]: the six small cases."""
    full = lambda h, w: np.ones((h, w), np.int32)
    return [("2 x 2", full(2, 2), [(1, 0)], 1), ("3 x 3", full(3, 3), [(1, 1)], 2), ("1 x 9", full(1, 9), [(0, c) for c in range(9)], 0),
            ("2 x 9", full(2, 9), [(1, c) for c in range(8)], 1), ("8 x 8", full(8, 8), [(4, 3)], 7),
            ("a full 5 x 7 frame", full(5, 7), [(2, 2), (2, 3), (2, 4)], 4)]


def hand_made():
    """[(name, labels int32 [H, W])]: the hand-made part of the shape list."""
    out = [(name, lab) for name, lab, _, _ in small_cases()]
    out += [("1 x 1", np.ones((1, 1), np.int32)), ("9 x 1", np.ones((9, 1), np.int32))]
    a = disc(47, 45, 23, 22, 15)
    a[(np.mgrid[0:47, 0:45][0] - 23) ** 2 + (np.mgrid[0:47, 0:45][1] - 22) ** 2 <= 36] = 0
    out.append(("a ring with a hole", a))
    a = np.zeros((21, 26), np.int32)
    a[:, 9:14] = 3
    a[8:12, :] = 3
    out.append(("an instance that touches all four frame edges", a))
    a = np.zeros((38, 52), np.int32)
    a[3:35, 4:26] = 1
    a[3:35, 26:49] = 2
    out.append(("two large instances that share a long straight border", a))
    a = np.zeros((17, 23), np.int32)
    a[2:9, 3:14] = 5
    a[9:15, 6:20] = 1000000
    out.append(("non-compact ids", a))
    return out
