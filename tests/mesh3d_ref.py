"""The definitions of utils.mesh3d as plain per-voxel loops over sets and dicts (DESIGN.md "7b, continued (3-D surfaces)"): the cuberille mesh, the
Euler number from the sets of lattice corners, edges and faces an object touches, the pinch edges by the four-voxel rule.  Shared by
tests/test_mesh3d_cpu.py (the numpy route against these) and tests/test_mesh3d_gpu.py (volumes and shapes)."""
import numpy as np

from tests import distance3d_ref as R3

NEIGHBOUR = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]                  # (dz, dy, dx) towards d
QUAD = [[(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)], [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],   # (dx, dy, dz), counter-clockwise from outside
        [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],
        [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)], [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)]]


def _at(vol, z, y, x):
    """the id at (z, y, x), 0 outside the volume"""
    n = vol.shape
    return int(vol[z, y, x]) if 0 <= z < n[0] and 0 <= y < n[1] and 0 <= x < n[2] else 0


def mesh(vol, k, only=None):
    """-> dict of lists: vertices [(x, y, z)], quads [[4 vertex indices]], source [face id], fstart, vstart [k + 1]"""
    Z, H, W = vol.shape
    faces = []
    for z in range(Z):
        for y in range(H):
            for x in range(W):
                l = int(vol[z, y, x])
                if l <= 0 or (only is not None and l not in only):
                    continue
                for d, (oz, oy, ox) in enumerate(NEIGHBOUR):
                    if _at(vol, z + oz, y + oy, x + ox) != l:
                        faces.append((l, 6 * ((z * H + y) * W + x) + d))
    faces.sort()
    corners = []
    for l, f in faces:
        p, d = divmod(f, 6)
        x, y, z = p % W, (p // W) % H, p // (W * H)
        corners.append([(l, ((z + dz) * (H + 1) + y + dy) * (W + 1) + x + dx) for dx, dy, dz in QUAD[d]])
    distinct = sorted({c for quad in corners for c in quad})
    index = {c: i for i, c in enumerate(distinct)}
    return {"vertices": [[c % (W + 1), (c // (W + 1)) % (H + 1), c // ((W + 1) * (H + 1))] for _, c in distinct],
            "quads": [[index[c] for c in quad] for quad in corners], "source": [f for _, f in faces],
            "fstart": [sum(1 for l, _ in faces if l <= i) for i in range(k + 1)], "vstart": [sum(1 for l, _ in distinct if l <= i) for i in range(k + 1)]}


def topology(vol, k):
    """-> (euler, pinch_edges), lists of k"""
    Z, H, W = vol.shape
    cells = [[set(), set(), set(), 0] for _ in range(k)]                             # corners, edges, faces, voxels per id
    for z in range(Z):
        for y in range(H):
            for x in range(W):
                l = int(vol[z, y, x])
                if l <= 0:
                    continue
                v, e, f, _ = cells[l - 1]
                cells[l - 1][3] += 1
                for a in (0, 1):
                    f.update([("x", x + a, y, z), ("y", x, y + a, z), ("z", x, y, z + a)])
                    for b in (0, 1):
                        e.update([("x", x, y + a, z + b), ("y", x + a, y, z + b), ("z", x + a, y + b, z)])
                        for c in (0, 1):
                            v.add((x + a, y + b, z + c))
    euler = [len(v) - len(e) + len(f) - c for v, e, f, c in cells]
    pinch = [0] * k
    ring = ((-1, -1), (0, -1), (0, 0), (-1, 0))                                       # the four voxels around an edge, in order round it
    for cz in range(Z + 1):
        for cy in range(H + 1):
            for cx in range(W + 1):
                for axis in "xyz":                                                    # the edge from the corner (cx, cy, cz) along `axis`
                    if axis == "x":
                        four = [_at(vol, cz + b, cy + a, cx) for a, b in ring] if cx < W else None
                    elif axis == "y":
                        four = [_at(vol, cz + b, cy, cx + a) for a, b in ring] if cy < H else None
                    else:
                        four = [_at(vol, cz, cy + b, cx + a) for a, b in ring] if cz < Z else None
                    if four is None:
                        continue
                    a, b, c, d = four
                    if a > 0 and a == c and b != a and d != a:
                        pinch[a - 1] += 1
                    if b > 0 and b == d and a != b and c != b:
                        pinch[b - 1] += 1
    return euler, pinch


def as_lists(t):
    return {n: getattr(t, n).tolist() for n in t._fields}


# ---- volumes ------------------------------------------------------------------------------------------------------------------------------------
def contact(kind):
    """two voxels of one id meeting along an edge only / at a corner only"""
    vol = np.zeros((2, 3, 3), np.int32)
    vol[0, 0, 0] = 1
    vol[(0, 1, 1) if kind == "edge" else (1, 1, 1)] = 1
    return vol


_CASES = []


def cases():
    """[(name, volume, K)]: the same list (and the same arrays) at every call."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(3)
    out = [("1x1x1", np.array([[[1]]], np.int32), 1),
           ("1x1x7 random", rng.integers(0, 4, (1, 1, 7)).astype(np.int32), 3),
           ("2x3x5 random", rng.integers(0, 4, (2, 3, 5)).astype(np.int32), 3),
           ("4x5x6 random", rng.integers(0, 4, (4, 5, 6)).astype(np.int32), 3),
           ("edge-only contact", contact("edge"), 1), ("corner-only contact", contact("corner"), 1)]
    a = np.zeros((4, 4, 7), np.int32)
    a[1:3, 1:3, 1:3] = 1
    a[1:3, 1:3, 3:6] = 2
    out.append(("two objects sharing a wall", a, 2))
    a = np.ones((3, 4, 5), np.int32)
    a[0, 0, 0] = 0
    a[1, 1, 1] = 2
    a[1, 2, 3] = 0
    out.append(("an object touching all six sides", a, 2))
    out.append(("one object filling the volume", np.ones((3, 4, 5), np.int32), 1))
    a = np.zeros((3, 4, 6), np.int32)
    a[0:2, 0:2, 0:3] = 1
    a[1:3, 2:4, 3:6] = 3
    out.append(("an absent id in the middle", a, 3))
    out.extend((name, vol, int(vol.max()) + 1) for name, vol in R3.cases())
    _CASES.extend(out)
    return _CASES


def shapes():
    """[(name, volume of one id, euler)]: the ball, the shell and the torus in (x, y, z) - 10 on a 21^3 grid, two 3^3 cubes one voxel apart"""
    z, y, x = (v.astype(np.int64) - 10 for v in np.meshgrid(np.arange(21), np.arange(21), np.arange(21), indexing="ij"))
    r2 = x * x + y * y + z * z
    two = np.zeros((5, 5, 9), np.int32)
    two[1:4, 1:4, 1:4] = 1
    two[1:4, 1:4, 5:8] = 1
    return [("ball", (r2 <= 64).astype(np.int32), 1), ("shell", ((r2 > 16) & (r2 <= 81)).astype(np.int32), 2),
            ("torus", ((np.sqrt(x * x + y * y) - 6) ** 2 + z * z <= 6.5).astype(np.int32), 0), ("two cubes", two, 2)]
