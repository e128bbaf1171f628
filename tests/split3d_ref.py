"""The definition of utils.split3d.split_labels3d as plain per-voxel loops over Python integers: nothing is vectorised, the distance map is the
brute-force one of tests/distance3d_ref.py, the merge round is tests/split_ref.py's (it never looks at a shape).  Shared by
tests/test_split3d_cpu.py (the host form against these) and tests/test_split3d_gpu.py (the kernels' raw outputs)."""
import numpy as np

from tests import distance3d_ref as R3
from tests.split_ref import merge_round, shallow  # noqa: F401  (shape-free: one round on an edge list, the exact shallow test)

NEIGHBOURS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
FORWARD = [(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1)] + [(1, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]   # every 26-adjacent pair once
assert len(NEIGHBOURS) == 26 and len(FORWARD) == 13 and sorted(FORWARD + [(-a, -b, -c) for a, b, c in FORWARD]) == sorted(NEIGHBOURS)


def _voxels(vol):
    z, h, w = vol.shape
    return [(a, b, c) for a in range(z) for b in range(h) for c in range(w)]


def ascent(vol, d2):
    """up [Z * H * W] (Python ints): the voxel of greatest (d2, -index) among p and its 26 neighbours with p's label; p itself on the background."""
    z, h, w = vol.shape
    up = list(range(z * h * w))
    for a, b, c in _voxels(vol):
        if vol[a, b, c] <= 0:
            continue
        best = (int(d2[a, b, c]), -((a * h + b) * w + c))
        for dz, dy, dx in NEIGHBOURS:
            aa, bb, cc = a + dz, b + dy, c + dx
            if 0 <= aa < z and 0 <= bb < h and 0 <= cc < w and vol[aa, bb, cc] == vol[a, b, c]:
                best = max(best, (int(d2[aa, bb, cc]), -((aa * h + bb) * w + cc)))
        up[(a * h + b) * w + c] = -best[1]
    return up


def roots(up):
    """[Z * H * W]: the root every chain reaches."""
    out = []
    for p in range(len(up)):
        while up[p] != p:
            p = up[p]
        out.append(p)
    return out


def passes(vol, d2, root):
    """{(a, b): S} for the basins a < b of one label that touch."""
    z, h, w = vol.shape
    out = {}
    for a, b, c in _voxels(vol):
        if vol[a, b, c] <= 0:
            continue
        for dz, dy, dx in FORWARD:
            aa, bb, cc = a + dz, b + dy, c + dx
            if 0 <= aa < z and 0 <= bb < h and 0 <= cc < w and vol[aa, bb, cc] == vol[a, b, c]:
                ra, rb = root[(a * h + b) * w + c], root[(aa * h + bb) * w + cc]
                if ra != rb:
                    k = (min(ra, rb), max(ra, rb))
                    out[k] = max(out.get(k, 0), min(int(d2[a, b, c]), int(d2[aa, bb, cc])))
    return out


def basins(vol, d2):
    """-> (rep [n], edges {(a, b): S}): what does not depend on min_depth, computed once per (volume, D2)."""
    rep = roots(ascent(vol, d2))
    return rep, passes(vol, d2, rep)


def split(vol, h, spacing=(1, 1, 1), edge=False, k=None, d2=None, start=None):
    """-> (labels [Z, H, W], parent [K'], peak_r2 [K'], peak_xyz [K', 3], parts_of [K], rounds), all int64.  d2: the brute-force map where the
    caller has it already; start = basins(vol, d2) likewise."""
    z, hh, w = vol.shape
    n = z * hh * w
    k = max(int(vol.max()), 0) if k is None else k
    d2 = R3.inner_distance(vol, spacing, edge) if d2 is None else d2
    d2f = [int(v) for v in d2.reshape(-1)]
    labf = [int(v) for v in vol.reshape(-1)]
    rep, edges = basins(vol, d2) if start is None else start
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
    reps = sorted({rep[p] for p in range(n) if labf[p] > 0}, key=lambda r: (labf[r], r))
    newid = {r: i + 1 for i, r in enumerate(reps)}
    out = np.array([newid[rep[p]] if labf[p] > 0 else 0 for p in range(n)], np.int64).reshape(z, hh, w)
    parent = np.array([labf[r] for r in reps], np.int64)
    parts_of = np.zeros(k, np.int64)
    for r in reps:
        parts_of[labf[r] - 1] += 1
    xyz = np.array([(r % w, (r // w) % hh, r // (w * hh)) for r in reps], np.int64).reshape(-1, 3)
    return out, parent, np.array([d2f[r] for r in reps], np.int64), xyz, parts_of, rounds


def component_count(vol):
    """The number of 26-connected components of equal positive label, by a plain stack search."""
    z, h, w = vol.shape
    seen = set()
    count = 0
    for v in _voxels(vol):
        if vol[v] <= 0 or v in seen:
            continue
        count += 1
        seen.add(v)
        stack = [v]
        while stack:
            a, b, c = stack.pop()
            for dz, dy, dx in NEIGHBOURS:
                q = (a + dz, b + dy, c + dx)
                if 0 <= q[0] < z and 0 <= q[1] < h and 0 <= q[2] < w and q not in seen and vol[q] == vol[a, b, c]:
                    seen.add(q)
                    stack.append(q)
    return count


# ---- label volumes ------------------------------------------------------------------------------------------------------------------------------
def ball(shape, centre, r, spacing=(1, 1, 1)):
    """The voxels within r (in spacing units) of `centre` (in voxels)."""
    zs, ys, xs = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return sum((s * (g - c)) ** 2 for s, g, c in zip(spacing, (zs, ys, xs), centre)) <= r * r


DENSE = [(41, 8, 12, 14), (44, 7, 13, 15), (45, 9, 12, 12)]
DENSE_SPACINGS = [(1, 1, 1), (2, 3, 5)]


def dense():
    """[(name, volume)]: random volumes of three ids in eight overlapping blobs each -- objects of several basins, merges over more than one round."""
    return [(f"dense blobs seed {s} {z} x {h} x {w}", R3.blobs(s, z, h, w, n=8, ids=3)) for s, z, h, w in DENSE]


def shapes():
    """{name: (volume int32 [Z, H, W], spacing, edges)}: the hand-made objects of the tests, a few hundred to about 1500 voxels each -- small enough
    for the brute-force distance map and the loops.  `edges` lists the edge arguments the case is run under."""
    out = {}
    plain = [False]
    # two balls of radius 4 voxels whose centres are 6 planes apart along z: at (1, 1, 1) the waist between them is a neck; under (1, 3, 3) the
    # same voxels are 15 units tall and 27 across, the waist is farther from the surface than either centre, and the map has one peak there
    two = (ball((15, 9, 9), (4, 4, 4), 4) | ball((15, 9, 9), (10, 4, 4), 4)).astype(np.int32)
    out["two balls fused along z, spacing (1, 1, 1): a neck"] = (two, (1, 1, 1), plain)
    out["two balls fused along z, spacing (1, 3, 3): no neck"] = (two, (1, 3, 3), plain)
    along_x = (ball((9, 9, 16), (4, 4, 4), 4) | ball((9, 9, 16), (4, 4, 11), 4)).astype(np.int32)
    out["two balls fused along x"] = (along_x, (1, 1, 1), plain)
    out["two balls fused along x, spacing (4, 4, 4)"] = (along_x, (4, 4, 4), plain)           # min_depth is in spacing units: 5 is 1.25 voxels here
    a = np.zeros((10, 10, 10), np.int32)                  # two cubes that share one corner-to-corner voxel pair: 26-adjacent, not 6- or 18-adjacent
    a[1:5, 1:5, 1:5] = 1
    a[5:9, 5:9, 5:9] = 1
    out["a neck diagonal in all three axes"] = (a, (1, 1, 1), plain)
    a = np.zeros((5, 13, 15), np.int32)                   # three bars of cross-section 3 x 3 in a U: D2 = 4 along the whole centre line, a plateau
    a[1:4, 1:12, 1:4] = 1                                 # many voxels wide with a root on either arm: it must join at min_depth = 0
    a[1:4, 1:12, 11:14] = 1
    a[1:4, 9:12, 1:14] = 1
    out["a U-shaped plateau"] = (a, (1, 1, 1), plain)
    a = np.zeros((7, 7, 15), np.int32)                    # two 5-cubes joined by a 1-voxel rod: peaks of equal D2 = 9, the tie goes to the smaller index
    a[1:6, 1:6, 1:6] = 1
    a[1:6, 1:6, 9:14] = 1
    a[3, 3, 6:9] = 1
    out["equal peaks"] = (a, (1, 1, 1), plain)
    a = np.zeros((6, 8, 14), np.int32)
    a[1:5, 1:6, 1:5] = 3
    a[2:6, 2:7, 8:13] = 3
    out["one id in two unconnected pieces"] = (a, (1, 1, 1), plain)
    a = np.zeros((6, 7, 8), np.int32)
    a[1:3, 1:4, 1:4] = 2
    a[3:6, 4:7, 4:8] = 5
    out["absent ids"] = (a, (2, 3, 5), plain)
    a = (ball((8, 9, 14), (0, 4, 3), 4) | ball((8, 9, 14), (2, 4, 10), 4)).astype(np.int32)     # cut by the z = 0 face
    out["an object touching the border"] = (a, (1, 1, 1), list(R3.EDGES))
    out["an object touching the border, spacing (2, 3, 5)"] = (a, (2, 3, 5), list(R3.EDGES))
    a = (ball((1, 12, 24), (0, 5, 6), 5) | ball((1, 12, 24), (0, 6, 16), 5)).astype(np.int32)
    out["Z = 1"] = (a, (3, 1, 1), list(R3.EDGES))
    out["Z = 2"] = (np.concatenate([a, a[:, ::-1]], 0), (3, 1, 1), list(R3.EDGES))
    a = np.zeros((1, 1, 40), np.int32)
    a[0, 0, 2:17] = 1
    a[0, 0, 17:30] = 2
    a[0, 0, 33:39] = 1
    out["a 1 x 1 x n line"] = (a, (1, 1, 4), list(R3.EDGES))
    return out
