"""The definitions of utils.distance3d as per-voxel brute force: every value is a minimum over ALL voxels of the volume (or, for the raw outputs of
the z and y passes, over all voxels of the voxel's column / plane), nothing is separated into passes.  O(N^2): volumes stay below about 4000 voxels.
Shared by tests/test_distance3d_cpu.py (the host form against these) and tests/test_distance3d_gpu.py (the kernels' raw outputs); reference()
computes a case's answers once and keeps them."""
import numpy as np

INF = 2 ** 31 - 1
SPACINGS = [(1, 1, 1), (3, 1, 1), (1, 1, 4), (2, 3, 5)]
EDGES = [False, True, (True, False, False)]


def edges(edge):
    return (bool(edge),) * 3 if isinstance(edge, (bool, np.bool_)) else tuple(bool(v) for v in edge)


def _grid(vol):
    zs, ys, xs = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in vol.shape), indexing="ij")
    return zs.reshape(-1), ys.reshape(-1), xs.reshape(-1), vol.reshape(-1).astype(np.int64)


def _pairs(vol, s, within, chunk=256):
    """Yields (rows, D2 int64 [len(rows), N]): the squared distances of a chunk of voxels to every voxel; within "column" / "plane": INF + 1 to the
    voxels outside the voxel's (y, x) column / x plane."""
    zs, ys, xs, _ = _grid(vol)
    far = INF + 1
    for a in range(0, vol.size, chunk):
        r = np.arange(a, min(a + chunk, vol.size))
        d = s[0] ** 2 * (zs[r, None] - zs[None]) ** 2 + s[1] ** 2 * (ys[r, None] - ys[None]) ** 2 + s[2] ** 2 * (xs[r, None] - xs[None]) ** 2
        if within in ("column", "plane"):
            d = np.where(xs[r, None] != xs[None], far, d)
        if within == "column":
            d = np.where(ys[r, None] != ys[None], far, d)
        yield r, d


def inner_distance(vol, s=(1, 1, 1), edge=False, within=None):
    e = edges(edge)
    zs, ys, xs, ls = _grid(vol)
    out = np.zeros(vol.size, np.int64)
    pos = (zs, ys, xs)
    for r, d in _pairs(vol, s, within):
        best = np.where(ls[r, None] != ls[None], d, INF).min(axis=1)
        for a in range(3):
            if e[a]:
                best = np.minimum(best, np.minimum((s[a] * (pos[a][r] + 1)) ** 2, (s[a] * (vol.shape[a] - pos[a][r])) ** 2))
        out[r] = np.where(ls[r] > 0, np.minimum(best, INF), 0)
    return out.reshape(vol.shape)


def background_feature(vol, s=(1, 1, 1), max_distance2=None, within=None):
    _, _, _, ls = _grid(vol)
    d2 = np.full(vol.size, INF, np.int64)
    near = np.zeros(vol.size, np.int64)
    on = ls > 0
    if on.any():
        for r, d in _pairs(vol, s, within):
            d = np.where(on[None], d, INF + 1)
            m = d.min(axis=1)
            lab = np.where(d == m[:, None], ls[None], INF).min(axis=1)          # the smallest id among ALL minimisers
            ok = m < INF
            if max_distance2 is not None:
                ok &= m <= max_distance2
            d2[r] = np.where(ok, m, INF)
            near[r] = np.where(ok, lab, 0)
    return d2.reshape(vol.shape), near.reshape(vol.shape)


def expand_labels(vol, r2, feature):
    d2, near = feature
    return np.where(vol > 0, vol, np.where(d2 <= r2, near, 0)).astype(np.int64)


def shrink_labels(vol, r2, d2):
    return np.where((vol > 0) & (d2 > r2), vol, 0).astype(np.int64)


def object_depth(vol, k, d2):
    r2 = np.zeros(k, np.int64)
    xyz = np.full((k, 3), -1, np.int64)
    for z in range(vol.shape[0]):                          # raster order: the first voxel that attains the maximum stays
        for y in range(vol.shape[1]):
            for x in range(vol.shape[2]):
                i = int(vol[z, y, x])
                if i > 0 and d2[z, y, x] > r2[i - 1]:
                    r2[i - 1] = d2[z, y, x]
                    xyz[i - 1] = (x, y, z)
    return r2, xyz


def _voxels(d2):
    """Squared distances along one unweighted line -> the 16-bit voxel counts of the z pass (0xFFFF: none)."""
    g = np.rint(np.sqrt(np.minimum(d2, INF).astype(np.float64))).astype(np.int64)
    assert np.array_equal(np.where(d2 >= INF, INF, g * g), d2)
    return np.where(d2 >= INF, 0xFFFF, g)


def z_inner(vol, ez):
    """g [Z, H, W]: the distance in voxels of a labelled voxel to the nearest voxel of its (y, x) column with another label (0xFFFF: none; 0 on the
    background)."""
    return _voxels(inner_distance(vol, (1, 1, 1), (ez, False, False), within="column"))


def z_feature(vol):
    d2, near = background_feature(vol, (1, 1, 1), within="column")
    return _voxels(d2), near


def y_inner(vol, s, edge):
    """h [Z, H, W]: the inner distance within the voxel's (z, y) plane."""
    e = edges(edge)
    return inner_distance(vol, s, (e[0], e[1], False), within="plane")


def y_feature(vol, s):
    return background_feature(vol, s, within="plane")


# ---- label volumes ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 9, 12), (7, 1, 11), (9, 10, 1), (1, 1, 8), (5, 1, 1), (1, 6, 1), (2, 2, 2), (4, 5, 6), (12, 7, 5), (6, 12, 9), (3, 11, 12),
          (10, 10, 10), (12, 12, 12)]


def blobs(seed, z, h, w, n=None, ids=None):
    """Random ellipsoids and bars, later ones on top; ids are drawn from 1..ids with repeats (disconnected objects) and gaps (absent ids)."""
    rng = np.random.default_rng([seed, 0xD153])
    n = int(rng.integers(1, 7)) if n is None else n
    ids = n + 2 if ids is None else ids
    vol = np.zeros((z, h, w), np.int32)
    zs, ys, xs = np.meshgrid(np.arange(z), np.arange(h), np.arange(w), indexing="ij")
    for _ in range(n):
        i = int(rng.integers(1, ids + 1))
        cz, cy, cx = rng.uniform(0, z), rng.uniform(0, h), rng.uniform(0, w)
        if rng.integers(0, 3) == 0:
            m = (abs(zs - cz) <= rng.uniform(0.5, 2.5)) & (abs(ys - cy) <= rng.uniform(0.5, 3)) & (abs(xs - cx) <= rng.uniform(1, max(w, 2) / 2))
        else:
            rz, ry, rx = (rng.uniform(0.7, max(v, 3) / 2.2) for v in (z, h, w))
            m = ((zs - cz) / rz) ** 2 + ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
        vol[m] = i
    return vol


def named_cases():
    """[(name, volume int32 [Z, H, W])]"""
    out = []
    a = np.zeros((5, 6, 7), np.int32)
    a[2, 3, 4] = 1
    out.append(("a one-voxel object", a))
    out.append(("one label filling the volume", np.full((4, 5, 6), 1, np.int32)))
    out.append(("no labelled voxel", np.zeros((3, 4, 5), np.int32)))
    a = np.zeros((5, 5, 14), np.int32)
    a[1:4, 1:4, 1:4] = 2
    a[1:4, 1:4, 4:8] = 1
    a[1:4, 1:4, 8:13] = 2
    out.append(("two pieces of one object on a row, another label between them", a))
    a = np.zeros((7, 9, 8), np.int32)
    a[1:6, 1:8, 1:7] = 3
    a[2:5, 3:6, 3:7] = 0
    out.append(("a C-shaped object", a))
    a = np.zeros((6, 7, 8), np.int32)
    a[1:3, 1:4, 1:4] = 2
    a[3:6, 4:7, 4:8] = 5
    out.append(("absent ids", a))
    return out


_CASES = []
_KEPT = {}


def cases():
    """[(name, volume)]: the same list (and the same arrays) at every call."""
    if not _CASES:
        _CASES.extend((f"blobs seed {i} {z} x {h} x {w}", blobs(i, z, h, w)) for i, (z, h, w) in enumerate(SHAPES))
        _CASES.extend(named_cases())
    return _CASES


def reference(name, what, spacing=(1, 1, 1), edge=False):
    """The brute-force answer of a case of cases(), computed once: what = "inner" -> D2; "feature" -> (D2, nearest), unbounded."""
    key = (name, what, tuple(spacing), edges(edge) if what == "inner" else None)
    if key not in _KEPT:
        vol = dict(cases())[name]
        _KEPT[key] = inner_distance(vol, spacing, edge) if what == "inner" else background_feature(vol, spacing)
    return _KEPT[key]


def bounded(feature, m):
    """background_feature's answer under max_distance2 = m from the unbounded one."""
    d2, near = feature
    return np.where(d2 <= m, d2, INF), np.where(d2 <= m, near, 0)
