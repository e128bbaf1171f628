"""The definitions of utils.measure3d as plain per-voxel Python loops (the checker of the numpy route, which in turn checks the device route): one
walk for the tables, one for the contacts, and the centroid, covariance and intensity mean / variance per object in exact rational arithmetic
(fractions.Fraction).  The volumes are those of tests/distance3d_ref.py."""
from fractions import Fraction

import numpy as np

from tests import distance3d_ref as R3
from tests.split3d_ref import ball

INT_MAX = 2 ** 31 - 1
IMAGES = ((None, 0), (np.uint8, 1), (np.uint8, 3), (np.uint16, 4), (np.uint16, 0))   # (dtype, C); C = 0: [Z, H, W] -- the five kinds of the 2-D tests
AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))                                             # the step to the next voxel along z, y, x


def cases():
    """[(name, volume int32 [Z, H, W], K)]: distance3d_ref.cases(), K two above the largest id (absent ids at the end of every table)."""
    return [(name, vol, int(vol.max()) + 2) for name, vol in R3.cases()]


def intensity(z, h, w, c, dtype, seed=0):
    """A deterministic image with the full range of the type in it; c = 0: [Z, H, W]."""
    rng = np.random.default_rng([seed, z, h, w, c])
    top = np.iinfo(dtype).max
    img = rng.integers(0, top + 1, (z, h, w, max(c, 1))).astype(dtype)
    img.reshape(-1)[::7] = top
    img.reshape(-1)[3::11] = 0
    return img[..., 0].copy() if c == 0 else img


def image(vol, dtype, c, seed=0):
    return None if dtype is None else intensity(vol.shape[0], vol.shape[1], vol.shape[2], c, dtype, seed)


def tables(vol, k, img=None):
    """dict of int lists, one row per id 1..k, by one walk over the voxels."""
    Z, H, W = vol.shape
    c = 0 if img is None else (1 if img.ndim == 3 else img.shape[3])
    im = None if img is None else img.reshape(Z, H, W, c)
    voxels = [0] * k
    box = [[INT_MAX, INT_MAX, INT_MAX, -1, -1, -1] for _ in range(k)]
    mom = [[0] * 9 for _ in range(k)]
    surf = [[0] * 7 for _ in range(k)]
    isum = [[0] * c for _ in range(k)]
    isum2 = [[0] * c for _ in range(k)]
    imin = [[INT_MAX] * c for _ in range(k)]
    imax = [[-1] * c for _ in range(k)]
    for z in range(Z):
        for y in range(H):
            for x in range(W):
                l = int(vol[z, y, x])
                if l <= 0:
                    continue
                i = l - 1
                voxels[i] += 1
                b = box[i]
                b[0], b[1], b[2], b[3], b[4], b[5] = min(b[0], x), min(b[1], y), min(b[2], z), max(b[3], x), max(b[4], y), max(b[5], z)
                for j, v in enumerate((x, y, z, x * x, y * y, z * z, x * y, x * z, y * z)):
                    mom[i][j] += v
                any_face = False
                for a, (dz, dy, dx) in enumerate(AXES):
                    for sign in (-1, 1):
                        zz, yy, xx = z + sign * dz, y + sign * dy, x + sign * dx
                        nb = int(vol[zz, yy, xx]) if 0 <= zz < Z and 0 <= yy < H and 0 <= xx < W else -1
                        if nb != l:
                            any_face = True
                            surf[i][1 + a] += 1
                            if nb > 0:
                                surf[i][4 + a] += 1
                surf[i][0] += 1 if any_face else 0
                for j in range(c):
                    v = int(im[z, y, x, j])
                    isum[i][j] += v
                    isum2[i][j] += v * v
                    imin[i][j] = min(imin[i][j], v)
                    imax[i][j] = max(imax[i][j], v)
    out = dict(voxels=voxels, box=box, moments=mom, surface=surf)
    if img is not None:
        out.update(isum=isum, isum2=isum2, imin=imin, imax=imax)
    return out


def contacts(vol):
    """sorted [(a, b, nz, ny, nx)], a < b: n_a = the faces normal to axis a shared by a voxel of a and its neighbour voxel of b (forward along each
    axis: every pair of voxels once)."""
    Z, H, W = vol.shape
    n = {}
    for z in range(Z):
        for y in range(H):
            for x in range(W):
                l = int(vol[z, y, x])
                for a, (dz, dy, dx) in enumerate(AXES):
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if zz < Z and yy < H and xx < W:
                        m = int(vol[zz, yy, xx])
                        if l > 0 and m > 0 and l != m:
                            n.setdefault((min(l, m), max(l, m)), [0, 0, 0])[a] += 1
    return sorted((a, b, c[0], c[1], c[2]) for (a, b), c in n.items())


def as_lists(table):
    """An ObjectTable (tensors) as the dict of lists `tables` returns."""
    return {name: getattr(table, name).cpu().numpy().astype(np.int64).tolist() for name in table._fields if getattr(table, name) is not None}


def shape_fraction(vol, k, spacing=(1, 1, 1)):
    """Per id 1..k, from the voxels in exact arithmetic: None for an absent id, else (V, centroid (x, y, z), covariance [3][3] in (x, y, z) order), all
    Fractions in physical units; spacing = (sz, sy, sx) as Fractions or what Fraction() takes exactly."""
    sz, sy, sx = (Fraction(v) for v in spacing)
    s = (sx, sy, sz)
    out = []
    for l in range(1, k + 1):
        zs, ys, xs = np.nonzero(vol == l)
        v = len(zs)
        if v == 0:
            out.append(None)
            continue
        pts = [tuple(int(t) * s[a] for a, t in enumerate(p)) for p in zip(xs, ys, zs)]
        cen = [Fraction(sum(p[a] for p in pts), v) for a in range(3)]
        cov = [[sum((p[a] - cen[a]) * (p[b] - cen[b]) for p in pts) / v for b in range(3)] for a in range(3)]
        out.append((v, cen, cov))
    return out


def invariants(cov):
    """(trace, second invariant, determinant) of a 3 x 3 Fraction matrix: e1 = l1 + l2 + l3, e2 = l1 l2 + l1 l3 + l2 l3, e3 = l1 l2 l3 of its eigenvalues."""
    c = cov
    e1 = c[0][0] + c[1][1] + c[2][2]
    e2 = (c[0][0] * c[1][1] - c[0][1] * c[1][0]) + (c[0][0] * c[2][2] - c[0][2] * c[2][0]) + (c[1][1] * c[2][2] - c[1][2] * c[2][1])
    e3 = (c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0])
          + c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]))
    return e1, e2, e3


def intensity_fraction(vol, k, img):
    """Per id and channel (mean, population variance) as Fractions from the voxels; None for an absent id."""
    im = img.reshape(vol.shape + (-1,))
    out = []
    for l in range(1, k + 1):
        m = vol == l
        v = int(m.sum())
        if v == 0:
            out.append(None)
            continue
        row = []
        for j in range(im.shape[3]):
            t = [int(u) for u in im[..., j][m]]
            mean = Fraction(sum(t), v)
            row.append((mean, sum((u - mean) ** 2 for u in t) / v))
        out.append(row)
    return out


def ellipsoid_scene(z=20, h=44, w=64):
    """-> (volume, K): well separated ellipsoids of clearly different axes in several directions, one of them cut by the volume, id 4 left absent.
    Under spacing (2.5, 1, 1) every one has l1 - l2 > 1e-3 l1 (the test verifies that on the exact covariance before it asserts on an axis)."""
    zs, ys, xs = np.meshgrid(np.arange(z), np.arange(h), np.arange(w), indexing="ij")
    vol = np.zeros((z, h, w), np.int32)
    # (centre x, y, z), semi-axes along the rotated u, v and along z, the rotation of (u, v) in the xy plane, a shear of z into u
    specs = [((11, 10, 5), (9, 4, 3), 0.0, 0.0), ((34, 11, 13), (10, 5, 4), 0.7, 0.0), ((55, 12, 6), (4, 9, 3), 0.3, 0.15),
             ((12, 32, 12), (5, 8, 5), -0.5, 0.0), ((36, 33, 7), (11, 4, 4), 2.0, -0.2), ((62, 36, 17), (10, 6, 5), 1.1, 0.0)]
    for i, ((cx, cy, cz), (a, b, c), th, sh) in enumerate(specs):
        dx, dy, dz = xs - cx, ys - cy, zs - cz
        u = dx * np.cos(th) + dy * np.sin(th) + sh * dz * 2.5
        v = -dx * np.sin(th) + dy * np.cos(th)
        vol[(u / a) ** 2 + (v / b) ** 2 + (dz / c) ** 2 < 1.0] = i + 1 if i < 3 else i + 2   # (id 4 stays absent)
    return vol, len(specs) + 1


__all__ = ["ball", "cases", "tables", "contacts"]
