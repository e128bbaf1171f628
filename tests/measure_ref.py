"""The definitions of utils.measure as plain per-pixel Python loops (the checker of the numpy route, which in turn checks the device route), the
contact list by the same kind of loop, and the moment-derived region properties in exact rational arithmetic (fractions.Fraction)."""
import math
from fractions import Fraction

import numpy as np

INT_MAX = 2 ** 31 - 1


def frames():
    """name -> (labels int32 [H, W], K): the small frames both test files walk."""
    from ullsam_amd.utils import synthetic as S
    checker = (np.arange(6 * 7, dtype=np.int32).reshape(6, 7) + 1)
    out = {
        "1x1": (np.array([[1]], np.int32), 1),
        "1x1 background": (np.array([[0]], np.int32), 2),
        "1x7": (np.array([[1, 1, 0, 2, 2, 2, 1]], np.int32), 3),
        "5x3": (np.array([[1, 1, 2], [1, 0, 2], [3, 3, 2], [3, 0, 0], [4, 4, 4]], np.int32), 5),
        "one label fills the frame": (np.full((9, 70), 2, np.int32), 2),
        "checkerboard of distinct ids": (checker, 42),
        "discs 150x170": (S.label_frame(3, 150, 170, 40, (4.0, 14.0)), 40),
    }
    return out


def intensity(h, w, c, dtype, seed=0):
    """A deterministic image with the full range of the type in it; c = 0: [H, W]."""
    rng = np.random.default_rng([seed, h, w, c])
    top = np.iinfo(dtype).max
    img = rng.integers(0, top + 1, (h, w, max(c, 1))).astype(dtype)
    img.reshape(-1)[::7] = top
    img.reshape(-1)[3::11] = 0
    return img[:, :, 0].copy() if c == 0 else img


def tables(lab, k, img=None):
    """dict of int lists, one row per label 1..k, by one walk over the pixels."""
    h, w = lab.shape
    c = 0 if img is None else (1 if img.ndim == 2 else img.shape[2])
    im = None if img is None else img.reshape(h, w, c)
    area = [0] * k
    box = [[INT_MAX, INT_MAX, -1, -1] for _ in range(k)]
    mom = [[0] * 5 for _ in range(k)]
    per = [[0] * 3 for _ in range(k)]
    isum = [[0] * c for _ in range(k)]
    isum2 = [[0] * c for _ in range(k)]
    imin = [[INT_MAX] * c for _ in range(k)]
    imax = [[-1] * c for _ in range(k)]
    for y in range(h):
        for x in range(w):
            l = int(lab[y, x])
            if l <= 0:
                continue
            i = l - 1
            area[i] += 1
            b = box[i]
            b[0], b[1], b[2], b[3] = min(b[0], x), min(b[1], y), max(b[2], x), max(b[3], y)
            for j, v in enumerate((x, y, x * x, y * y, x * y)):
                mom[i][j] += v
            edges = contact = 0
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                nb = int(lab[yy, xx]) if 0 <= yy < h and 0 <= xx < w else -1
                if nb != l:
                    edges += 1
                    if nb > 0:
                        contact += 1
            per[i][0] += 1 if edges else 0
            per[i][1] += edges
            per[i][2] += contact
            for j in range(c):
                v = int(im[y, x, j])
                isum[i][j] += v
                isum2[i][j] += v * v
                imin[i][j] = min(imin[i][j], v)
                imax[i][j] = max(imax[i][j], v)
    out = dict(area=area, box=box, moments=mom, perimeter=per)
    if img is not None:
        out.update(isum=isum, isum2=isum2, imin=imin, imax=imax)
    return out


def contacts(lab):
    """sorted [(a, b, n)], a < b: n = the pixel sides shared by a pixel of a and a 4-neighbour pixel of b (right and down: each pair of pixels once)."""
    h, w = lab.shape
    n = {}
    for y in range(h):
        for x in range(w):
            l = int(lab[y, x])
            for yy, xx in ((y, x + 1), (y + 1, x)):
                if yy < h and xx < w:
                    m = int(lab[yy, xx])
                    if l > 0 and m > 0 and l != m:
                        key = (min(l, m), max(l, m))
                        n[key] = n.get(key, 0) + 1
    return sorted((a, b, c) for (a, b), c in n.items())


def as_lists(table):
    """An InstanceTable (tensors) as the dict of lists `tables` returns."""
    return {name: getattr(table, name).cpu().numpy().astype(np.int64).tolist() for name in table._fields if getattr(table, name) is not None}


def shape_fraction(lab, k):
    """Per label 1..k, from the pixels in exact arithmetic: None for an absent label, else a dict with the exact centroid and central moments
    (Fractions) and, computed from them in float64 at the very end, the eigenvalues and what follows from them."""
    out = []
    for l in range(1, k + 1):
        ys, xs = np.nonzero(lab == l)
        a = len(ys)
        if a == 0:
            out.append(None)
            continue
        xs, ys = [int(v) for v in xs], [int(v) for v in ys]
        cx, cy = Fraction(sum(xs), a), Fraction(sum(ys), a)
        u20 = sum((x - cx) ** 2 for x in xs) / a
        u02 = sum((y - cy) ** 2 for y in ys) / a
        u11 = sum((x - cx) * (y - cy) for x, y in zip(xs, ys)) / a
        rad = math.sqrt(float(((u20 - u02) / 2) ** 2 + u11 ** 2))
        mid = float((u20 + u02) / 2)
        l1, l2 = mid + rad, max(mid - rad, 0.0)
        out.append(dict(area=a, centroid=(float(cx), float(cy)), equivalent_diameter=math.sqrt(4 * a / math.pi), l1=l1, l2=l2,
                        major_axis_length=4 * math.sqrt(l1), minor_axis_length=4 * math.sqrt(l2),
                        eccentricity=math.sqrt(max(1 - l2 / l1, 0.0)) if l1 > 0 else 0.0,
                        orientation=0.5 * math.atan2(float(2 * u11), float(u20 - u02))))
    return out


def intensity_fraction(lab, k, img):
    """Per label and channel (mean, population std) from the pixels in exact arithmetic; None for an absent label."""
    h, w = lab.shape
    im = img.reshape(h, w, -1)
    out = []
    for l in range(1, k + 1):
        m = lab == l
        a = int(m.sum())
        if a == 0:
            out.append(None)
            continue
        row = []
        for j in range(im.shape[2]):
            v = [int(t) for t in im[:, :, j][m]]
            mean = Fraction(sum(v), a)
            var = sum((t - mean) ** 2 for t in v) / a
            row.append((float(mean), math.sqrt(float(var))))
        out.append(row)
    return out


def ellipse_scene(h=96, w=120):
    """Well separated ellipses of clearly different axes at several angles, one of them cut by the frame, one id left absent: a scene whose
    definition gives l1 - l2 > 1e-3 l1 for every instance."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    lab = np.zeros((h, w), np.int32)
    specs = [(20, 20, 14, 5, 0.0), (60, 22, 12, 6, 0.6), (100, 20, 15, 4, 1.3), (25, 60, 16, 7, -0.4), (70, 62, 10, 5, 2.2),
             (112, 70, 14, 6, 0.9), (40, 90, 18, 4, 0.1)]
    for i, (cx, cy, a, b, th) in enumerate(specs):
        u = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
        v = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
        lab[(u / a) ** 2 + (v / b) ** 2 < 1.0] = i + 1 if i < 5 else i + 2          # (id 6 stays absent)
    return lab, len(specs) + 1
