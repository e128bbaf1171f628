"""Numpy definitions of the instance-label-map step, written from the definitions (DESIGN.md "7b, continued: instance label maps"), not from the
product code: the sequential overwrite, visible areas / boxes, the overlap table by np.add.at, brute-force instance matching, the integer nearest
rule -- and the case list the CPU and the GPU tests share."""
import math

import numpy as np


# ---- RLE (uncompressed, column-major, runs alternate 0, 1, 0, ... starting with a 0-run) ----------------------------------------------
def mask_to_rle(mask):
    h, w = mask.shape
    flat = np.asarray(mask, bool).T.reshape(-1)
    edges = np.concatenate([[0], np.nonzero(flat[1:] != flat[:-1])[0] + 1, [h * w]])
    counts = np.diff(edges).tolist()
    return {"size": [h, w], "counts": ([0] + counts) if flat[0] else counts}


def rle_to_mask(rle):
    h, w = rle["size"]
    flat = np.zeros(h * w, bool)
    pos, val = 0, False
    for c in rle["counts"]:
        flat[pos:pos + c] = val
        pos += c
        val = not val
    assert pos == h * w
    return flat.reshape(w, h).T


# ---- paint --------------------------------------------------------------------------------------------------------------------------------
def paint_order(masks, order, keys=None):
    """-> the record indices in paint order (first painted first)."""
    n = len(masks)
    if order == "record":
        return list(range(n))
    if order == "area":
        k = [int(m.sum()) for m in masks] if keys is None else list(keys)
        return sorted(range(n), key=lambda i: (-k[i], i))
    if order == "score":
        return sorted(range(n), key=lambda i: (float(keys[i]), i))
    raise ValueError(order)


def paint(masks, hw, order="record", keys=None, min_visible_area=0):
    """-> (labels int32 [H, W], label_of_record int32 [N], areas int32 [K], boxes int32 [K, 4] inclusive XYXY)."""
    h, w = hw
    n = len(masks)
    seq = paint_order(masks, order, keys)
    raw = np.zeros((h, w), np.int64)
    for r, i in enumerate(seq):                                   # the app's loop: later instances overwrite earlier ones
        raw[masks[i]] = r + 1
    labels = np.zeros((h, w), np.int32)
    of_record = np.zeros(n, np.int32)
    areas, boxes = [], []
    for r, i in enumerate(seq):
        vis = raw == r + 1
        a = int(vis.sum())
        if a == 0 or a < min_visible_area:
            continue                                              # dropped: its pixels stay 0, nothing underneath is re-exposed
        areas.append(a)
        labels[vis] = len(areas)
        of_record[i] = len(areas)
        ys, xs = np.nonzero(vis)
        boxes.append([xs.min(), ys.min(), xs.max(), ys.max()])
    return labels, of_record, np.asarray(areas, np.int32).reshape(-1), np.asarray(boxes, np.int32).reshape(-1, 4)


# ---- overlap / scores -----------------------------------------------------------------------------------------------------------------------
def overlap(a, b, na, nb):
    """T[i, j] = #{p: a[p] = i and b[p] = j}; pixels with an id outside 0..na / 0..nb are skipped.  -> (T, skipped pixel count)."""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    ok = (a >= 0) & (a <= na) & (b >= 0) & (b <= nb)
    t = np.zeros((na + 1, nb + 1), np.int64)
    np.add.at(t, (a[ok], b[ok]), 1)
    return t, int((~ok).sum())


def scores(table, thresholds):
    """Brute force over every (i, j) pair, i, j >= 1."""
    t = np.asarray(table, np.int64)
    aa, ab = t.sum(1), t.sum(0)
    n_pred, n_gt = int((aa[1:] > 0).sum()), int((ab[1:] > 0).sum())
    out = {k: [] for k in ("tp", "fp", "fn", "precision", "recall", "f1", "ap", "mean_matched_iou")}
    for th in thresholds:
        tp, matched = 0, []
        for i in range(1, t.shape[0]):
            for j in range(1, t.shape[1]):
                u = aa[i] + ab[j] - t[i, j]
                if u > 0 and float(t[i, j]) / float(u) > th:
                    tp += 1
                    matched.append(float(t[i, j]) / float(u))
        fp, fn = n_pred - tp, n_gt - tp
        out["tp"].append(tp); out["fp"].append(fp); out["fn"].append(fn)
        out["precision"].append(tp / (tp + fp) if tp + fp else 0.0)
        out["recall"].append(tp / (tp + fn) if tp + fn else 0.0)
        out["f1"].append(2 * tp / (2 * tp + fp + fn) if tp + fp + fn else 0.0)
        out["ap"].append(tp / (tp + fp + fn) if tp + fp + fn else 0.0)
        out["mean_matched_iou"].append(math.fsum(matched) / tp if tp else 0.0)     # (fsum: the exact sum, rounded once -- no order to agree on)
    return {k: np.asarray(v) for k, v in out.items()}


# ---- nearest resize ---------------------------------------------------------------------------------------------------------------------------
def nearest(x, out_hw, window=None):
    ih, iw = x.shape
    oh, ow = out_hw
    top, left, h, w = (0, 0, oh, ow) if window is None else window
    out = np.zeros((h, w), x.dtype)
    for y in range(h):
        sy = min(((2 * (top + y) + 1) * ih) // (2 * oh), ih - 1)
        for xx in range(w):
            out[y, xx] = x[sy, min(((2 * (left + xx) + 1) * iw) // (2 * ow), iw - 1)]
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
FRAMES = [(1, 1), (1, 37), (37, 1), (33, 65), (65, 33), (64, 64), (96, 160)]


def _disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def blobs(h, w, n, seed):
    """n seeded discs / rectangles; many are fully hidden under later ones."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if rng.random() < 0.5:
            out.append(_disc(h, w, rng.integers(0, h), rng.integers(0, w), int(rng.integers(1, max(2, min(h, w) // 3)))))
        else:
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            m = np.zeros((h, w), bool)
            m[y0:y0 + rng.integers(1, h // 2 + 2), x0:x0 + rng.integers(1, w // 2 + 2)] = True
            out.append(m)
    return out


def record_sets(h, w):
    """name -> list of boolean masks of one [h, w] frame."""
    z = lambda: np.zeros((h, w), bool)
    first = z(); first[0, 0] = True                               # a record whose first pixel is set (counts start with 0)
    span = np.zeros(h * w, bool); span[h // 2: h // 2 + min(3 * h + 1, h * w - h // 2)] = True       # one run over several whole columns
    span = span.reshape(w, h).T.copy()
    checker = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0 # runs of length 1
    r = max(1, min(h, w) // 2)
    nested = [_disc(h, w, h // 2, w // 2, rr) for rr in (r, max(r * 2 // 3, 0), max(r // 3, 0))]
    half_l = z(); half_l[:, : (w + 1) // 2] = True
    half_t = z(); half_t[: (h + 1) // 2, :] = True
    eq = [half_l, half_l[:, ::-1].copy(), half_t, half_t[::-1].copy()]      # equal areas in pairs: the tie rule
    sets = {
        "none": [],
        "empty": [z()],
        "full": [np.ones((h, w), bool)],
        "first_pixel": [first, checker],
        "span_columns": [span, first],
        "checker": [checker, ~checker, checker],
        "identical": [nested[0], nested[1], nested[1].copy(), first],   # the earlier of the two identical records vanishes: ids compact
        "nested": nested,
        "nested_reversed": nested[::-1],                                # in list order the large disc hides the others
        "equal_areas": eq,
        "mixed": [z(), np.ones((h, w), bool), span, checker, first] + nested,
    }
    if (h, w) == (96, 160):
        sets["blobs300"] = blobs(h, w, 300, 7)
    return sets


ORDERS = ("record", "area", "score", "permuted")


def paint_cases(h, w):
    """Every (name, masks, order, keys, min_visible_area) of one frame: all record sets x the three orders and a seeded permutation of the list
    under "record" x min_visible_area 0, 1 and the value that drops about half of the visible records."""
    rng = np.random.default_rng(h * 1000 + w)
    for name, masks in record_sets(h, w).items():
        n = len(masks)
        for order in ORDERS:
            ms, keys = masks, None
            if order == "permuted":
                ms = [masks[i] for i in rng.permutation(n)]
            if order == "score":
                keys = np.round(rng.random(n), 1).tolist()       # one decimal: ties
            o = "record" if order == "permuted" else order
            vis = paint(ms, (h, w), o, keys, 0)[2]
            half = int(np.median(vis)) + 1 if len(vis) else 2
            for mva in (0, 1, half):
                yield f"{name}/{order}/{mva}", ms, o, keys, mva
