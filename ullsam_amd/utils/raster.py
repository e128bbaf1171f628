"""Polygons to an instance label image: exact scanline rasterisation in fixed point, the inverse of utils.outline.  This module is the definition
(numpy, integers only) and the driver of the device route (csrc/raster.hip); the two are equal bit for bit (tests/test_raster_*.py).  DESIGN.md
"7b, continued (rasterising)" states the definition and its facts.

    r = rasterize_polygons(vertices, start, ring_label, (H, W), order="label", device="cuda")
    r.labels    # int32 [H, W]: the covering label of largest paint rank, 0 where none covers
    r.covered   # int32 [K]: the pixels of the frame inside label k, before overlaps
    r.area      # int32 [K]: the pixels that carry k in `labels`
    r.box       # int32 [K, 4]: their inclusive XYXY box, (INT_MAX, INT_MAX, -1, -1) where there are none (label_stats' convention)
    from_geojson(obj, pixel_size, origin) -> (vertices, start, ring_label, properties); labels_from_geojson(obj, size, ...): the two together.

The definition (pixel (x, y) is the square [x, x + 1] x [y, y + 1], its centre (x + 1/2, y + 1/2), y points down: the geometry of label_outlines):
  input      vertices [N, 2] as (x, y); start [R + 1]: ring r owns vertices[start[r] : start[r + 1]], open (the last vertex joins the first), at
             least 3 vertices; ring_label [R] in 1..K; size = (H, W), 1 <= H, W <= 32767; K <= 65535.  Ids are not renumbered.
  fixed      coordinates are snapped to 1/256 pixel, q = floor(v * 256 + 0.5) (float input: in float64 on the host; integer input: times 256
  point      where it lives); |q| <= 65535 * 256.  From here on everything is an integer; centres are (256 x + 128, 256 y + 128).
  crossings  edge (x0, y0) -> (x1, y1) with y0 != y1 crosses row y iff min(y0, y1) <= 256 y + 128 < max(y0, y1): half-open, a vertex on a scanline
             counts once; horizontal and zero-length edges cross nothing; rows outside 0..H - 1 are skipped.  The crossing toggles every pixel of
             the row whose centre is at or right of it: with the endpoints ordered by y, d = y1 - y0 > 0, cy = 256 y + 128,
             A = (x0 - 128) d + (cy - y0)(x1 - x0), B = 256 d, xs = clamp(ceil(A / B), 0, W) (|A| < 2^52); the pixels x >= xs toggle.  The value
             does not depend on the edge's direction: two polygons that share an edge share its crossings.
  coverage   pixel (x, y) is covered by label k iff the number of crossings of ALL rings of k in row y with xs <= x is odd (even-odd: holes need
             no orientation, a MultiPolygon is several rings of one label, a bow-tie has two lobes).  Sorted by xs the crossings of (k, y) are an
             even number; consecutive pairs are the spans [xs_a, xs_b).  A centre exactly on a left or top edge belongs to the polygon, one on a
             right or bottom edge does not.
  overlaps   labels[p] = the covering label of largest paint rank.  order="label": a larger id is on top; "area": ranks by `covered` descending,
             ties by ascending id, later on top (paint_ranks' rule: small objects end up on top).
  errors     ValueError (host): a ring with fewer than 3 vertices, non-finite coordinates, a start that is not 0 .. N in ascending steps, a bad
             size / order / num.  UllsamError (both routes; a status word on the device, nothing is indexed with the bad value, the next call
             works): a ring_label outside 1..K, a coordinate beyond the range, more than 2^31 - 1 crossings.  R = 0 gives an all-zero frame.
Both routes take the same steps: per edge its rows and their count, an exclusive scan (C crossings), one key label << 32 | row << 16 | xs per
crossing, a sort, covered per label from the spans, the ranks, atomicMax(raw, rank + 1) over every span, rank -> label with area and box.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from . import distance as D

SUB = 256                  # fixed point: 1/256 pixel
LIMIT = 65535 * SUB        # |q| at most
MAX_SIDE = 32767           # utils.distance's limit
MAX_IDS = 65535            # paint_label_map's limit
MAX_CROSSINGS = 2 ** 31 - 1
INT_MAX = 2 ** 31 - 1
ORDERS = ("label", "area")
PAINT = "waves"            # the default paint form of the device route (profiles/r21_raster.txt); "pixels" is the other


class Raster(NamedTuple):
    labels: torch.Tensor      # int32 [H, W]
    covered: torch.Tensor     # int32 [K]
    area: torch.Tensor        # int32 [K]
    box: torch.Tensor         # int32 [K, 4] inclusive XYXY


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _is_float(v) -> bool:
    return v.dtype.is_floating_point if isinstance(v, torch.Tensor) else np.asarray(v).dtype.kind == "f"


def _snap(vertices) -> np.ndarray:
    """q int64 [N, 2] on the host: floor(v * 256 + 0.5) in float64 for float input, v * 256 for integers (held at +-2^40: far beyond the range)."""
    v = _np(vertices)
    if v.dtype.kind not in "fiu":
        raise ValueError(f"rasterize_polygons: vertices of dtype {v.dtype}")
    if v.dtype.kind == "f":
        v = v.astype(np.float64)
        if not np.isfinite(v).all():
            raise ValueError("rasterize_polygons: a coordinate is not finite")
        return np.floor(np.clip(v, -2.0 ** 32, 2.0 ** 32) * SUB + 0.5).astype(np.int64)
    return np.clip(v.astype(np.int64), -2 ** 32, 2 ** 32) * SUB


def _check_start(start: np.ndarray, n: int):
    if start.ndim != 1 or len(start) < 1 or int(start[0]) != 0 or int(start[-1]) != n or (len(start) > 1 and int(np.diff(start).min()) < 3):
        raise ValueError("rasterize_polygons: start must run from 0 to N in steps of at least 3 (a ring has at least 3 vertices)")


def _integer(v, name: str) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"rasterize_polygons: {name} must be an integer, got {v!r}")
    return int(v)


def _size(size) -> Tuple[int, int]:
    try:
        h, w = (_integer(v, "size") for v in size)
    except TypeError:
        raise ValueError(f"rasterize_polygons: size must be (H, W), got {size!r}") from None
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"rasterize_polygons: a frame of {h} x {w} (each side must lie in 1..{MAX_SIDE})")
    return h, w


def _ids(ring_label, num) -> int:
    if num is None:
        count = ring_label.numel() if isinstance(ring_label, torch.Tensor) else ring_label.size
        k = max(int(ring_label.max()), 0) if count else 0
        if k > MAX_IDS:
            raise _lib.UllsamError(f"rasterize_polygons: a ring_label of {k} (at most {MAX_IDS} ids)")
        return k
    k = _integer(num, "num")
    if not 0 <= k <= MAX_IDS:
        raise ValueError(f"rasterize_polygons: num = {k} must lie in 0..{MAX_IDS}")
    return k


_STATUS = ((1, "a ring_label outside 1..K"), (2, "a coordinate beyond 65535 pixels"), (4, "more than 2^31 - 1 crossings"), (8, "an index left its table"))


def _raise_status(word: int, k: int):
    if word:
        raise _lib.UllsamError(f"rasterize_polygons (K = {k}): " + ", ".join(text for bit, text in _STATUS if word & bit))


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _ceil_sub(a: np.ndarray) -> np.ndarray:
    return -((-a) // SUB)


def _edges_host(q: np.ndarray, start: np.ndarray, ring_label: np.ndarray, h: int, k: int):
    """(row0, cnt, nxt, elab, off) int64 [N] and the status word: per edge the rows 0..H - 1 it crosses, its second vertex, its label, the scan"""
    n = len(q)
    ring_of = np.repeat(np.arange(len(ring_label), dtype=np.int64), np.diff(start))
    i = np.arange(n, dtype=np.int64)
    nxt = np.where(i + 1 < start[ring_of + 1], i + 1, start[ring_of]) if n else i
    lab = ring_label[ring_of]
    bad_lab = (lab < 1) | (lab > k)
    far = (np.abs(q) > LIMIT).any(1) if n else np.zeros(0, bool)
    bad_xy = ~bad_lab & (far | far[nxt])
    status = 1 * bool(bad_lab.any()) | 2 * bool(bad_xy.any())
    y0, y1 = q[:, 1], q[nxt, 1]
    lo = np.maximum(_ceil_sub(np.minimum(y0, y1) - 128), 0)
    hi = np.minimum(_ceil_sub(np.maximum(y0, y1) - 128), h)
    cnt = np.where(bad_lab | bad_xy, 0, np.maximum(hi - lo, 0))
    off = np.cumsum(cnt) - cnt
    if int(cnt.sum()) > MAX_CROSSINGS:
        status |= 4
    return np.where(cnt > 0, lo, 0), cnt, nxt, np.where(bad_lab | bad_xy, 0, lab), off, status


def _keys_host(q: np.ndarray, row0, cnt, nxt, elab, off, w: int) -> np.ndarray:
    """keys int64 [C] in edge order: label << 32 | row << 16 | xs"""
    e = np.repeat(np.arange(len(q), dtype=np.int64), cnt)
    y = row0[e] + np.arange(len(e), dtype=np.int64) - off[e]
    x0, y0, x1, y1 = q[e, 0], q[e, 1], q[nxt[e], 0], q[nxt[e], 1]
    flip = y0 > y1
    x0, x1, y0, y1 = np.where(flip, x1, x0), np.where(flip, x0, x1), np.where(flip, y1, y0), np.where(flip, y0, y1)
    cy = SUB * y + 128
    d = y1 - y0
    a = (x0 - 128) * d + (cy - y0) * (x1 - x0)
    xs = np.clip(-((-a) // (SUB * d)), 0, w)              # (floor division: the mathematical ceiling for either sign)
    return elab[e] << 32 | y << 16 | xs


def _spans(keys: np.ndarray):
    """the sorted keys -> (label, row, xa, length) int64 [C / 2]"""
    ka, kb = keys[0::2], keys[1::2]
    assert np.array_equal(ka >> 16, kb >> 16)             # closed rings: every (label, row) holds an even number of crossings
    return ka >> 32, (ka >> 16) & 0xFFFF, ka & 0xFFFF, (kb & 0xFFFF) - (ka & 0xFFFF)


def _ranks_host(covered: np.ndarray, order: str) -> np.ndarray:
    idx = np.arange(len(covered), dtype=np.int64)
    if order == "label":
        return idx
    rank = np.empty_like(idx)
    rank[np.lexsort((idx, -covered))] = idx
    return rank


def _paint_host(lab, row, xa, length, rank: np.ndarray, h: int, w: int) -> np.ndarray:
    """raw int64 [H, W] = 1 + the largest rank among the spans covering the pixel: the spans in ascending rank, every pixel assigned in that order"""
    raw = np.zeros(h * w, np.int64)
    value = rank[lab - 1] + 1
    o = np.argsort(value, kind="stable")
    n = length[o]
    first = row[o] * w + xa[o]
    pix = np.repeat(first - (np.cumsum(n) - n), n) + np.arange(int(n.sum()), dtype=np.int64)
    raw[pix] = np.repeat(value[o], n)                     # (a repeated index keeps the last value assigned: the largest)
    return raw.reshape(h, w)


def _finish_host(raw: np.ndarray, rank: np.ndarray, k: int):
    h, w = raw.shape
    label_of = np.zeros(k + 1, np.int64)
    label_of[rank + 1] = np.arange(1, k + 1)
    labels = label_of[raw]
    area = np.bincount(labels.reshape(-1), minlength=k + 1)[1:k + 1]
    box = np.tile(np.array([INT_MAX, INT_MAX, -1, -1], np.int64), (k, 1))
    ys, xs = np.nonzero(labels)
    at = labels[ys, xs] - 1
    np.minimum.at(box[:, 0], at, xs)
    np.minimum.at(box[:, 1], at, ys)
    np.maximum.at(box[:, 2], at, xs)
    np.maximum.at(box[:, 3], at, ys)
    return labels, area, box


def _raster_host(q: np.ndarray, start: np.ndarray, ring_label: np.ndarray, h: int, w: int, k: int, order: str):
    row0, cnt, nxt, elab, off, status = _edges_host(q, start, ring_label, h, k)
    _raise_status(status, k)
    keys = np.sort(_keys_host(q, row0, cnt, nxt, elab, off, w))
    lab, row, xa, length = _spans(keys)
    covered = np.zeros(k, np.int64)
    np.add.at(covered, lab - 1, length)
    rank = _ranks_host(covered, order)
    labels, area, box = _finish_host(_paint_host(lab, row, xa, length, rank, h, w), rank, k)
    return labels, covered, area, box


# ---- the public functions -----------------------------------------------------------------------------------------------------------------------
def _pack(res) -> Raster:
    return Raster(*(torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32) for a in res))


def rasterize_polygons(vertices, start, ring_label, size, order: str = "label", num: Optional[int] = None, device=None, paint: Optional[str] = None) -> Raster:
    """The instance label image of polygon rings -- the module's text states the definition, DESIGN.md its facts.  vertices [N, 2] as (x, y), float
    or integer pixels; start [R + 1]; ring_label [R] in 1..K; size = (H, W).  -> Raster(labels int32 [H, W], covered int32 [K], area int32 [K],
    box int32 [K, 4]).  K = num (default ring_label.max(): one more read-back where the labels live on the device).
    device None: where the vertices are (numpy, CPU tensor: the numpy form; a GPU tensor: csrc/raster.hip); "cpu" / a GPU device: that route.  The
    device route leaves every output on the device and reads back once (the status word with the crossing count); integer vertices on the device
    (Outlines.vertices) never visit the host, float ones are snapped there in float64.  paint: "waves" (one wave per span) or "pixels" (one lane
    per pixel over a scan of the span lengths; where C / 2 * W could pass 2^31 - 1 this form reads the status word once more) on the device route,
    default PAINT; both give the same frame."""
    h, w = _size(size)
    if order not in ORDERS:
        raise ValueError(f'rasterize_polygons: order must be "label" or "area", got {order!r}')
    if paint is not None and paint not in ("waves", "pixels"):
        raise ValueError(f'rasterize_polygons: paint must be "waves" or "pixels", got {paint!r}')
    if not hasattr(vertices, "shape"):
        vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 2) if len(vertices) else np.zeros((0, 2), np.float64)
    if len(vertices.shape) != 2 or vertices.shape[1] != 2:
        raise ValueError(f"rasterize_polygons: vertices must be [N, 2], got {tuple(vertices.shape)}")
    n = int(vertices.shape[0])
    dev = D._route(vertices, device)
    if dev.type != "cuda":
        q = _snap(vertices)
        st, rl = _np(start).astype(np.int64).reshape(-1), _np(ring_label).astype(np.int64).reshape(-1)
        _check_start(st, n)
        if len(rl) != len(st) - 1:
            raise ValueError(f"rasterize_polygons: {len(rl)} ring labels for {len(st) - 1} rings")
        return _pack(_raster_host(q, st, rl, h, w, _ids(rl, num), order))
    from .. import ops
    on_device = lambda t: isinstance(t, torch.Tensor) and t.is_cuda
    if on_device(vertices) and not _is_float(vertices):
        q = (vertices.to(dev).long() * SUB).clamp(-INT_MAX, INT_MAX).to(torch.int32).contiguous()
    else:
        q = torch.from_numpy(np.clip(_snap(vertices), -INT_MAX, INT_MAX).astype(np.int32)).to(dev)
    bad_start = None
    if on_device(start):                                  # checked where it lives: the verdict travels with the status word
        st = start.to(dev).reshape(-1).to(torch.int32).contiguous()
        if st.numel() < 1:
            raise ValueError("rasterize_polygons: start is empty")
        bad_start = (st[0] != 0) | (st[-1] != n)
        if st.numel() > 1:
            bad_start = bad_start | ((st[1:] - st[:-1]).min() < 3)
    else:
        st_h = _np(start).astype(np.int64).reshape(-1)
        _check_start(st_h, n)
        st = torch.from_numpy(st_h.astype(np.int32)).to(dev)
    rl = ring_label.to(dev).reshape(-1) if on_device(ring_label) else torch.from_numpy(np.clip(_np(ring_label).astype(np.int64).reshape(-1), -INT_MAX, INT_MAX)).to(dev)
    rl = rl.clamp(-INT_MAX, INT_MAX).to(torch.int32).contiguous()
    if rl.numel() != st.numel() - 1:
        raise ValueError(f"rasterize_polygons: {rl.numel()} ring labels for {st.numel() - 1} rings")
    k = _ids(rl, num)
    flags = torch.zeros((ops.RASTER_FLAGS,), dtype=torch.int32, device=dev)
    row0, cnt, nxt, elab, off, _ = ops.raster_edges(q, st, rl, h, w, k, flags)
    word = flags if bad_start is None else torch.cat([flags, bad_start.reshape(1).to(torch.int32)])
    fl = word.cpu().tolist()                              # the one read-back: the status word, C (and the verdict on a device start)
    if bad_start is not None and fl[-1]:
        raise ValueError("rasterize_polygons: start must run from 0 to N in steps of at least 3 (a ring has at least 3 vertices)")
    _raise_status(fl[0], k)
    keys, _ = ops.raster_keys(q, row0, cnt, nxt, elab, off, fl[1], h, w, k, flags)
    keys = torch.sort(keys).values                        # plumbing: a table of C rows
    covered, length, _ = ops.raster_covered(keys, h, w, k, flags)
    idx = torch.arange(k, dtype=torch.int32, device=dev)
    rank = idx
    if order == "area":                                   # a table of K rows: descending covered, ties by ascending id, later on top
        rank = torch.empty_like(idx)
        rank[torch.sort(-covered.long(), stable=True).indices] = idx
    form = PAINT if paint is None else paint
    raw, _ = ops.raster_paint(keys, rank, h, w, form, length, flags)
    if form == "pixels" and (fl[1] // 2) * w > INT_MAX:   # the scan of the span lengths may have left 31 bits: that form's own read-back
        _raise_status(int(flags.cpu()[0]), k)
    label_of = torch.zeros((k + 1,), dtype=torch.int32, device=dev)
    label_of[(rank + 1).long()] = idx + 1
    labels, area, box, _ = ops.raster_finish(raw, label_of, flags)
    return Raster(labels, covered, area, box)


def from_geojson(obj, pixel_size: float = 1.0, origin: Tuple[float, float] = (0.0, 0.0), label_key: str = "label"):
    """A GeoJSON FeatureCollection, Feature, or Polygon / MultiPolygon geometry (a dict, as json.loads gives it) -> (vertices float64 [N, 2], start
    int32 [R + 1], ring_label int32 [R], properties): every ring of every polygon -- exteriors and holes alike, the rule is even-odd -- with the
    closing vertex stripped and the coordinates mapped by (c - origin) / pixel_size, the inverse of to_geojson.  The label of a feature is
    properties[label_key], else its integer `id`, else 1, 2, ... in feature order; properties[k - 1] is the properties dict of label k ({} where
    there is none): the argument to_geojson takes."""
    kind = obj.get("type") if isinstance(obj, dict) else None
    if kind == "FeatureCollection":
        feats = list(obj.get("features", []))
    elif kind == "Feature":
        feats = [obj]
    elif kind in ("Polygon", "MultiPolygon"):
        feats = [{"type": "Feature", "geometry": obj, "properties": {}}]
    else:
        raise ValueError(f"from_geojson: a FeatureCollection, a Feature or a Polygon / MultiPolygon geometry, got type {kind!r}")
    ps, ox, oy = float(pixel_size), float(origin[0]), float(origin[1])
    if not (np.isfinite([ps, ox, oy]).all() and ps > 0):
        raise ValueError("from_geojson: pixel_size must be positive, and finite like the origin")
    rings, ring_label, by_label = [], [], {}
    for i, f in enumerate(feats):
        geom, props = f.get("geometry") or {}, f.get("properties") or {}
        if label_key in props:
            label = props[label_key]
        elif isinstance(f.get("id"), (int, np.integer)) and not isinstance(f.get("id"), bool):
            label = f["id"]
        else:
            label = i + 1
        if isinstance(label, bool) or not isinstance(label, (int, np.integer)):
            raise ValueError(f"from_geojson: feature {i} has the label {label!r} (an integer is needed)")
        if geom.get("type") == "Polygon":
            polys = [geom["coordinates"]]
        elif geom.get("type") == "MultiPolygon":
            polys = geom["coordinates"]
        else:
            raise ValueError(f"from_geojson: feature {i} has a geometry of type {geom.get('type')!r} (Polygon or MultiPolygon)")
        by_label.setdefault(int(label), {}).update(props)
        for poly in polys:
            for ring in poly:
                v = np.asarray([c[:2] for c in ring], dtype=np.float64).reshape(-1, 2)
                if len(v) > 1 and np.array_equal(v[0], v[-1]):
                    v = v[:-1]
                rings.append((v - (ox, oy)) / ps)
                ring_label.append(int(label))
    vertices = np.concatenate(rings) if rings else np.zeros((0, 2), np.float64)
    start = np.concatenate([[0], np.cumsum([len(v) for v in rings])]).astype(np.int32)
    k = max([l for l in by_label if l > 0], default=0)
    properties = [by_label.get(l, {}) for l in range(1, min(k, MAX_IDS) + 1)]
    return vertices, start, np.asarray(ring_label, np.int64).clip(-INT_MAX, INT_MAX).astype(np.int32), properties


def labels_from_geojson(obj, size, pixel_size: float = 1.0, origin: Tuple[float, float] = (0.0, 0.0), label_key: str = "label", order: str = "label",
                        num: Optional[int] = None, device=None, paint: Optional[str] = None) -> Raster:
    """from_geojson, then rasterize_polygons: GeoJSON annotations as an instance label image (device="cuda": on the GPU, where prompts_from_labels,
    measure_instances and instance_scores take it)."""
    vertices, start, ring_label, _ = from_geojson(obj, pixel_size, origin, label_key)
    return rasterize_polygons(vertices, start, ring_label, size, order, num, device, paint)
