"""Exact squared Euclidean distance transforms of instance label images, and what the microscopy workflow builds on them: how far a pixel is from
the edge of its instance, which instance a background pixel is nearest to, labels grown and shrunk by a disc, the deepest pixel of every instance.
This module is the definition (numpy, integers only) and the driver of the device route (csrc/distance.hip); the two are equal bit for bit
(tests/test_distance_*.py).  DESIGN.md "7b, continued (distances)" states the definitions and why the transform separates exactly.

    d2 = inner_distance(labels, device="cuda")                    # int32 [H, W]: squared distance to the nearest pixel of another label
    d2, nearest = background_feature(labels, device="cuda")       # every pixel: squared distance to the nearest labelled pixel, and its label
    cells = expand_labels(nuclei, distance=8, device="cuda")      # skimage.segmentation.expand_labels, ties to the smaller id
    cores = shrink_labels(labels, distance=4, device="cuda")      # erosion by a disc per instance, nothing merges
    depth = instance_depth(labels, device="cuda")                 # r2 [K], xy [K, 2]: the largest inscribed disc of every instance

Everything is squared and integer: a caller who wants pixels takes the square root.  INF = 2^31 - 1 says "no such pixel".
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _lib

INF = 2 ** 31 - 1
MAX_SIDE = 32767          # every finite squared distance <= 2 * 32766^2 < INF
MAX_IDS = 2 ** 31 - 2


class InstanceDepth(NamedTuple):
    r2: torch.Tensor      # int32 [K]: the largest inner_distance over the pixels of instance k + 1 (0: the id is absent)
    xy: torch.Tensor      # int32 [K, 2]: (x, y) of the first pixel in row-major order that attains it ((-1, -1): absent)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def _frame(labels, what: str) -> Tuple[int, int]:
    shape = tuple(labels.shape) if hasattr(labels, "shape") else ()
    if len(shape) != 2:
        raise ValueError(f"{what}: labels must be [H, W], got {shape}")
    h, w = (int(v) for v in shape)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"{what}: a frame of {h} x {w} (each side must lie in 1..{MAX_SIDE})")
    return h, w


def _integer(v, name: str, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what}: {name} must be an integer, got {v!r} (a radius that is no integer goes through distance2)")
    return int(v)


def _radius2(distance, distance2, what: str) -> int:
    if distance2 is not None:
        r2 = _integer(distance2, "distance2", what)
    else:
        d = _integer(distance, "distance", what)
        if d < 0:
            raise ValueError(f"{what}: distance must be >= 0, got {d}")
        r2 = d * d
    if not 0 <= r2 < INF:
        raise ValueError(f"{what}: the squared radius {r2} must lie in 0..2^31 - 2")
    return r2


def _route(labels, device) -> torch.device:
    """None: where the labels are (numpy and CPU tensors: the host form)."""
    if device is None:
        return labels.device if isinstance(labels, torch.Tensor) else torch.device("cpu")
    return torch.device(device)


def _host_labels(labels, what: str) -> np.ndarray:
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    lab = np.ascontiguousarray(lab.astype(np.int32, copy=False))
    if lab.size and int(lab.min()) < 0:
        raise ValueError(f"{what}: the label image holds a negative id")
    return lab


def _device_labels(labels, dev) -> torch.Tensor:
    return torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()


def _raise_bad(flags: torch.Tensor, what: str, k=None):
    if int(flags.cpu()[0]):                               # the one read-back of the call
        raise _lib.UllsamError(f"{what}: the label image holds " + ("a negative id" if k is None else f"an id outside 0..{k}"))


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _run_ends(lab: np.ndarray, axis: int):
    """Along `axis`: (before, after, open_before, open_after) int64 / bool [H, W].  before = the distance from a pixel to the first pixel with another
    label towards index 0, after = towards the far end; where the run of equal labels reaches the frame's end the distance is the one to the pixel just
    outside the frame and open_* is set."""
    a = np.moveaxis(lab, axis, 0)
    n = a.shape[0]
    pos = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (a.ndim - 1))

    def towards_zero(v):
        change = np.ones(v.shape, bool)
        change[1:] = v[1:] != v[:-1]
        start = np.maximum.accumulate(np.where(change, pos, 0), axis=0)
        return pos - start + 1, start == 0
    before, ob = towards_zero(a)
    after, oa = towards_zero(a[::-1])
    mv = lambda v: np.moveaxis(v, 0, axis)
    return mv(before), mv(after[::-1]), mv(ob), mv(oa[::-1])


def _inner_host(lab: np.ndarray, edge: bool, maxdx: Optional[int] = None) -> np.ndarray:
    """D2 int64 [H, W] (INF where no pixel of another label exists).  maxdx = isqrt(r2): scan no farther than that many columns -- a candidate farther
    along the row is above r2 already, so the result exceeds r2 exactly where D2 does (what shrink_labels needs)."""
    h, w = lab.shape
    inside = lab > 0
    up, down, oup, odown = _run_ends(lab, 0)
    if not edge:
        up[oup] = INF
        down[odown] = INF
    g = np.minimum(up, down)
    g2 = np.where(g >= INF, INF, g * g)
    left, right, oleft, oright = _run_ends(lab, 1)        # the run [x - left + 1, x + right - 1] of equal label around x
    best = g2.copy()
    for d, opened in ((left, oleft), (right, oright)):
        term = d * d
        if not edge:
            term = np.where(opened, INF, term)
        best = np.minimum(best, term)
    best[~inside] = 0
    reach = w - 1 if maxdx is None else min(int(maxdx), w - 1)
    for dx in range(1, reach + 1):
        if dx * dx >= int(best.max()):                    # no pixel can still improve (best only falls)
            break
        c = dx * dx + g2[:, :-dx]                         # the pixel dx to the left, where it belongs to the run
        best[:, dx:] = np.where(left[:, dx:] > dx, np.minimum(best[:, dx:], c), best[:, dx:])
        c = dx * dx + g2[:, dx:]
        best[:, :-dx] = np.where(right[:, :-dx] > dx, np.minimum(best[:, :-dx], c), best[:, :-dx])
    return np.minimum(best, INF)


def _feature_columns_host(lab: np.ndarray):
    """(g2 int64 [H, W], near int64 [H, W]): the squared vertical distance to the nearest labelled pixel of the column (INF: none) and its label, the
    smaller one at equal distance above and below."""
    h, w = lab.shape
    pos = np.arange(h, dtype=np.int64)[:, None]
    cols = np.arange(w)[None, :]

    def above(v):
        at = np.maximum.accumulate(np.where(v > 0, pos, -1), axis=0)
        return np.where(at >= 0, pos - at, INF), np.where(at >= 0, v[np.maximum(at, 0), cols], 0).astype(np.int64)
    du, lu = above(lab)
    dd, ld = above(lab[::-1])
    dd, ld = dd[::-1], ld[::-1]
    take = (dd < du) | ((dd == du) & (ld < lu))
    g = np.where(take, dd, du)
    return np.where(g >= INF, INF, g * g), np.where(take, ld, lu)


def _feature_host(lab: np.ndarray, limit: int) -> Tuple[np.ndarray, np.ndarray]:
    h, w = lab.shape
    g2, near = _feature_columns_host(lab)
    bd, bl = g2.copy(), near.copy()
    reach = min(math.isqrt(limit), w - 1)
    for dx in range(1, reach + 1):
        if dx * dx > int(bd.max()):
            break
        for dst, src in ((np.s_[:, dx:], np.s_[:, :-dx]), (np.s_[:, :-dx], np.s_[:, dx:])):
            c = np.minimum(dx * dx + g2[src], INF)
            better = (c < bd[dst]) | ((c == bd[dst]) & (c < INF) & (near[src] < bl[dst]))
            bd[dst] = np.where(better, c, bd[dst])
            bl[dst] = np.where(better, near[src], bl[dst])
    far = bd > limit
    bd[far] = INF
    bl[far] = 0
    return bd, bl


def _depth_host(lab: np.ndarray, d2: np.ndarray, k: int):
    if lab.size and int(lab.max()) > k:
        raise ValueError(f"instance_depth: the label image holds an id outside 0..{k}")
    w = lab.shape[1]
    idx = np.flatnonzero(lab)
    ids = lab.reshape(-1)[idx].astype(np.int64) - 1
    d = d2.reshape(-1)[idx]
    r2 = np.zeros(k, np.int64)
    np.maximum.at(r2, ids, d)
    top = d == r2[ids]
    first = np.full(k, -1, np.int64)
    order = np.argsort(-idx[top], kind="stable")          # descending index: the smallest one is written last
    first[ids[top][order]] = idx[top][order]
    xy = np.where(first[:, None] >= 0, np.stack([first % w, first // w], 1), -1)
    return r2.astype(np.int32), xy.astype(np.int32).reshape(k, 2)


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))


def _num(labels, num, what: str) -> int:
    if num is None:
        return max(int(labels.max()), 0)                  # (a frame has at least one pixel; one read-back on the device route)
    k = _integer(num, "num", what)
    if not 0 <= k <= MAX_IDS:
        raise ValueError(f"{what}: num = {k} must lie in 0..2^31 - 2")
    return k


# ---- the public functions -----------------------------------------------------------------------------------------------------------------------
def inner_distance(labels, edge: bool = False, device=None) -> torch.Tensor:
    """D2 int32 [H, W].  labels int32 [H, W], 0 = background, an instance need not be connected.  For a pixel p of instance i > 0: D2[p] = the smallest
    |p - q|^2 over the pixels q of the frame with labels[q] != i (the background is not i).  edge=True: the pixels just outside the frame are not i
    either -- they contribute (x + 1)^2, (W - x)^2, (y + 1)^2, (H - y)^2, the convention of d1 in utils.prompts.  edge=False: an instance that fills the
    frame has no such q and D2 = INF.  Background pixels get 0.  For edge=False this is rint(scipy.ndimage.distance_transform_edt(labels == i)^2)
    on the pixels of i.  1 <= H, W <= 32767 (ValueError, as for a negative id on the host route; the device route raises UllsamError for that).
    device None: where the labels are (numpy, CPU tensor: the numpy definition; a GPU tensor: csrc/distance.hip); "cpu" / a GPU device: that route.
    The result lives where it was computed; the device route reads one status word back."""
    _frame(labels, "inner_distance")
    dev = _route(labels, device)
    if dev.type != "cuda":
        return _t(_inner_host(_host_labels(labels, "inner_distance"), bool(edge)))
    from .. import ops
    lab = _device_labels(labels, dev)
    g, _, flags = ops.distance_columns(lab, False, edge)
    d2, _ = ops.distance_rows(lab, g, None, "inner", edge, flags=flags)
    _raise_bad(flags, "inner_distance")
    return d2


def background_feature(labels, max_distance2: Optional[int] = None, device=None, route: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """(D2 int32 [H, W], nearest int32 [H, W]).  For every pixel p: D2[p] = the smallest |p - q|^2 over the labelled pixels q, nearest[p] = the SMALLEST
    label among all q that attain it (symmetric, independent of any scan order; scipy's feature transform returns some minimiser).  A labelled pixel
    gets (0, its label); a frame without a labelled pixel gets (INF, 0) everywhere.  max_distance2 = m: a pixel with D2 > m reports (INF, 0), the
    others are unchanged; None is exact over the whole frame (on the device its scan walks up to W columns a pixel on a nearly empty frame).
    route (device only): "auto", "lds", "global" -- where the row pass reads from (ops.distance_rows); the outputs do not depend on it."""
    _frame(labels, "background_feature")
    limit = INF
    if max_distance2 is not None:
        limit = _integer(max_distance2, "max_distance2", "background_feature")
        if not 0 <= limit < INF:
            raise ValueError(f"background_feature: max_distance2 = {limit} must lie in 0..2^31 - 2")
    dev = _route(labels, device)
    if dev.type != "cuda":
        bd, bl = _feature_host(_host_labels(labels, "background_feature"), limit)
        return _t(bd), _t(bl)
    from .. import ops
    lab = _device_labels(labels, dev)
    g, near, flags = ops.distance_columns(lab, True)
    out, _ = ops.distance_rows(lab, g, near, "feature", limit=limit, route=route, flags=flags)
    _raise_bad(flags, "background_feature")
    return out


def expand_labels(labels, distance=1, distance2: Optional[int] = None, device=None, route: str = "auto") -> torch.Tensor:
    """int32 [H, W]: every label grown into the background by a disc, without growing into another label.  r2 = distance2 if given, else distance^2
    (distance an integer >= 0; other radii go through distance2).  out[p] = labels[p] where that is > 0; otherwise background_feature's nearest[p]
    where D2[p] <= r2; otherwise 0.  This is skimage.segmentation.expand_labels except on exact ties -- a background pixel equally near to two
    labels --, where skimage inherits the unspecified choice of scipy's feature transform and this function takes the smaller id."""
    _frame(labels, "expand_labels")
    r2 = _radius2(distance, distance2, "expand_labels")
    dev = _route(labels, device)
    if dev.type != "cuda":
        lab = _host_labels(labels, "expand_labels")
        _, bl = _feature_host(lab, r2)
        return _t(np.where(lab > 0, lab, bl))
    from .. import ops
    lab = _device_labels(labels, dev)
    g, near, flags = ops.distance_columns(lab, True)
    out, _ = ops.distance_rows(lab, g, near, "expand", limit=r2, route=route, flags=flags)
    _raise_bad(flags, "expand_labels")
    return out


def shrink_labels(labels, distance=1, distance2: Optional[int] = None, edge: bool = False, device=None, route: str = "auto") -> torch.Tensor:
    """int32 [H, W]: out[p] = labels[p] where inner_distance(labels, edge)[p] > r2, else 0 (r2 as in expand_labels).  Per instance this is
    scipy.ndimage.binary_erosion(labels == i, disc) with the disc {d : |d|^2 <= r2}; border_value=0 is edge=True, border_value=1 is edge=False.
    Instances never merge, and one that touches another is eroded from that side too."""
    _frame(labels, "shrink_labels")
    r2 = _radius2(distance, distance2, "shrink_labels")
    dev = _route(labels, device)
    if dev.type != "cuda":
        lab = _host_labels(labels, "shrink_labels")
        return _t(np.where(_inner_host(lab, bool(edge), math.isqrt(r2)) > r2, lab, 0))
    from .. import ops
    lab = _device_labels(labels, dev)
    g, _, flags = ops.distance_columns(lab, False, edge)
    out, _ = ops.distance_rows(lab, g, None, "shrink", edge, limit=r2, route=route, flags=flags)
    _raise_bad(flags, "shrink_labels")
    return out


def instance_depth(labels, num: Optional[int] = None, edge: bool = False, device=None) -> InstanceDepth:
    """InstanceDepth(r2 int32 [K], xy int32 [K, 2]), K = num (default labels.max(): one more read-back on the device route).  r2[i - 1] = the largest
    inner_distance(labels, edge) over the pixels of i -- the squared radius of its largest inscribed disc, a thickness --, xy[i - 1] = (x, y) of the
    first pixel in row-major order that attains it: the deepest interior pixel, the natural place of a positive click.  An absent id gets 0 and
    (-1, -1).  An id outside 0..K raises ValueError on the host route and UllsamError on the device route (a status word; the id is skipped)."""
    _frame(labels, "instance_depth")
    dev = _route(labels, device)
    if dev.type != "cuda":
        lab = _host_labels(labels, "instance_depth")
        k = _num(lab, num, "instance_depth")
        r2, xy = _depth_host(lab, _inner_host(lab, bool(edge)), k)
        return InstanceDepth(torch.from_numpy(r2), torch.from_numpy(xy))
    from .. import ops
    lab = _device_labels(labels, dev)
    k = _num(lab, num, "instance_depth")
    g, _, flags = ops.distance_columns(lab, False, edge, num=k)
    best, _ = ops.distance_rows(lab, g, None, "depth", edge, num=k, flags=flags)
    r2, xy = ops.distance_depth_decode(best, lab.shape[1])
    _raise_bad(flags, "instance_depth", k)
    return InstanceDepth(r2, xy)
