"""Exact squared Euclidean distance transforms of instance label VOLUMES with anisotropic voxels -- utils.distance with a third axis and a spacing:
how far a voxel is from the surface of its object, which object a background voxel is nearest to, objects grown and shrunk by a ball, the deepest
voxel of every object.  This module is the definition (numpy, integers only) and the driver of the device route (csrc/distance3d.hip); the two
are equal bit for bit (tests/test_distance3d_*.py).  DESIGN.md "7b, continued (3-D distances)" states the definitions, the limits and why the
transform separates exactly.

    volume, records, objects = generator.generate_stack_label_volume(stack)  # SamAutomaticMaskGenerator: int32 [Z, H, W] on the device, or
    volume = link_label_stack(planes, counts, device="cuda")[0]              # utils.stack, from any per-plane label maps: one id per 3-D object
    depth = object_depth(volume, spacing=(5, 2, 2))                          # planes 2.5 times as far apart as pixels: r2 [K], xyz [K, 3]
    d2 = inner_distance3d(volume, spacing=(5, 2, 2))                         # int32 [Z, H, W]: squared distance to the nearest voxel of another label
    d2, nearest = background_feature3d(volume, spacing=(5, 2, 2))            # every voxel: squared distance to the nearest labelled voxel, its label
    cells = expand_labels3d(nuclei, distance=8, spacing=(5, 2, 2))           # grown by a ball of radius 8 (in spacing units), ties to the smaller id
    cores = shrink_labels3d(volume, distance=4, spacing=(5, 2, 2))           # erosion by a ball per object, nothing merges

spacing = (sz, sy, sx) holds positive integers and |p - q|^2 = sz^2 dz^2 + sy^2 dy^2 + sx^2 dx^2; a ratio such as 2.5 : 1 is (5, 2, 2).  edge is a
bool or a triple (ez, ey, ex): where set, the voxels just outside the volume along that axis count as another label.  Everything is squared and
integer; INF = 2^31 - 1 says "no such voxel".
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .distance import INF, MAX_SIDE, _device_labels, _host_labels, _integer, _num, _radius2, _raise_bad, _route, _run_ends, _t

MAX_VOXELS = 2 ** 31 - 1  # the linear index of a voxel fits 32 bits
MAX_SPACING = 46340       # s^2 < 2^31
MAX_B = 2 ** 31 - 2       # B = sum of s_a^2 (n_a - 1 + e_a)^2, the largest squared distance a call can meet: every finite result fits int32


class ObjectDepth(NamedTuple):
    r2: torch.Tensor      # int32 [K]: the largest inner_distance3d over the voxels of object k + 1 (0: the id is absent)
    xyz: torch.Tensor     # int32 [K, 3]: (x, y, z) of the first voxel in (z, y, x) raster order that attains it ((-1, -1, -1): absent)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def _edges(edge, what: str) -> Tuple[bool, bool, bool]:
    if isinstance(edge, (bool, np.bool_)):
        return (bool(edge),) * 3
    try:
        e = tuple(edge)
    except TypeError:
        e = ()
    if len(e) != 3 or not all(isinstance(v, (bool, np.bool_)) for v in e):
        raise ValueError(f"{what}: edge must be a bool or a triple of bools (ez, ey, ex), got {edge!r}")
    return tuple(bool(v) for v in e)


def _metric(volume, spacing, edge, what: str):
    """-> ((Z, H, W), (sz, sy, sx), (ez, ey, ex)), every limit checked before any voxel is read (a stub with a .shape is enough)."""
    shape = tuple(volume.shape) if hasattr(volume, "shape") else ()
    if len(shape) != 3:
        raise ValueError(f"{what}: volume must be [Z, H, W], got {shape}")
    n = tuple(int(v) for v in shape)
    for v in n:
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: a volume of {n[0]} x {n[1]} x {n[2]}: the side {v} must lie in 1..{MAX_SIDE}")
    if n[0] * n[1] * n[2] > MAX_VOXELS:
        raise ValueError(f"{what}: a volume of {n[0]} x {n[1]} x {n[2]} = {n[0] * n[1] * n[2]} voxels (at most 2^31 - 1)")
    try:
        s = tuple(spacing)
    except TypeError:
        s = ()
    if len(s) != 3:
        raise ValueError(f"{what}: spacing must be a triple (sz, sy, sx), got {spacing!r}")
    for v in s:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: the spacing {v!r} must be an integer (a ratio such as 2.5 : 1 is given as (5, 2, 2))")
        if not 1 <= int(v) <= MAX_SPACING:
            raise ValueError(f"{what}: the spacing {v} must lie in 1..{MAX_SPACING}")
    s = tuple(int(v) for v in s)
    e = _edges(edge, what)
    b = sum(sa * sa * (na - 1 + int(ea)) ** 2 for sa, na, ea in zip(s, n, e))
    if b > MAX_B:
        raise ValueError(f"{what}: the largest squared distance of this volume and spacing, {b}, must be at most 2^31 - 2")
    return n, s, e


def _reach(limit: int, s: int) -> int:
    """floor(sqrt(limit) / s): a voxel farther along an axis than this is beyond limit already."""
    return math.isqrt(limit // (s * s))


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _inner_pass(lab: np.ndarray, cost: np.ndarray, axis: int, w: int, edge: bool, maxd: Optional[int]) -> np.ndarray:
    """One pass of the inner transform along `axis` (weight w = s^2).  cost int64 = the result of the passes before (INF: none; all INF for the
    first pass).  Within the run of equal label around a voxel: min(w * (distance to either run end + 1)^2 -- an open end only when the edge
    counts --, min over the run of w * d^2 + cost).  Background voxels give 0."""
    n = lab.shape[axis]
    last = lambda v: np.moveaxis(v, axis, -1)
    before, after, ob, oa = (last(v) for v in _run_ends(lab, axis))    # the run [p - before + 1, p + after - 1] of equal label around p
    c = last(cost)
    best = c.copy()
    for d, opened in ((before, ob), (after, oa)):
        term = w * d * d
        if not edge:
            term = np.where(opened, INF, term)
        best = np.minimum(best, term)
    best[last(lab) <= 0] = 0
    reach = n - 1 if maxd is None else min(int(maxd), n - 1)
    if bool((c < INF).any()):
        for d in range(1, reach + 1):
            wd = w * d * d
            if wd >= int(best.max()):                     # no voxel can still improve (best only falls)
                break
            cand = np.minimum(wd + c[..., :-d], INF)      # the voxel d before, where it belongs to the run
            best[..., d:] = np.where(before[..., d:] > d, np.minimum(best[..., d:], cand), best[..., d:])
            cand = np.minimum(wd + c[..., d:], INF)
            best[..., :-d] = np.where(after[..., :-d] > d, np.minimum(best[..., :-d], cand), best[..., :-d])
    return np.ascontiguousarray(np.moveaxis(best, -1, axis))


def _inner_host(lab: np.ndarray, s, e, limit: Optional[int] = None) -> np.ndarray:
    """D2 int64 [Z, H, W] (INF where no voxel of another label exists).  limit = r2: no scan looks farther than floor(sqrt(r2) / s_a) voxels -- a
    candidate farther along the line is above r2 already, so the result exceeds r2 exactly where D2 does (what shrink_labels3d needs)."""
    cost = np.full(lab.shape, INF, np.int64)
    for axis in range(3):
        cost = _inner_pass(lab, cost, axis, s[axis] * s[axis], e[axis], None if limit is None else _reach(limit, s[axis]))
    return np.minimum(cost, INF)


def _feature_pass(bd: np.ndarray, bl: np.ndarray, axis: int, w: int, maxd: int):
    """One pass of the feature transform along `axis`: the lexicographic minimum of (w * d^2 + bd(line voxel), bl(line voxel)) over the line."""
    n = bd.shape[axis]
    d0, l0 = np.moveaxis(bd, axis, -1), np.moveaxis(bl, axis, -1)
    nd, nl = d0.copy(), l0.copy()
    for d in range(1, min(maxd, n - 1) + 1):
        wd = w * d * d
        if wd > int(nd.max()):                            # (> and not >=: a tie with a smaller id must still be seen)
            break
        for dst, src in ((np.s_[..., d:], np.s_[..., :-d]), (np.s_[..., :-d], np.s_[..., d:])):
            c = np.minimum(wd + d0[src], INF)
            better = (c < nd[dst]) | ((c == nd[dst]) & (c < INF) & (l0[src] < nl[dst]))
            nd[dst] = np.where(better, c, nd[dst])
            nl[dst] = np.where(better, l0[src], nl[dst])
    return np.ascontiguousarray(np.moveaxis(nd, -1, axis)), np.ascontiguousarray(np.moveaxis(nl, -1, axis))


def _feature_host(lab: np.ndarray, s, limit: int) -> Tuple[np.ndarray, np.ndarray]:
    bd = np.where(lab > 0, 0, INF).astype(np.int64)
    bl = lab.astype(np.int64)
    for axis in range(3):
        bd, bl = _feature_pass(bd, bl, axis, s[axis] * s[axis], _reach(limit, s[axis]))
    far = bd > limit
    bd[far] = INF
    bl[far] = 0
    return bd, bl


def _depth_host(lab: np.ndarray, d2: np.ndarray, k: int):
    if lab.size and int(lab.max()) > k:
        raise ValueError(f"object_depth: the label volume holds an id outside 0..{k}")
    _, h, w = lab.shape
    idx = np.flatnonzero(lab)
    ids = lab.reshape(-1)[idx].astype(np.int64) - 1
    d = d2.reshape(-1)[idx]
    r2 = np.zeros(k, np.int64)
    np.maximum.at(r2, ids, d)
    top = d == r2[ids]
    first = np.full(k, -1, np.int64)
    order = np.argsort(-idx[top], kind="stable")          # descending index: the smallest one is written last
    first[ids[top][order]] = idx[top][order]
    xyz = np.where(first[:, None] >= 0, np.stack([first % w, (first // w) % h, first // (w * h)], 1), -1)
    return r2.astype(np.int32), xyz.astype(np.int32).reshape(k, 3)


def _limit(max_distance2, what: str) -> int:
    if max_distance2 is None:
        return INF
    limit = _integer(max_distance2, "max_distance2", what)
    if not 0 <= limit < INF:
        raise ValueError(f"{what}: max_distance2 = {limit} must lie in 0..2^31 - 2")
    return limit


# ---- the public functions -----------------------------------------------------------------------------------------------------------------------
def inner_distance3d(volume, spacing=(1, 1, 1), edge=False, device=None) -> torch.Tensor:
    """D2 int32 [Z, H, W].  volume int32 [Z, H, W], 0 = background, ids 1..K (some may be absent), an object need not be connected.  For a voxel p
    of object i > 0: D2[p] = the smallest |p - q|^2 over the voxels q of the volume with volume[q] != i (the background is not i), and, where
    edge is set for axis a, (s_a (p_a + 1))^2 and (s_a (n_a - p_a))^2: the voxels just outside the volume along a.  A voxel with no such q and
    no edge term gets INF; background voxels get 0.  For edge=False this is rint(scipy.ndimage.distance_transform_edt(volume == i,
    sampling=spacing)^2) on the voxels of i.
    Limits (ValueError, stating the number): 1 <= Z, H, W <= 32767; Z * H * W <= 2^31 - 1; 1 <= s_a <= 46340; B = sum over the axes of
    s_a^2 (n_a - 1 + e_a)^2 <= 2^31 - 2 (e_a = 1 where the edge counts), which keeps every finite result in int32.  A negative id: ValueError on
    the host route, UllsamError on the device route.
    device None: where the volume is (numpy, CPU tensor: the numpy definition; a GPU tensor: csrc/distance3d.hip, used where it is -- the volume
    of link_label_stack goes in without a host trip); "cpu" / a GPU device: that route.  The device route reads one status word back."""
    n, s, e = _metric(volume, spacing, edge, "inner_distance3d")
    dev = _route(volume, device)
    if dev.type != "cuda":
        return _t(_inner_host(_host_labels(volume, "inner_distance3d"), s, e))
    from .. import ops
    vol = _device_labels(volume, dev)
    g, _, flags = ops.distance3d_z(vol, False, e[0])
    h, _ = ops.distance3d_y(vol, g, None, s, e)
    d2, _ = ops.distance3d_x(vol, h, None, "inner", s, e, flags=flags)
    _raise_bad(flags, "inner_distance3d")
    return d2


def background_feature3d(volume, spacing=(1, 1, 1), max_distance2: Optional[int] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(D2 int32 [Z, H, W], nearest int32 [Z, H, W]).  For every voxel p: D2[p] = the smallest |p - q|^2 over the labelled voxels q, nearest[p] =
    the SMALLEST id among all q that attain it.  A labelled voxel gets (0, its id); a volume without a labelled voxel gets (INF, 0) everywhere.
    max_distance2 = m (in spacing units, squared): a voxel with D2 > m reports (INF, 0), the others are unchanged; None is exact over the whole
    volume (on the device its scans walk up to H and W voxels a voxel of a nearly empty volume)."""
    n, s, e = _metric(volume, spacing, False, "background_feature3d")
    limit = _limit(max_distance2, "background_feature3d")
    dev = _route(volume, device)
    if dev.type != "cuda":
        bd, bl = _feature_host(_host_labels(volume, "background_feature3d"), s, limit)
        return _t(bd), _t(bl)
    from .. import ops
    vol = _device_labels(volume, dev)
    g, near, flags = ops.distance3d_z(vol, True)
    h, hl = ops.distance3d_y(vol, g, near, s, e, limit=limit)
    out, _ = ops.distance3d_x(vol, h, hl, "feature", s, e, limit=limit, flags=flags)
    _raise_bad(flags, "background_feature3d")
    return out


def expand_labels3d(volume, distance=1, distance2: Optional[int] = None, spacing=(1, 1, 1), device=None) -> torch.Tensor:
    """int32 [Z, H, W]: every object grown into the background by a ball, without growing into another object.  r2 = distance2 if given, else
    distance^2 (distance an integer >= 0), in spacing units: with spacing (5, 2, 2), distance=8 reaches 4 voxels along x and y and 1 along z.
    out[p] = volume[p] where that is > 0; otherwise background_feature3d's nearest[p] where D2[p] <= r2; otherwise 0."""
    n, s, e = _metric(volume, spacing, False, "expand_labels3d")
    r2 = _radius2(distance, distance2, "expand_labels3d")
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host_labels(volume, "expand_labels3d")
        _, bl = _feature_host(vol, s, r2)
        return _t(np.where(vol > 0, vol, bl))
    from .. import ops
    vol = _device_labels(volume, dev)
    g, near, flags = ops.distance3d_z(vol, True)
    h, hl = ops.distance3d_y(vol, g, near, s, e, limit=r2)
    out, _ = ops.distance3d_x(vol, h, hl, "expand", s, e, limit=r2, flags=flags)
    _raise_bad(flags, "expand_labels3d")
    return out


def shrink_labels3d(volume, distance=1, distance2: Optional[int] = None, spacing=(1, 1, 1), edge=False, device=None) -> torch.Tensor:
    """int32 [Z, H, W]: out[p] = volume[p] where inner_distance3d(volume, spacing, edge)[p] > r2, else 0 (r2 as in expand_labels3d): erosion by
    the ball {d : |d|^2 <= r2} per object.  Objects never merge, and one that touches another is eroded from that side too."""
    n, s, e = _metric(volume, spacing, edge, "shrink_labels3d")
    r2 = _radius2(distance, distance2, "shrink_labels3d")
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host_labels(volume, "shrink_labels3d")
        return _t(np.where(_inner_host(vol, s, e, r2) > r2, vol, 0))
    from .. import ops
    vol = _device_labels(volume, dev)
    g, _, flags = ops.distance3d_z(vol, False, e[0])
    h, _ = ops.distance3d_y(vol, g, None, s, e, limit=r2)
    out, _ = ops.distance3d_x(vol, h, None, "shrink", s, e, limit=r2, flags=flags)
    _raise_bad(flags, "shrink_labels3d")
    return out


def object_depth(volume, num: Optional[int] = None, spacing=(1, 1, 1), edge=False, device=None) -> ObjectDepth:
    """ObjectDepth(r2 int32 [K], xyz int32 [K, 3]), K = num (default volume.max(): one more read-back on the device route).  r2[i - 1] = the
    largest inner_distance3d(volume, spacing, edge) over the voxels of i -- the squared radius of its largest inscribed ball, a thickness --,
    xyz[i - 1] = (x, y, z) of the first voxel in (z, y, x) raster order that attains it: the deepest interior voxel, a seed.  An absent id gets 0
    and (-1, -1, -1).  An id outside 0..K raises ValueError on the host route and UllsamError on the device route (a status word; the id is
    skipped)."""
    n, s, e = _metric(volume, spacing, edge, "object_depth")
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host_labels(volume, "object_depth")
        k = _num(vol, num, "object_depth")
        r2, xyz = _depth_host(vol, _inner_host(vol, s, e), k)
        return ObjectDepth(torch.from_numpy(r2), torch.from_numpy(xyz))
    from .. import ops
    vol = _device_labels(volume, dev)
    k = _num(vol, num, "object_depth")
    g, _, flags = ops.distance3d_z(vol, False, e[0], num=k)
    h, _ = ops.distance3d_y(vol, g, None, s, e)
    best, _ = ops.distance3d_x(vol, h, None, "depth", s, e, num=k, flags=flags)
    r2, xyz = ops.distance3d_depth_decode(best, n[1], n[2])
    _raise_bad(flags, "object_depth", k)
    return ObjectDepth(r2, xyz)
