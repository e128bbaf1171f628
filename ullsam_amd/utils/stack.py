"""Z-stacks and time-lapse series: the per-plane instance label maps of a stack are linked along the third axis into 3-D objects.  Plane z calls
a cell 7 and plane z + 1 calls it 3; this module decides that they are one object.  It is the definition (numpy, integers only) and the driver of
the device route (csrc/stack.hip); the two are equal bit for bit (tests/test_stack_*.py).  DESIGN.md "7b, continued (stacks)" states the
definition and why it is what it is.

    volume, label_of_global, voxels, zrange, boxes = link_label_stack(planes, counts, iou=(1, 4), device="cuda")
    table = track_table(label_of_global, counts)        # [K, Z]: the local id of object k in plane z -> per-object series of per-plane rows
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import _lib
from .mosaic import MAX_IDS, _merge_components

MAX_PLANES = 65535
MAX_SIDE = 46340          # H * W < 2^31: areas, overlaps and unions fit 32 bits and n * u fits unsigned 64 (utils.measure's bound)
MODES = ("mutual", "all")


def _check_iou(iou) -> Tuple[int, int]:
    try:
        num, den = (int(v) for v in iou)
    except (TypeError, ValueError):
        raise ValueError(f"link_label_stack: iou must be a pair (num, den) of integers, got {iou!r}")
    if not 0 < num <= den < 2 ** 31:
        raise ValueError(f"link_label_stack: iou = (num, den) needs 0 < num <= den < 2^31, got {iou}")
    return num, den


def _bases(counts, nplanes: int, what: str = "link_label_stack") -> np.ndarray:
    k = (counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).astype(np.int64).reshape(-1)
    if len(k) != nplanes or (k < 0).any():
        raise ValueError(f"{what}: {len(k)} counts for {nplanes} planes (each >= 0)")
    base = np.concatenate([[0], np.cumsum(k)])
    if int(base[-1]) > MAX_IDS:
        raise _lib.UllsamError(f"{what}: {int(base[-1])} ids in all (at most 2^31 - 2)")
    return base


def _plane_pairs(a: np.ndarray, b: np.ndarray, ka: int, kb: int):
    """(local a, local b, n) of the distinct pairs a, b > 0 of two planes, ascending in (a, b)."""
    both = (a > 0) & (b > 0)
    key = a[both].astype(np.int64) * (kb + 1) + b[both]
    if (ka + 1) * (kb + 1) <= 1 << 24:
        cnt = np.bincount(key, minlength=1)
        uniq = np.nonzero(cnt)[0]
        n = cnt[uniq]
    else:
        uniq, n = np.unique(key, return_counts=True)
    return uniq // (kb + 1), uniq % (kb + 1), n.astype(np.int64)


def _best(group: np.ndarray, partner: np.ndarray, n: np.ndarray, u: np.ndarray, size: int) -> np.ndarray:
    """best int64 [size]: for every id, the index of the best candidate among those whose `group` end it is (-1: none).  The order is exact:
    n1 / u1 against n2 / u2 by n1 * u2 against n2 * u1 in unsigned 64-bit (n < 2^31, u < 2^32), equal ones by the smaller partner.  Round r
    offers every group's r-th candidate to the best so far, so a round holds one candidate per group and is one vectorised comparison."""
    best = np.full(size, -1, np.int64)
    if not len(group):
        return best
    order = np.argsort(group, kind="stable")
    gs = group[order]
    start = np.concatenate([[0], np.nonzero(gs[1:] != gs[:-1])[0] + 1])
    pos = np.arange(len(gs)) - np.repeat(start, np.diff(np.concatenate([start, [len(gs)]])))
    nu, uu = n.astype(np.uint64), u.astype(np.uint64)
    for r in range(int(pos.max()) + 1):
        c = order[pos == r]
        cur = best[group[c]]
        has = cur >= 0
        j = np.where(has, cur, c)
        left, right = nu[c] * uu[j], nu[j] * uu[c]
        better = ~has | (left > right) | ((left == right) & (partner[c] < partner[j]))
        best[group[c[better]]] = c[better]
    return best


def _link_host(planes: np.ndarray, base: np.ndarray, num: int, den: int, mode: str, min_planes: int, min_volume: int, max_pairs: int):
    Z, H, W = planes.shape
    g = int(base[-1])
    k = np.diff(base)
    for z in range(Z):
        if planes[z].size and (int(planes[z].min()) < 0 or int(planes[z].max()) > int(k[z])):
            raise _lib.UllsamError(f"link_label_stack: plane {z} holds an id outside 0..{int(k[z])}")
    flat = planes.reshape(Z, -1)
    # 1. areas and pair counts
    local = [np.bincount(flat[z], minlength=int(k[z]) + 1) for z in range(Z)]      # pixel counts by LOCAL id
    area = np.zeros(g + 1, np.int64)
    for z in range(Z):
        area[base[z] + 1:base[z + 1] + 1] = local[z][1:]
    pa, pb, pn, npairs = [], [], [], 0
    for z in range(Z - 1):
        la, lb, n = _plane_pairs(flat[z], flat[z + 1], int(k[z]), int(k[z + 1]))
        npairs += len(n)
        if npairs > max_pairs:
            raise _lib.UllsamError(f"link_label_stack: more than max_pairs = {max_pairs} distinct label pairs between consecutive planes")
        pa.append(la + base[z])
        pb.append(lb + base[z + 1])
        pn.append(n)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    a, b, n = cat(pa), cat(pb), cat(pn)
    u = area[a] + area[b] - n
    # 2. candidates
    cand = (n > 0) & (n * den >= num * u)
    a, b, n, u = a[cand], b[cand], n[cand], u[cand]
    # 3. + 4. ranking and links, 5. objects
    if mode == "mutual":
        idx = np.arange(len(a))
        linked = (_best(a, b, n, u, g + 1)[a] == idx) & (_best(b, a, n, u, g + 1)[b] == idx)
        rep = np.arange(g + 1, dtype=np.int64)
        rep[b[linked]] = a[linked]                       # at most one predecessor each: chains, walked by pointer jumping
        while True:
            nxt = rep[rep]
            if np.array_equal(nxt, rep):
                break
            rep = nxt
    else:
        rep = _merge_components(a, b, g)
    # voxels, plane range and box per representative
    big = np.iinfo(np.int32).max
    vox = np.zeros(g + 1, np.int64)
    lo = {name: np.full(g + 1, big, np.int64) for name in ("z", "x", "y")}
    hi = {name: np.full(g + 1, -1, np.int64) for name in ("z", "x", "y")}
    for z in range(Z):
        kz = int(k[z])
        ids = np.nonzero(local[z][1:])[0] + 1
        if not len(ids):
            continue
        ys, xs = np.nonzero(planes[z])
        lab = planes[z][ys, xs]
        r = rep[base[z] + ids]
        np.add.at(vox, r, local[z][ids])
        np.minimum.at(lo["z"], r, z)
        np.maximum.at(hi["z"], r, z)
        for name, vals in (("x", xs), ("y", ys)):
            mn, mx = np.full(kz + 1, big, np.int64), np.full(kz + 1, -1, np.int64)
            np.minimum.at(mn, lab, vals)
            np.maximum.at(mx, lab, vals)
            np.minimum.at(lo[name], r, mn[ids])
            np.maximum.at(hi[name], r, mx[ids])
    # 6. dropping and renumbering
    keep = (vox != 0) & (vox >= min_volume) & (hi["z"] - lo["z"] + 1 >= min_planes)
    keep[0] = False
    lmap = (np.cumsum(keep) * keep).astype(np.int32)
    log = lmap[rep]
    volume = np.zeros((Z, H, W), np.int32)
    for z in range(Z):
        lut = log[base[z]:base[z + 1] + 1].copy()
        lut[0] = 0
        volume[z] = lut[planes[z]]
    zrange = np.stack([lo["z"][keep], hi["z"][keep]], 1).astype(np.int32).reshape(-1, 2)
    boxes = np.stack([lo["x"][keep], lo["y"][keep], hi["x"][keep], hi["y"][keep]], 1).astype(np.int32).reshape(-1, 4)
    return volume, log, vox[keep], zrange, boxes


def link_label_stack(planes, counts, iou=(1, 4), mode: str = "mutual", min_planes: int = 1, min_volume: int = 0, max_pairs: int = 1 << 20,
                     device=None):
    """Per-plane instance label maps -> one label volume of 3-D objects.  planes int32 [Z, H, W] (a z-stack, or the frames of a time-lapse),
    counts[z] = K_z: plane z uses the ids 0..K_z, 0 = background; an id may be absent from its plane.  The global id of (z, l > 0) is
    base_z + l, base_z = the sum of K_s over s < z; G = the sum of all K_z (utils.mosaic's convention).

    1. Areas and pair counts: A(g) = the pixels of g in its own plane, over the whole plane.  For every two consecutive planes (z, z + 1) and
       a, b > 0: n(a, b) = #{p: plane_z(p) = a and plane_z+1(p) = b}, u(a, b) = A(a) + A(b) - n(a, b).
    2. (a, b) is a CANDIDATE iff n > 0 and n * den >= num * u, iou = (num, den): the IoU of the two labels' footprints is at least num / den.
       Equality qualifies.
    3. Candidates that share an end are ranked by IoU, compared exactly by cross-multiplication in 64-bit integers (n1 * u2 against n2 * u1; no
       float is formed anywhere); equal IoU is broken by the smaller partner id.  succ*(a) = the best candidate partner of a in the next
       plane, pred*(b) = the best candidate partner of b in the previous plane.
    4. mode="mutual" (default): (a, b) is linked iff succ*(a) = b and pred*(b) = a.  There is no second choice: a label whose best partner
       prefers another label stays unlinked at that side.  Every label then has at most one predecessor and one successor, so objects are
       chains with one label per plane.  mode="all": every candidate is a link; splits and merges fuse into one object (the mosaic's rule
       applied along z).
    5. Objects are the components of the link graph over 1..G, each represented by its SMALLEST global id = its first appearance in plane
       order.  Links join consecutive planes only, so an object occupies every plane from its first to its last.
    6. An object is dropped (its voxels become 0) when its voxel count is 0 or below min_volume, or when it spans fewer than min_planes
       planes (last - first + 1); the others are renumbered 1..K by ascending representative.

    The default threshold is (1, 4), not the mosaic's (1, 2): the two sides of a seam see the SAME pixels, two planes do not -- a cell's section
    grows, shrinks and drifts from plane to plane.  Above 1 / 2 a label can have only one candidate per side (two disjoint partners cannot both
    cover more than half of their union with it), so the ranking of step 3 only ever matters at thresholds <= 1 / 2.

    -> (volume int32 [Z, H, W], label_of_global int32 [G + 1] (0 for the background and for members of dropped objects), voxels int64 [K],
    zrange int32 [K, 2] (inclusive first and last plane), boxes int32 [K, 4] inclusive XYXY over all planes of the object), torch tensors on
    the chosen device.  1 <= Z <= 65535 and H, W <= 46340 (ValueError otherwise, as for any bad argument); more than max_pairs distinct
    pairs, G > 2^31 - 2 or an id outside 0..K_z raise UllsamError.  Z = 1, empty planes and K_z = 0 are valid.
    device None / "cpu": this definition in numpy.  A GPU device: csrc/stack.hip on the planes where they are (integer atomics only, so two runs
    are bit-equal; ONE read-back: the status words and K); `counts` is host data there (a GPU tensor costs a second read-back)."""
    num, den = _check_iou(iou)
    if mode not in MODES:
        raise ValueError(f"link_label_stack: mode must be one of {MODES}, got {mode!r}")
    min_planes, min_volume, max_pairs = int(min_planes), int(min_volume), int(max_pairs)
    if min_planes < 1 or min_volume < 0:
        raise ValueError(f"link_label_stack: min_planes >= 1 and min_volume >= 0, got {(min_planes, min_volume)}")
    if not 1 <= max_pairs <= 2 ** 30:
        raise ValueError(f"link_label_stack: max_pairs must lie in 1..2^30, got {max_pairs}")
    if len(planes.shape) != 3:
        raise ValueError(f"link_label_stack: planes must be [Z, H, W], got {tuple(planes.shape)}")
    Z, H, W = (int(v) for v in planes.shape)
    if not (1 <= Z <= MAX_PLANES and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"link_label_stack: planes {(Z, H, W)} must be [1..{MAX_PLANES}, 1..{MAX_SIDE}, 1..{MAX_SIDE}]")
    base = _bases(counts, Z)
    min_planes, min_volume = min(min_planes, 2 ** 31 - 1), min(min_volume, 2 ** 62)
    dev = torch.device("cpu" if device is None else device)
    if dev.type != "cuda":
        pl = planes.detach().cpu().numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
        out = _link_host(np.ascontiguousarray(pl.astype(np.int32)), base, num, den, mode, min_planes, min_volume, max_pairs)
        return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in out)
    from .. import ops
    pl = torch.as_tensor(planes, device=dev).to(torch.int32).contiguous()
    g = int(base[-1])
    base_d = torch.from_numpy(base.astype(np.int32)).to(dev)
    flags = torch.empty((ops.STACK_FLAGS,), dtype=torch.int32, device=dev)              # bad id | overflow | pairs | K: the one read-back
    keys, cnt, areas, _ = ops.stack_pairs(pl, base_d, g, max_pairs, flags=flags)
    if mode == "mutual":
        succ, pred, _ = ops.stack_best(keys, cnt, areas, g, (num, den), flags=flags)
        parent, _ = ops.stack_link(g, succ=succ, pred=pred, flags=flags)
    else:
        parent, _ = ops.stack_link(g, keys=keys, counts=cnt, areas=areas, iou=(num, den), flags=flags)
    vox_raw, zr_raw, box_raw, _ = ops.stack_stats(pl, base_d, g, parent, flags=flags)
    log, voxels, zrange, boxes, _ = ops.stack_compact(vox_raw, zr_raw, box_raw, parent, min_planes, min_volume, k_out=flags[3:])
    volume = ops.stack_relabel(pl, base_d, g, log)
    fl = flags.cpu().numpy()
    if fl[0]:
        raise _lib.UllsamError("link_label_stack: a plane holds an id outside 0..K_z")
    if fl[1] or fl[2] > max_pairs:
        raise _lib.UllsamError(f"link_label_stack: more than max_pairs = {max_pairs} distinct label pairs between consecutive planes")
    kk = int(fl[3])
    return volume, log, voxels[:kk], zrange[:kk], boxes[:kk]


def track_table(label_of_global, counts) -> torch.Tensor:
    """label_of_global (link_label_stack's) and the same counts -> int32 [K, Z] on the host: the LOCAL id of object k + 1 in plane z, 0 where the
    object is absent (or its label there is).  It is the index that gathers per-plane tables (utils.measure.measure_instances of every plane) into
    per-object series: row (z, table[k, z] - 1) of plane z's table for every z with table[k, z] > 0.  Raises UllsamError when an object holds two
    labels in one plane, which mode="all" allows (a split or a merge): such an object has no single row per plane."""
    log = (label_of_global.detach().cpu().numpy() if isinstance(label_of_global, torch.Tensor) else np.asarray(label_of_global)).astype(np.int64).reshape(-1)
    k = (counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).astype(np.int64).reshape(-1)
    base = _bases(k, len(k), "track_table")
    if len(log) != int(base[-1]) + 1:
        raise ValueError(f"track_table: label_of_global has {len(log)} entries for {int(base[-1])} ids")
    if (log < 0).any():
        raise ValueError("track_table: label_of_global holds a negative label")
    nobj = int(log.max()) if len(log) else 0
    table = np.zeros((nobj, len(k)), np.int32)
    for z in range(len(k)):
        obj = log[base[z] + 1:base[z + 1] + 1]
        local = np.nonzero(obj)[0] + 1
        obj = obj[local - 1]
        if len(np.unique(obj)) != len(obj):
            raise _lib.UllsamError(f"track_table: an object holds two labels in plane {z} (mode='all' fuses splits and merges)")
        table[obj - 1, z] = local
    return torch.from_numpy(table)
