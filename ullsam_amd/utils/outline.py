"""Outlines of an instance label image: every instance as closed polygon loops on the pixel lattice, outer loops and holes, with one answer per
label image.  This module is the definition (numpy, integers only) and the driver of the device route (csrc/outline.hip); the two are equal bit
for bit (tests/test_outline_*.py).  DESIGN.md "7b, continued (outlines)" states the definition and its facts.

    out = label_outlines(labels, connectivity=8, device="cuda")
    out.label      # int32 [L]: the label of every loop, loops ordered by (label, leader)
    out.start      # int32 [L + 1]: loop i owns vertices[start[i] : start[i + 1]]
    out.edges      # int32 [L]: the unit edges of the loop (its crack length)
    out.area2      # int64 [L]: the signed twice-area; > 0 an outer loop, < 0 a hole
    out.parent     # int32 [L]: the index of the enclosing outer loop (the loop itself for an outer loop)
    out.vertices   # int32 [N, 2]: (x, y) corners on the lattice 0..W x 0..H
    out.loops_of   # int32 [K]: loops per label (0: the id is absent)
    polygons(out, k) / to_geojson(out, pixel_size, origin, properties): the host exits (float64).

The definition in short (pixel (x, y) is the square [x, x + 1] x [y, y + 1], y points down, the frame's outside is "not k"):
  edges      side s of a pixel of label k > 0 whose 4-neighbour is not k is a directed unit edge, the instance on its right: 0 = top (east), 1 =
             right (south), 2 = bottom (west), 3 = left (north); its id is 4 * (y * W + x) + s.
  successor  the edge of the same label that starts at the head.  With AL / AR the pixels ahead-left / ahead-right of the head: connectivity 8
             turns left when AL == k, else goes straight when AR == k, else turns right; connectivity 4 turns right unless AR == k, and then
             left when AL == k too, else straight.  Left -> side (s + 3) % 4 of AL, straight -> side s of AR, right -> side (s + 1) % 4 of the
             same pixel.  The map is a permutation of the edges.
  loops      its cycles; the leader of a loop is its edge of smallest id, area2 the shoelace sum over its edges; loops are ordered by (label,
             leader).  The vertices are the tails of the edges whose predecessor has another direction, in travel order from the leader's tail.
  parent     of a hole: from the leader's pixel walk left while the pixel is k; the left side of the last one lies on a loop of k -- the parent
             when it is an outer loop, else repeat from that loop's leader.
Both routes take the same steps: side masks, an exclusive scan (the compact index of edge (p, s) is offset[p] + popcount(mask[p] & ((1 << s) - 1)),
so compact order is id order), successors by the local rule, pointer doubling on the cycles for (leader, rank), an ordered compaction.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from . import distance as D

MAX_PIXELS = 2 ** 29      # H * W below this: edge ids fit 31 bits


class Outlines(NamedTuple):
    label: torch.Tensor       # int32 [L]
    start: torch.Tensor       # int32 [L + 1]
    edges: torch.Tensor       # int32 [L]
    area2: torch.Tensor       # int64 [L]
    parent: torch.Tensor      # int32 [L]
    vertices: torch.Tensor    # int32 [N, 2] as (x, y)
    loops_of: torch.Tensor    # int32 [K]


# side -> the offsets (dx, dy) of the tail from the pixel's corner, of the pixel ahead-left and of the pixel ahead-right
TAIL = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.int64)
AHEAD_L = np.array([(1, -1), (1, 1), (-1, 1), (-1, -1)], np.int64)
AHEAD_R = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.int64)
_BELOW = np.array([[bin(m & ((1 << s) - 1)).count("1") for s in range(4)] for m in range(16)], np.int64)   # popcount(mask & ((1 << s) - 1))
_COUNT = np.array([bin(m).count("1") for m in range(16)], np.int64)


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _masks_host(lab: np.ndarray) -> np.ndarray:
    """mask int64 [H, W]: bit s = side s of a labelled pixel faces a pixel that is not of its label"""
    h, w = lab.shape
    pad = np.full((h + 2, w + 2), -1, np.int64)
    pad[1:-1, 1:-1] = lab
    c = pad[1:-1, 1:-1]
    on = c > 0
    mask = (on & (pad[:-2, 1:-1] != c)) * 1 + (on & (pad[1:-1, 2:] != c)) * 2 + (on & (pad[2:, 1:-1] != c)) * 4 + (on & (pad[1:-1, :-2] != c)) * 8
    return mask.astype(np.int64)


def _edges_host(mask: np.ndarray):
    """(off int64 [H * W], eid int64 [E]): the exclusive scan of the side counts, and the edge ids in compact (= id) order"""
    m = mask.reshape(-1)
    cnt = _COUNT[m]
    off = np.cumsum(cnt) - cnt
    bits = (m[:, None] >> np.arange(4)) & 1
    return off, np.flatnonzero(bits.reshape(-1))


def _successors_host(lab: np.ndarray, mask: np.ndarray, off: np.ndarray, eid: np.ndarray, connectivity: int) -> np.ndarray:
    """succ int64 [E], compact indices"""
    h, w = lab.shape
    pad = np.full((h + 2, w + 2), -1, np.int64)
    pad[1:-1, 1:-1] = lab
    p, s = eid >> 2, eid & 3
    x, y = p % w, p // w
    k = pad[y + 1, x + 1]
    lx, ly = x + AHEAD_L[s, 0], y + AHEAD_L[s, 1]
    rx, ry = x + AHEAD_R[s, 0], y + AHEAD_R[s, 1]
    al, ar = pad[ly + 1, lx + 1] == k, pad[ry + 1, rx + 1] == k
    if connectivity == 8:
        left, straight = al, ~al & ar
    else:
        left, straight = ar & al, ar & ~al
    tx = np.where(left, lx, np.where(straight, rx, x))
    ty = np.where(left, ly, np.where(straight, ry, y))
    ts = np.where(left, (s + 3) & 3, np.where(straight, s, (s + 1) & 3))
    tp = ty * w + tx
    return off[tp] + _BELOW[mask.reshape(-1)[tp], ts]


def _rounds(e: int) -> int:
    """ceil(log2 e): after that many doublings a window is at least as long as any cycle"""
    return max(int(e) - 1, 0).bit_length()


def _rank_host(succ: np.ndarray):
    """(leader, rank) int64 [E] by pointer doubling, never in place: after r rounds mn[e] is the smallest index among the 2^r edges from e on,
    pos[e] the steps from e to its first occurrence, jump[e] the edge 2^r steps ahead."""
    e = len(succ)
    idx = np.arange(e, dtype=np.int64)
    mn, pos, jump = idx.copy(), np.zeros(e, np.int64), succ.copy()
    for r in range(_rounds(e)):
        m2, p2 = mn[jump], pos[jump] + (1 << r)
        take = m2 < mn                                    # (a tie keeps the first half: the first occurrence)
        mn, pos, jump = np.where(take, m2, mn), np.where(take, p2, pos), jump[jump]
    length = np.zeros(e, np.int64)
    if e:
        length = pos[succ[mn]] + 1                        # the leader's successor is one step short of a whole turn
    return mn, np.where(pos == 0, 0, length - pos)


def _outline_host(lab: np.ndarray, k: int, connectivity: int):
    h, w = lab.shape
    mask = _masks_host(lab)
    off, eid = _edges_host(mask)
    e = len(eid)
    succ = _successors_host(lab, mask, off, eid, connectivity)
    side = eid & 3
    pdir = np.zeros(e, np.int64)
    pdir[succ] = side                                     # every edge tells its successor its direction
    leader, rank = _rank_host(succ)
    lead = np.flatnonzero(leader == np.arange(e))
    lab_of = lab.reshape(-1).astype(np.int64)[eid[lead] >> 2]
    lead = lead[np.argsort(lab_of, kind="stable")]        # (label, leader)
    label = lab.reshape(-1).astype(np.int64)[eid[lead] >> 2]
    n_loops = len(lead)
    loop_of = np.zeros(e, np.int64)
    loop_of[lead] = np.arange(n_loops)
    loop = loop_of[leader]
    x, y = (eid >> 2) % w, (eid >> 2) // w
    cross = np.choose(side, [-y, x + 1, y + 1, -x])
    edges = np.bincount(loop, minlength=n_loops)[:n_loops]
    area2 = np.zeros(n_loops, np.int64)
    np.add.at(area2, loop, cross)
    estart = np.cumsum(edges) - edges
    slot = estart[loop] + rank                            # rank order inside every loop's slice: compacting it gives the vertices
    reid = np.zeros(e, np.int64)
    reid[slot] = eid
    corner = np.zeros(e, bool)
    corner[slot] = pdir != side
    coff = np.cumsum(corner) - corner
    ceid = reid[corner]
    vertices = np.stack([(ceid >> 2) % w + TAIL[ceid & 3, 0], (ceid >> 2) // w + TAIL[ceid & 3, 1]], 1).reshape(-1, 2)
    start = np.concatenate([coff[estart], [int(corner.sum())]]) if n_loops else np.zeros(1, np.int64)
    # parents: all holes chase together, one hop per pass
    xs = np.broadcast_to(np.arange(w, dtype=np.int64), (h, w))
    head = np.ones((h, w), bool)
    head[:, 1:] = lab[:, 1:] != lab[:, :-1]
    run_x0 = np.maximum.accumulate(np.where(head, xs, 0), 1)      # the first column of every pixel's run
    parent = np.arange(n_loops, dtype=np.int64)
    todo = np.flatnonzero(area2 <= 0)
    mflat = mask.reshape(-1)
    while len(todo):
        p = eid[lead[parent[todo]]] >> 2
        q = (p // w) * w + run_x0.reshape(-1)[p]
        parent[todo] = loop_of[leader[off[q] + _BELOW[mflat[q], 3]]]
        todo = todo[area2[parent[todo]] <= 0]
    loops_of = np.bincount(label - 1, minlength=k)[:k] if k else np.zeros(0, np.int64)
    return label, start, edges, area2, parent, vertices, loops_of


# ---- the public function ------------------------------------------------------------------------------------------------------------------------
def _frame(labels) -> Tuple[int, int]:
    shape = tuple(labels.shape) if hasattr(labels, "shape") else ()
    if len(shape) != 2:
        raise ValueError(f"label_outlines: labels must be [H, W], got {shape}")
    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError(f"label_outlines: a frame of {h} x {w} (each side must be at least 1)")
    if h * w >= MAX_PIXELS:
        raise _lib.UllsamError(f"label_outlines: a frame of {h} x {w} has 2^29 pixels or more (edge ids are 31 bits)")
    return h, w


def _pack(res) -> Outlines:
    dt = (torch.int32, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32)
    return Outlines(*(torch.from_numpy(np.ascontiguousarray(a)).to(t) for a, t in zip(res, dt)))


def label_outlines(labels, connectivity: int = 8, num: Optional[int] = None, device=None) -> Outlines:
    """The polygon loops of every instance of `labels` (int32 [H, W], 0 = background, ids 1..K, H * W < 2^29; an instance need not be connected) --
    the module's text states the definition, DESIGN.md its facts.  connectivity 8 (the default, as split_labels' components) keeps two pixels
    that touch at a corner in one loop, 4 separates them.  -> Outlines(label int32 [L], start int32 [L + 1], edges int32 [L], area2 int64 [L],
    parent int32 [L], vertices int32 [N, 2], loops_of int32 [K]); a frame without a labelled pixel gives L = N = 0.
    K = num (default labels.max(): one more read-back on the device route); an id outside 0..K raises UllsamError on both routes (a status word on
    the device route: nothing is indexed with it, and the next call works).  A frame of 2^29 pixels or more raises UllsamError from its shape
    alone; other bad arguments raise ValueError.
    device None: where the labels are (numpy, CPU tensor: the numpy form; a GPU tensor: csrc/outline.hip); "cpu" / a GPU device: that route.  The
    device route leaves every output on the device and reads back twice: the status word with the edge count, then the loop and vertex counts."""
    h, w = _frame(labels)
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"label_outlines: connectivity must be 4 or 8, got {connectivity!r}")
    connectivity = int(connectivity)
    dev = D._route(labels, device)
    if dev.type != "cuda":
        lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        lab = np.ascontiguousarray(lab.astype(np.int32, copy=False))
        k = D._num(lab, num, "label_outlines")
        if int(lab.min()) < 0 or int(lab.max()) > k:
            raise _lib.UllsamError(f"label_outlines: the label image holds an id outside 0..{k}")
        return _pack(_outline_host(lab, k, connectivity))
    from .. import ops
    lab = D._device_labels(labels, dev)
    k = D._num(lab, num, "label_outlines")
    flags = torch.zeros((ops.OUTLINE_FLAGS,), dtype=torch.int32, device=dev)
    mask, off, _ = ops.outline_sides(lab, k, flags)
    fl = flags.cpu().tolist()                             # the status word, and E
    if fl[0]:
        raise _lib.UllsamError(f"label_outlines: the label image holds an id outside 0..{k}")
    e = fl[1]
    eid, succ, pdir, _ = ops.outline_successors(lab, mask, off, e, connectivity, flags)
    leader, rank, _ = ops.outline_rank(succ, eid, pdir, flags)
    lst, _ = ops.outline_collect(lab, eid, leader, min(e, (e + 3) // 4 + 1), flags)   # (a loop has at least 4 edges)
    fl = flags.cpu().tolist()                             # L and N
    if fl[0]:
        raise _lib.UllsamError("label_outlines: an index left its table (the status word)")
    n_loops, n_vert = fl[3], fl[2]
    keys = torch.sort(lst[:n_loops]).values               # tables of L rows from here on: (label, leader)
    label = (keys >> 32).to(torch.int32)
    lead = (keys & 0xFFFFFFFF).to(torch.int32)
    loop_of = torch.empty((e,), dtype=torch.int32, device=dev)
    loop_of[lead.long()] = torch.arange(n_loops, dtype=torch.int32, device=dev)
    edges, area2, _ = ops.outline_loops(eid, leader, loop_of, n_loops, w, flags)
    estart = (torch.cumsum(edges, 0) - edges).to(torch.int32)
    reid, corner, _ = ops.outline_order(eid, pdir, leader, rank, loop_of, estart, flags)
    coff, _ = ops.outline_scan(corner)
    vertices = ops.outline_vertices(reid, corner, coff, n_vert, w)
    start = torch.cat([coff[estart.long()], torch.full((1,), n_vert, dtype=torch.int32, device=dev)])
    parent, _ = ops.outline_parents(lab, mask, off, eid, leader, loop_of, lead, area2, flags)
    loops_of = torch.bincount((label - 1).long(), minlength=k)[:k].to(torch.int32) if k else torch.zeros((0,), dtype=torch.int32, device=dev)
    return Outlines(label, start, edges, area2, parent, vertices, loops_of)


# ---- the host exits -----------------------------------------------------------------------------------------------------------------------------
def _np(t) -> np.ndarray:
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.int64)


def _polygons(out: Outlines) -> dict:
    """{label: [(exterior, [holes])]}: one pass over the loops (holes follow their label's outer loops only in index, so two sweeps)"""
    label, start, area2, parent, verts = _np(out.label), _np(out.start), _np(out.area2), _np(out.parent), _np(out.vertices).astype(np.float64)
    res, at = {}, {}
    for i in np.flatnonzero(area2 > 0):
        at[int(i)] = (verts[start[i]:start[i + 1]], [])
        res.setdefault(int(label[i]), []).append(at[int(i)])
    for i in np.flatnonzero(area2 < 0):
        at[int(parent[i])][1].append(verts[start[i]:start[i + 1]])
    return res


def polygons(out: Outlines, k: int) -> List[Tuple[np.ndarray, List[np.ndarray]]]:
    """The polygons of label k: [(exterior float64 [n, 2], [hole float64 [m, 2], ...])], one per outer loop in loop order; rings are open (the
    last vertex joins the first), the exterior runs clockwise on the screen (y down) and the holes the other way."""
    return _polygons(out).get(int(k), [])


def to_geojson(out: Outlines, pixel_size: float = 1.0, origin: Tuple[float, float] = (0.0, 0.0), properties=None) -> dict:
    """A GeoJSON FeatureCollection (a dict; json.dumps writes it): one Feature per present label with id = label and a MultiPolygon geometry, one
    polygon per outer loop with its holes (by `parent`) after it; rings are closed (first vertex = last), coordinates are origin + vertex *
    pixel_size in float64.  properties: a sequence of dicts, properties[k - 1] is merged into the feature of label k."""
    ps, ox, oy = float(pixel_size), float(origin[0]), float(origin[1])
    ring = lambda v: [[ox + float(x) * ps, oy + float(y) * ps] for x, y in np.concatenate([v, v[:1]])]
    feats, by_label = [], _polygons(out)
    for k in np.flatnonzero(_np(out.loops_of) > 0) + 1:
        k = int(k)
        props = {"label": k}
        if properties is not None:
            props.update(properties[k - 1])
        coords = [[ring(ext)] + [ring(hl) for hl in holes] for ext, holes in by_label[k]]
        feats.append({"type": "Feature", "id": k, "properties": props, "geometry": {"type": "MultiPolygon", "coordinates": coords}})
    return {"type": "FeatureCollection", "features": feats}
