"""Simplified outlines of an instance label image: Douglas-Peucker on label_outlines' loops with exact integer arithmetic and a rule that does not
depend on the direction of travel or on where a loop starts, so there is one answer per label image and the border two instances share comes out
as the same vertex sequence in both rings (watertight).  This module is the definition (numpy, integers only) and the driver of the device route
(csrc/simplify.hip); the two are equal bit for bit (tests/test_simplify_*.py).  DESIGN.md "7b, continued (simplifying)" states the definition, its
facts and the arguments for them.

    res = simplify_outlines(labels, tolerance=1.0, connectivity=8, device="cuda")
    res.outlines   # an Outlines of the surviving loops in their old order (parent re-indexed, edges still the source loop's crack length, loops_of
                   # recounted, vertices int32 (x, y)); polygons, to_geojson and rasterize_polygons take it as it is
    res.source     # int32 [L']: the row of every surviving loop in label_outlines' table

The definition in short (labels int32 [H, W], 0 = background, ids 1..K, sides at most 32767, H * W < 2^29; T = floor(tolerance * 256 + 1/2),
0 <= T <= 255 * 256):
  loops       exactly label_outlines' loops: same edges, leaders, travel order and order of loops.
  fixed       a lattice point is fixed when at least three of the four pixel sides that meet at it separate different values (the frame's outside
              is 0): the junctions of three or more values, and the saddles.
  candidates  of a loop, in travel order: the tails of its edges that are corners (as in label_outlines) or whose tail is a fixed point -- a loop
              that runs straight through a T-junction has the junction as a candidate.
  kept        at first every candidate on a fixed point.  A loop without one visits every lattice point at most once and gets two anchors: the
              candidate of smallest (y, x), and the one of largest squared distance from it, ties to the smallest (y, x).
  distance    of a candidate p to the chord a -> b of the kept candidates around it (cyclic in the loop), as num / den with L = |b - a|^2 and
              t = (p - a).(b - a):  L = 0: |p - a|^2 / 1;  t <= 0: |p - a|^2 L / L;  t >= L: |p - b|^2 L / L;  else cross(b - a, p - a)^2 / L.
              Every num is below 2^62 and T^2 den below 2^63 (sides at most 32767), so int64 holds them.
  rule        among the candidates strictly inside a segment take the one of largest num, ties to the smallest (y, x); keep it iff
              num * 65536 > T^2 den, computed as num > (T^2 den) >> 16 (strict: a candidate at exactly the tolerance goes).  Repeat on the two new
              segments until no segment adds a vertex; all segments are worked in rounds, which gives the same set as the recursion.
  rings       the kept candidates in travel order from the first at or after the leader's tail; area2 = the shoelace sum of the ring.  A loop is
              dropped when its ring has fewer than 3 vertices or area2 has not the strict sign of the source loop's; a hole goes with its parent.
Both routes take the same steps: flags per ordered edge slot, a compaction of the candidates, the anchors by a minimum and a maximum per loop, the
segments from a scan of the kept flags, rounds (a maximum, then a minimum per segment, then the winners), the ordered compaction of the kept.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from . import distance as D
from . import outline as O

MAX_SIDE = 32767
MAX_T = 255 * 256
ROUND_BLOCK = 4            # rounds before the first read-back of the round counters on the device route; every later block is twice as long,
ROUND_BLOCK_MAX = 64       # up to this (the rounds of a block after one that kept nothing return at once)
_NONE = np.int64(2 ** 63 - 1)


class Simplified(NamedTuple):
    outlines: O.Outlines
    source: torch.Tensor      # int32 [L']


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _ordered_host(lab: np.ndarray, connectivity: int):
    """label_outlines' stages up to the rank-ordered copy -> (reid int64 [E], corner bool [E], estart int64 [L]), as ops.outline_order gives them.
    A copy of the first half of outline._outline_host, which returns none of the three and is not to change: keep the two in step.  The host form
    therefore runs these stages twice, once there for the source table and once here."""
    mask = O._masks_host(lab)
    off, eid = O._edges_host(mask)
    e = len(eid)
    succ = O._successors_host(lab, mask, off, eid, connectivity)
    side = eid & 3
    pdir = np.zeros(e, np.int64)
    pdir[succ] = side
    leader, rank = O._rank_host(succ)
    lead = np.flatnonzero(leader == np.arange(e))
    lead = lead[np.argsort(lab.reshape(-1).astype(np.int64)[eid[lead] >> 2], kind="stable")]
    n_loops = len(lead)
    loop_of = np.zeros(e, np.int64)
    loop_of[lead] = np.arange(n_loops)
    loop = loop_of[leader]
    edges = np.bincount(loop, minlength=n_loops)[:n_loops]
    estart = np.cumsum(edges) - edges
    slot = estart[loop] + rank
    reid = np.zeros(e, np.int64)
    reid[slot] = eid
    corner = np.zeros(e, bool)
    corner[slot] = pdir != side
    return reid, corner, estart


def _num_host(px, py, ax, ay, bx, by):
    """(num, den) int64 of the candidates p against the chords a -> b"""
    ux, uy, vx, vy = bx - ax, by - ay, px - ax, py - ay
    length = ux * ux + uy * uy
    t = vx * ux + vy * uy
    cr = ux * vy - uy * vx
    da, db = vx * vx + vy * vy, (px - bx) ** 2 + (py - by) ** 2
    num = np.where(length == 0, da, np.where(t <= 0, da * length, np.where(t >= length, db * length, cr * cr)))
    return num, np.where(length == 0, 1, length)


def _simplify_host(lab: np.ndarray, t: int, reid: np.ndarray, corner: np.ndarray, estart: np.ndarray):
    """-> (vertices int64 [N, 2], vloop int64 [N], nvert int64 [L], area2 int64 [L], info): every loop's ring before any loop is dropped"""
    h, w = lab.shape
    e, n_loops = len(reid), len(estart)
    s, p = reid & 3, reid >> 2
    x, y = p % w + O.TAIL[s, 0], p // w + O.TAIL[s, 1]
    pad = np.zeros((h + 2, w + 2), np.int64)
    pad[1:-1, 1:-1] = lab
    a, b, c, d = pad[y, x], pad[y, x + 1], pad[y + 1, x], pad[y + 1, x + 1]          # the four pixels around the lattice point
    fixed = (a != b).astype(np.int64) + (c != d) + (a != c) + (b != d) >= 3
    cand = corner | fixed
    coff = np.cumsum(cand) - cand
    n_cand = int(cand.sum())
    slot_loop = np.searchsorted(estart, np.arange(e), side="right") - 1
    cx, cy, cloop, kept = x[cand], y[cand], slot_loop[cand], fixed[cand].copy()
    cstart = np.concatenate([coff[estart], [n_cand]]).astype(np.int64) if n_loops else np.zeros(1, np.int64)
    idx = np.arange(n_cand, dtype=np.int64)
    yx = cy << 16 | cx
    # the anchors of the loops without a fixed point
    nfixed = np.bincount(cloop[kept], minlength=n_loops)[:n_loops]
    free = nfixed[cloop] == 0
    amin = np.full(n_loops, _NONE, np.int64)
    np.minimum.at(amin, cloop[free], yx[free] << 32 | idx[free])
    first = (amin >> 32)[cloop]
    d2 = (cx - (first & 0xFFFF)) ** 2 + (cy - (first >> 16)) ** 2
    amax = np.zeros(n_loops, np.int64)
    np.maximum.at(amax, cloop[free], d2[free] << 32 | (0xFFFFFFFF - yx[free]))
    kept |= free & ((yx == first) | (yx == 0xFFFFFFFF - (amax[cloop] & 0xFFFFFFFF)))
    # the segments: the kept candidates before and after every other candidate, cyclic in its loop
    koff = np.cumsum(kept) - kept
    klist = np.flatnonzero(kept)
    pa, pb = np.full(n_cand, -1, np.int64), np.full(n_cand, -1, np.int64)
    if n_cand:
        ce = cstart[cloop + 1]
        k0, k1 = koff[cstart[cloop]], np.where(ce < n_cand, koff[np.minimum(ce, n_cand - 1)], len(klist))
        pa = np.where(kept, -1, klist[np.where(koff > k0, koff - 1, k1 - 1)])
        pb = np.where(kept, -1, klist[np.where(koff < k1, koff, k0)])
    rounds = 0
    while True:
        i = np.flatnonzero(pa >= 0)
        if not len(i):
            break
        sa, sb = pa[i], pb[i]
        num, den = _num_host(cx[i], cy[i], cx[sa], cy[sa], cx[sb], cy[sb])
        segmax = np.zeros(n_cand, np.int64)
        np.maximum.at(segmax, sa, num)
        win = (num == segmax[sa]) & (num > (t * t * den) >> 16)
        segwin = np.full(n_cand, _NONE, np.int64)
        np.minimum.at(segwin, sa[win], yx[i[win]] << 32 | i[win])
        wv = segwin[sa]
        none, wi = wv == _NONE, wv & 0xFFFFFFFF
        won = ~none & (wi == i)
        rest = ~none & ~won
        cs = cstart[cloop[i]]
        n = cstart[cloop[i] + 1] - cs
        before = rest & ((i - sa + n) % n < (wi - sa + n) % n)        # between a and the winner, in travel order
        after = rest & ~before
        kept[i[won]] = True
        pa[i[none | won]] = -1
        pb[i[before]] = wi[before]
        pa[i[after]] = wi[after]
        if not won.any():
            break
        rounds += 1
    # the rings
    klist = np.flatnonzero(kept)
    voff = np.cumsum(kept) - kept
    vloop = cloop[klist]
    nvert = np.bincount(vloop, minlength=n_loops)[:n_loops]
    area2 = np.zeros(n_loops, np.int64)
    if len(klist):
        ce = cstart[vloop + 1]
        k0, k1 = voff[cstart[vloop]], np.where(ce < n_cand, voff[np.minimum(ce, n_cand - 1)], len(klist))
        r = np.arange(len(klist))
        nxt = klist[np.where(r + 1 < k1, r + 1, k0)]
        np.add.at(area2, vloop, cx[klist] * cy[nxt] - cx[nxt] * cy[klist])
    vertices = np.stack([cx[klist], cy[klist]], 1).reshape(-1, 2)
    return vertices, vloop, nvert, area2, {"rounds": rounds, "candidates": n_cand}


# ---- what both routes share: the loops that survive ---------------------------------------------------------------------------------------------
def _finish(src: O.Outlines, vertices: torch.Tensor, vloop: torch.Tensor, nvert: torch.Tensor, area2: torch.Tensor, k: int) -> Simplified:
    """Tensors on one device.  Drops the loops whose ring has fewer than 3 vertices or not the strict sign of the source loop's area2, and the holes of
    dropped loops; re-indexes the rest."""
    dev = vertices.device
    keep = (nvert >= 3) & (torch.sign(area2) == torch.sign(src.area2)) & (area2 != 0)
    keep = keep & keep[src.parent.long()]                 # (a hole's parent is an outer loop, its own parent: one step is enough)
    new = (torch.cumsum(keep, 0) - 1).to(torch.int32)
    source = torch.nonzero(keep).reshape(-1).to(torch.int32)
    at = source.long()
    counts = nvert[at].to(torch.int32)
    start = torch.cat([torch.zeros((1,), dtype=torch.int32, device=dev), torch.cumsum(counts, 0).to(torch.int32)])
    label = src.label[at]
    loops_of = torch.bincount((label - 1).long(), minlength=k)[:k].to(torch.int32) if k else torch.zeros((0,), dtype=torch.int32, device=dev)
    out = O.Outlines(label, start, src.edges[at], area2[at], new[src.parent[at].long()], vertices[keep[vloop.long()]].to(torch.int32).reshape(-1, 2), loops_of)
    return Simplified(out, source)


# ---- the device route ---------------------------------------------------------------------------------------------------------------------------
def _ordered_device(lab: torch.Tensor, k: int, connectivity: int):
    """label_outlines' device stages -> (src, reid, corner, estart, n_vert): src is its Outlines with label, edges, area2 and parent filled and
    start, vertices and loops_of left empty (nothing here needs them), n_vert the number of its vertices.  The body is a copy of label_outlines'
    device driver up to outline_order plus outline_parents, because that function hands none of its intermediate tables out and is not to change:
    keep the two in step."""
    from .. import ops
    dev, w = lab.device, lab.shape[1]
    flags = torch.zeros((ops.OUTLINE_FLAGS,), dtype=torch.int32, device=dev)
    mask, off, _ = ops.outline_sides(lab, k, flags)
    fl = flags.cpu().tolist()                             # the status word, and E
    if fl[0]:
        raise _lib.UllsamError(f"simplify_outlines: the label image holds an id outside 0..{k}")
    e = fl[1]
    eid, succ, pdir, _ = ops.outline_successors(lab, mask, off, e, connectivity, flags)
    leader, rank, _ = ops.outline_rank(succ, eid, pdir, flags)
    lst, _ = ops.outline_collect(lab, eid, leader, min(e, (e + 3) // 4 + 1), flags)
    fl = flags.cpu().tolist()                             # L and N
    if fl[0]:
        raise _lib.UllsamError("simplify_outlines: an index left its table (the status word)")
    n_loops, n_vert = fl[3], fl[2]
    keys = torch.sort(lst[:n_loops]).values
    label = (keys >> 32).to(torch.int32)
    lead = (keys & 0xFFFFFFFF).to(torch.int32)
    loop_of = torch.empty((e,), dtype=torch.int32, device=dev)
    loop_of[lead.long()] = torch.arange(n_loops, dtype=torch.int32, device=dev)
    edges, area2, _ = ops.outline_loops(eid, leader, loop_of, n_loops, w, flags)
    estart = (torch.cumsum(edges, 0) - edges).to(torch.int32)
    reid, corner, _ = ops.outline_order(eid, pdir, leader, rank, loop_of, estart, flags)
    parent, _ = ops.outline_parents(lab, mask, off, eid, leader, loop_of, lead, area2, flags)
    none = torch.zeros((0,), dtype=torch.int32, device=dev)
    return O.Outlines(label, none, edges, area2, parent, none, none), reid, corner, estart, n_vert


def _simplify_device(lab: torch.Tensor, t: int, reid: torch.Tensor, corner: torch.Tensor, estart: torch.Tensor, block: int):
    from .. import ops
    dev = lab.device
    h, w = lab.shape
    flags = torch.zeros((ops.SIMPLIFY_FLAGS,), dtype=torch.int32, device=dev)
    cand, _ = ops.simplify_flags(lab, reid, corner, flags)
    coff, total = ops.outline_scan(cand)
    n_cand = int(total.cpu())                             # C
    cxy, cloop, kept, nfixed, _ = ops.simplify_candidates(reid, cand, coff, estart, n_cand, h, w, flags)
    cstart = torch.cat([coff[estart.long()], total])
    ops.simplify_anchors(cxy, cloop, nfixed, kept, flags)
    pa, pb, _ = ops.simplify_segments(kept, cloop, cstart, flags)
    rounds = 0
    while n_cand:
        got = ops.simplify_rounds(cxy, cloop, cstart, t, block, pa, pb, kept, flags)[0].cpu().tolist()   # one read-back for `block` rounds
        rounds += sum(1 for v in got if v)
        if got[-1] == 0:                                  # (a round that keeps nothing closes every open segment: the ones after it do nothing)
            break
        block = min(2 * block, max(block, ROUND_BLOCK_MAX))
    voff, total = ops.outline_scan(kept)
    n_vert = int(total.cpu())                             # N
    vertices, nvert, area2, _ = ops.simplify_rings(cxy, cloop, kept, voff, total, cstart, n_vert, flags)
    if int(flags.cpu()[0]):
        raise _lib.UllsamError("simplify_outlines: an index left its table (the status word)")
    return vertices, cloop[kept.bool()], nvert, area2, {"rounds": rounds, "candidates": n_cand}


# ---- the public function ------------------------------------------------------------------------------------------------------------------------
def _tolerance(tolerance) -> int:
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)) or not math.isfinite(float(tolerance)):
        raise ValueError(f"simplify_outlines: tolerance must be a finite number of pixels, got {tolerance!r}")
    t = math.floor(float(tolerance) * 256 + 0.5)
    if not 0 <= t <= MAX_T:
        raise ValueError(f"simplify_outlines: tolerance = {tolerance!r} must lie in 0..255 pixels")
    return int(t)


def _run(labels, tolerance, connectivity=8, num=None, device=None, block: int = ROUND_BLOCK):
    """simplify_outlines, and what the bench and the tests ask about the run: -> (Simplified, {"rounds", "candidates", "vertices" and "loops" (of the source)})"""
    shape = tuple(labels.shape) if hasattr(labels, "shape") else ()
    if len(shape) != 2 or min(shape) < 1 or max(shape) > MAX_SIDE or shape[0] * shape[1] >= O.MAX_PIXELS:
        raise ValueError(f"simplify_outlines: labels must be [H, W] with sides in 1..32767 and H * W < 2^29, got {shape}")
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"simplify_outlines: connectivity must be 4 or 8, got {connectivity!r}")
    connectivity, t = int(connectivity), _tolerance(tolerance)
    dev = D._route(labels, device)
    if dev.type != "cuda":
        lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        lab = np.ascontiguousarray(lab.astype(np.int32, copy=False))
        k = D._num(lab, num, "simplify_outlines")
        if int(lab.min()) < 0 or int(lab.max()) > k:
            raise _lib.UllsamError(f"simplify_outlines: the label image holds an id outside 0..{k}")
        src = O._pack(O._outline_host(lab, k, connectivity))
        res = _simplify_host(lab, t, *_ordered_host(lab, connectivity))
        vertices, vloop, nvert, area2 = (torch.from_numpy(np.ascontiguousarray(a)) for a in res[:4])
        info, n_src = res[4], int(src.vertices.shape[0])
    else:
        lab = D._device_labels(labels, dev)
        k = D._num(lab, num, "simplify_outlines")
        src, reid, corner, estart, n_src = _ordered_device(lab, k, connectivity)
        vertices, vloop, nvert, area2, info = _simplify_device(lab, t, reid, corner, estart, int(block))
    return _finish(src, vertices, vloop, nvert, area2, k), dict(info, vertices=n_src, loops=int(src.label.numel()))


def simplify_outlines(labels, tolerance, connectivity: int = 8, num: Optional[int] = None, device=None) -> Simplified:
    """label_outlines' loops of `labels` (int32 [H, W], 0 = background, ids 1..K, sides at most 32767, H * W < 2^29), simplified within `tolerance`
    pixels (snapped to T / 256, T = floor(tolerance * 256 + 1/2) in 0..255 * 256) -- the module's text states the definition, DESIGN.md its facts:
    tolerance 0 only adds the fixed points to label_outlines' vertices; every candidate of a loop lies within the tolerance of its ring; a border
    two instances share is the same vertex sequence in both rings.  -> Simplified(outlines, source int32 [L']).
    K = num (default labels.max()); an id outside 0..K raises UllsamError on both routes (a status word on the device route: nothing is indexed
    with it, and the next call works); every other bad argument raises ValueError.
    device None: where the labels are (numpy, CPU tensor: the numpy form; a GPU tensor: csrc/simplify.hip); "cpu" / a GPU device: that route.  The
    device route leaves every output on the device; it reads back label_outlines' two words, the candidate count, the round counters once per
    block of rounds (ROUND_BLOCK, then twice as many each time), and the vertex count."""
    return _run(labels, tolerance, connectivity, num, device)[0]
