"""Splitting the touching objects of an instance label image: a watershed of every instance's own depth map (utils.distance.inner_distance),
defined without a flood so that it has exactly one answer.  This module is the definition (numpy, integers only) and the driver of the device route
(csrc/split.hip); the two are equal bit for bit (tests/test_split_*.py).  DESIGN.md "7b, continued (splitting)" states the definition and its facts.

    parts = split_labels(labels, min_depth=2, device="cuda")
    parts.labels      # int32 [H, W]: the parts, numbered 1..K' by (old id, index of the part's deepest pixel)
    parts.parent      # int32 [K']: the old id of every part
    parts.peak_r2     # int32 [K']: the largest inner_distance over the part -- the squared radius of its largest inscribed disc
    parts.peak_xy     # int32 [K', 2]: (x, y) of the first pixel in row-major order that attains it
    parts.parts_of    # int32 [K]: how many parts every old id was cut into (0: the id is absent)

The definition in short (D2 = inner_distance, p = the row-major index, key(p) = (D2[p], -p), a strict total order):
  ascent   up(p) = the pixel of greatest key among p and its 8 neighbours with p's label; a root has up(p) = p; basin(p) = the root p's chain reaches.
  passes   S(a, b) = the largest min(D2[p], D2[q]) over the 8-adjacent pixel pairs p in basin a, q in basin b (of one label).
  rounds   every basin starts as its own component; the representative of a component is its root of greatest key, its peak P the D2 there.  In one
           round every component X picks the pass to another component Y of greatest (S, -rep Y) and is absorbed into Y when key(rep X) <
           key(rep Y) and sqrt(P_X) - sqrt(S) <= min_depth; all absorptions are decided on the state at the round's start and applied together.
           Rounds repeat until none fires.
min_depth = h is in pixels: a neck is cut when the distance map falls by more than h from the lower of the two peaks to the pass.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from . import distance as D

MAX_DEPTH = 32767
ROUTES = ("auto", "lds", "global")


class SplitLabels(NamedTuple):
    labels: torch.Tensor      # int32 [H, W]
    parent: torch.Tensor      # int32 [K']
    peak_r2: torch.Tensor     # int32 [K']
    peak_xy: torch.Tensor     # int32 [K', 2] as (x, y)
    parts_of: torch.Tensor    # int32 [K]


def shallow(p: int, s: int, h: int) -> bool:
    """sqrt(p) - sqrt(s) <= h for integers 0 <= s <= p, taken exactly: with t = p - s - h^2 it is t <= 0 or t^2 <= 4 h^2 s (Python integers)."""
    p, s, h = int(p), int(s), int(h)
    t = p - s - h * h
    return t <= 0 or t * t <= 4 * h * h * s


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _shift(h: int, w: int, dy: int, dx: int):
    """(dst, src): the pixels whose neighbour at (dy, dx) lies in the frame, and those neighbours."""
    ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
    return (ys, xs), (slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx))


def _ascent_host(lab: np.ndarray, d2: np.ndarray) -> np.ndarray:
    """up int64 [H * W]"""
    h, w = lab.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    bd, bq = d2.astype(np.int64), idx.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy or dx) and h > abs(dy) and w > abs(dx):
                dst, src = _shift(h, w, dy, dx)
                same = (lab[dst] > 0) & (lab[src] == lab[dst])
                better = same & ((d2[src] > bd[dst]) | ((d2[src] == bd[dst]) & (idx[src] < bq[dst])))
                bd[dst] = np.where(better, d2[src], bd[dst])
                bq[dst] = np.where(better, idx[src], bq[dst])
    return bq.reshape(-1)


def _flatten_host(up: np.ndarray) -> np.ndarray:
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            return up
        up = nxt


def _passes_host(lab: np.ndarray, d2: np.ndarray, root: np.ndarray):
    """(a, b, S) int64 [m]: the pairs of basins a < b of one label that touch, and their passes."""
    h, w = lab.shape
    r2 = root.reshape(h, w)
    ks, ss = [], []
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        if h > abs(dy) and w > abs(dx):
            dst, src = _shift(h, w, dy, dx)
            m = (lab[dst] > 0) & (lab[src] == lab[dst]) & (r2[src] != r2[dst])
            ra, rb = r2[dst][m], r2[src][m]
            ks.append(np.minimum(ra, rb) * (h * w) + np.maximum(ra, rb))
            ss.append(np.minimum(d2[dst][m], d2[src][m]))
    key = np.concatenate(ks) if ks else np.zeros(0, np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    s = np.zeros(len(uniq), np.int64)
    if len(uniq):
        np.maximum.at(s, inv.reshape(-1), np.concatenate(ss).astype(np.int64))
    return uniq // (h * w), uniq % (h * w), s


def _round_host(ea: np.ndarray, eb: np.ndarray, es: np.ndarray, d2f: np.ndarray, up: np.ndarray, h: int):
    """One round on the flattened `up`: (X, Y) int64 [f] -- the representatives absorbed and what absorbs them."""
    none = np.zeros(0, np.int64)
    x, y = up[ea], up[eb]
    m = x != y
    if not m.any():
        return none, none
    u, v, s = np.concatenate([x[m], y[m]]), np.concatenate([y[m], x[m]]), np.concatenate([es[m], es[m]])
    word = (s.astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - v).astype(np.uint64)            # the greatest (S, -rep Y)
    reps, inv = np.unique(u, return_inverse=True)
    best = np.zeros(len(reps), np.uint64)
    np.maximum.at(best, inv.reshape(-1), word)
    bs = (best >> np.uint64(32)).astype(np.int64)
    by = 0xFFFFFFFF - (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    p, py = d2f[reps], d2f[by]
    lower = np.flatnonzero((p < py) | ((p == py) & (reps > by)))                                  # key(rep X) < key(rep Y)
    fired = np.array([i for i in lower if shallow(p[i], bs[i], h)], np.int64)
    return reps[fired], by[fired]


def _split_host(lab: np.ndarray, d2: np.ndarray, k: int, h: int, max_pairs: int, max_rounds: int, stats: Optional[dict]):
    hh, w = lab.shape
    n = hh * w
    labf, d2f = lab.reshape(-1).astype(np.int64), d2.reshape(-1).astype(np.int64)
    up = _flatten_host(_ascent_host(lab, d2.astype(np.int64)))
    ea, eb, es = _passes_host(lab, d2.astype(np.int64), up)
    if len(ea) > max_pairs:
        raise _lib.UllsamError(f"split_labels: more than max_pairs = {max_pairs} pairs of touching basins")
    basins = int(((up == np.arange(n)) & (labf > 0)).sum()) if stats is not None else 0
    rounds = 0
    for _ in range(max_rounds):
        x, y = _round_host(ea, eb, es, d2f, up, h)
        if not len(x):
            break
        up[x] = y
        up = _flatten_host(up)
        rounds += 1
    else:
        raise _lib.UllsamError(f"split_labels: the merging did not come to rest within max_rounds = {max_rounds} rounds")
    reps = np.flatnonzero((up == np.arange(n)) & (labf > 0))
    reps = reps[np.argsort(labf[reps], kind="stable")]                                            # (old label, index)
    newid = np.zeros(n, np.int64)
    newid[reps] = np.arange(1, len(reps) + 1)
    out = np.where(labf > 0, newid[up], 0).reshape(hh, w)
    parent = labf[reps]
    parts_of = np.bincount(parent - 1, minlength=k)[:k] if k else np.zeros(0, np.int64)
    if stats is not None:
        stats.update(basins=basins, pairs=len(ea), rounds=rounds, parts=len(reps))
    return out, parent, d2f[reps], np.stack([reps % w, reps // w], 1).reshape(-1, 2), parts_of


# ---- the public function ------------------------------------------------------------------------------------------------------------------------
def _int_in(v, name: str, lo: int, hi: int) -> int:
    v = D._integer(v, name, "split_labels")
    if not lo <= v <= hi:
        raise ValueError(f"split_labels: {name} = {v} must lie in {lo}..{hi}")
    return v


def split_labels(labels, min_depth=1, edge: bool = False, num: Optional[int] = None, max_pairs: int = 1 << 20, max_rounds: int = 256, device=None,
                 route: str = "auto", stats: Optional[dict] = None) -> SplitLabels:
    """Cut every instance of `labels` (int32 [H, W], 0 = background, ids 1..K, an instance need not be connected, 1 <= H, W <= 32767) at the necks of
    its distance map inner_distance(labels, edge) -- the module's text states the rule, DESIGN.md its facts.  min_depth = h, an integer in 0..32767,
    in pixels: two neighbouring peaks stay one part when the map falls by at most h from the lower peak to the pass between them.  h = 0 keeps
    every rise apart (plateaus still join); h = 32767 leaves exactly the 8-connected components of every instance.
    -> SplitLabels(labels int32 [H, W], parent int32 [K'], peak_r2 int32 [K'], peak_xy int32 [K', 2], parts_of int32 [K]): the parts are numbered
    1..K' by (old id, row-major index of the part's representative); the representative is the first pixel in row-major order among the part's
    deepest pixels, peak_r2 / peak_xy describe it.  An instance that is not cut keeps its pixels; its id may change, parent says how.
    K = num (default labels.max(): one more read-back on the device route); an id above K raises as a negative one does.
    max_pairs: the capacity of the table of touching basin pairs (more raise UllsamError); max_rounds: the merge rounds allowed (typically 1..4 are
    needed; one that has not come to rest raises UllsamError, nothing is truncated).  Bad arguments raise ValueError; a bad id raises ValueError
    on the host route and UllsamError on the device route (a status word; nothing is indexed with it, and the next call works).
    device None: where the labels are (numpy, CPU tensor: the numpy definition; a GPU tensor: csrc/split.hip); "cpu" / a GPU device: that route.
    route (device only): "auto", "lds", "global" -- where the ascent reads its 3 x 3 neighbourhood from; the outputs do not depend on it.
    stats: a dict that receives basins, pairs, rounds, parts (the device route counts the basins with one more read-back when it is given).
    The device route reads back one word per round and the status word."""
    D._frame(labels, "split_labels")
    h = _int_in(min_depth, "min_depth", 0, MAX_DEPTH)
    max_pairs = _int_in(max_pairs, "max_pairs", 1, 2 ** 30)
    max_rounds = _int_in(max_rounds, "max_rounds", 1, 2 ** 20)
    if route not in ROUTES:
        raise ValueError(f"split_labels: route must be one of {ROUTES}, got {route!r}")
    dev = D._route(labels, device)
    if dev.type != "cuda":
        lab = D._host_labels(labels, "split_labels")
        k = D._num(lab, num, "split_labels")
        if lab.size and int(lab.max()) > k:
            raise ValueError(f"split_labels: the label image holds an id outside 0..{k}")
        res = _split_host(lab, D._inner_host(lab, bool(edge)), k, h, max_pairs, max_rounds, stats)
        return SplitLabels(*(D._t(np.asarray(a)) for a in res))
    from .. import ops
    lab = D._device_labels(labels, dev)
    k = D._num(lab, num, "split_labels")
    flags = torch.zeros((ops.SPLIT_FLAGS,), dtype=torch.int32, device=dev)
    g, _, _ = ops.distance_columns(lab, False, edge, num=k, flags=flags[:ops.DISTANCE_FLAGS])
    d2, _ = ops.distance_rows(lab, g, None, "inner", edge, num=k, flags=flags[:ops.DISTANCE_FLAGS])
    up, _ = ops.split_ascent(lab, d2, k, route, flags)
    ops.split_flatten(up, flags=flags)
    basins = 0
    if stats is not None:
        basins = int(ops.split_collect(lab, up, None, k)[4].cpu())
    keys, vals, _ = ops.split_passes(lab, d2, up, max_pairs, k, flags)
    best = torch.zeros((lab.numel(),), dtype=torch.int64, device=dev)
    changed = torch.zeros((max_rounds,), dtype=torch.int32, device=dev)
    rounds = 0
    for r in range(max_rounds):
        ops.split_round(keys, vals, lab, d2, up, h, best, changed[r:r + 1], k, flags)
        if not int(changed[r].cpu()):                     # the one read-back of the round
            break
        ops.split_flatten(up, flags=flags)
        rounds += 1
    else:
        raise _lib.UllsamError(f"split_labels: the merging did not come to rest within max_rounds = {max_rounds} rounds")
    ops.split_collect(lab, up, None, k, flags)
    fl = flags.cpu().tolist()                             # the status word, and K'
    if fl[0]:
        raise _lib.UllsamError(f"split_labels: the label image holds an id outside 0..{k}")
    if fl[1] or fl[2] > max_pairs:
        raise _lib.UllsamError(f"split_labels: more than max_pairs = {max_pairs} pairs of touching basins")
    if fl[3]:
        raise _lib.UllsamError("split_labels: a chain of the ascent is longer than the frame has pixels")
    lst, _ = ops.split_collect(lab, up, fl[4], k, flags)
    out, parent, peak_r2, peak_xy, parts_of, _ = ops.split_relabel(torch.sort(lst).values, lab, d2, up, k, flags)
    if stats is not None:
        stats.update(basins=basins, pairs=fl[2], rounds=rounds, parts=fl[4])
    return SplitLabels(out, parent, peak_r2, peak_xy, parts_of)
