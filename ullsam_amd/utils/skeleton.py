"""Skeletons of an instance label image: every instance thinned to its centreline by Guo and Hall's two-sub-iteration parallel rule, all instances at
once, and the end points, junctions, links and local widths of the result.  This module is the definition (numpy, integers only) and the driver of
the device route (csrc/skeleton.hip); the two are equal bit for bit (tests/test_skeleton_*.py).  DESIGN.md "7b, continued (skeletons)" states the
rule and its facts.

    sk = skeletonize_labels(labels, device="cuda")
    sk.labels             # int32 [H, W]: the input with the deleted pixels set to 0
    sk.subiterations      # one plus the index of the last sub-iteration that deleted a pixel (0: nothing was deleted)
    table = measure_skeletons(sk.labels, d2=inner_distance(labels))     # SkeletonTable, one row per id
    nodes = node_image(sk.labels)                                       # uint8 [H, W]: 1 end point, 2 ordinary, 3 junction, 4 isolated
    props = derive_skeletons(table, pixel_size=0.325)                   # float64: length, widths

The rule in short.  A neighbour of pixel p is ON when it lies in the frame, has not been deleted and carries p's label: the background, the frame's
outside and every other instance are off, so two cells that share a border thin as if each were alone.  The 8-bit code of p has bit i for the
neighbour N, NE, E, SE, S, SW, W, NW (y grows downwards), i = 0..7 -- p2..p9 of the paper.  With
  C  = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2)),
  N  = min((p9|p2) + (p3|p4) + (p5|p6) + (p7|p8), (p2|p3) + (p4|p5) + (p6|p7) + (p8|p9)),
  m  = (p2|p3|!p5) & p4 in sub-iterations 0, 2, 4, ... and (p6|p7|!p9) & p8 in sub-iterations 1, 3, 5, ...
p is deleted iff C == 1, 2 <= N <= 3 and m == 0: two tables of 256 entries, 37 deletable codes each.  A sub-iteration reads the state at its start
and applies all its deletions together; sub-iterations alternate from index 0 until two consecutive ones delete nothing.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from . import distance as D

ROUTES = ("auto", "global", "lds")
AUTO_ROUTE = "lds"        # the winner of the A/B of tools/skeleton_bench.py (profiles/r27_skeleton.txt)
# A full n x n block needs n - 1 sub-iterations (every sub-iteration takes one layer off two of its four sides; tests/test_skeleton_cpu.py checks
# n = 2..33), so the thickest instance a frame of 32767 a side can hold, the full frame, needs 32766.  The default allows twice that and two more:
# no instance of such a frame comes near it, and a call that would exceed it raises, nothing is truncated.
MAX_SUBITERATIONS = 2 * 32767 + 2
INT_MAX = 2 ** 31 - 1
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # (dy, dx) of bit i: N, NE, E, SE, S, SW, W, NW
COUNT_FIELDS = ("pixels", "end_points", "junctions", "isolated", "links_orth", "links_diag", "degree_sum")


class Skeleton(NamedTuple):
    labels: torch.Tensor      # int32 [H, W]
    subiterations: int


class SkeletonTable(NamedTuple):
    """Row k - 1 belongs to id k.  pixels; end_points (degree 1), junctions (degree >= 3), isolated (degree 0); links_orth, links_diag (every link
    once); degree_sum: int64 [K].  With d2: d2_sum int64 [K], d2_min / d2_max int32 [K] -- (2^31 - 1, -1) for an absent id; None without."""
    pixels: torch.Tensor
    end_points: torch.Tensor
    junctions: torch.Tensor
    isolated: torch.Tensor
    links_orth: torch.Tensor
    links_diag: torch.Tensor
    degree_sum: torch.Tensor
    d2_sum: Optional[torch.Tensor] = None
    d2_min: Optional[torch.Tensor] = None
    d2_max: Optional[torch.Tensor] = None


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------
def _table(parity: int) -> np.ndarray:
    """bool [256]: the deletable codes of the sub-iterations of that parity."""
    code = np.arange(256)
    p2, p3, p4, p5, p6, p7, p8, p9 = (((code >> i) & 1).astype(bool) for i in range(8))
    i = lambda b: b.astype(np.int64)
    c = i(~p2 & (p3 | p4)) + i(~p4 & (p5 | p6)) + i(~p6 & (p7 | p8)) + i(~p8 & (p9 | p2))
    n = np.minimum(i(p9 | p2) + i(p3 | p4) + i(p5 | p6) + i(p7 | p8), i(p2 | p3) + i(p4 | p5) + i(p6 | p7) + i(p8 | p9))
    m = ((p2 | p3 | ~p5) & p4) if parity == 0 else ((p6 | p7 | ~p9) & p8)
    return (c == 1) & (n >= 2) & (n <= 3) & ~m


TABLES = (_table(0), _table(1))


def table_words(parity: int):
    """The table as eight 32-bit words: bit (code & 31) of word (code >> 5) -- what the kernels hold."""
    return [int(sum(1 << b for b in range(32) if TABLES[parity][32 * j + b])) for j in range(8)]


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _same(img: np.ndarray):
    """[8] bool [H, W]: neighbour i of the pixel is on (in the frame, the pixel's own positive label)."""
    h, w = img.shape
    pad = np.zeros((h + 2, w + 2), img.dtype)
    pad[1:-1, 1:-1] = img
    on = img > 0
    return [on & (pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] == img) for dy, dx in OFFSETS]


def _subiteration_host(img: np.ndarray, index: int):
    """-> (the image after sub-iteration `index`, the number of pixels it deleted)"""
    code = np.zeros(img.shape, np.int64)
    for i, s in enumerate(_same(img)):
        code |= s.astype(np.int64) << i
    gone = (img > 0) & TABLES[index & 1][code]
    n = int(gone.sum())
    return (np.where(gone, 0, img) if n else img), n


def _thin_host(lab: np.ndarray, max_subiterations: int):
    img, last, i = lab, 0, 0
    while i < last + 2:
        img, n = _subiteration_host(img, i)
        if n:
            if i >= max_subiterations:
                raise _lib.UllsamError(f"skeletonize_labels: the thinning did not come to rest within max_subiterations = {max_subiterations}")
            last = i + 1
        i += 1
    return img, last


def _links_host(img: np.ndarray):
    """[8] bool [H, W]: the pixel is linked to its neighbour i."""
    s = _same(img)
    out = list(s)
    for i in (1, 3, 5, 7):                                 # a diagonal link: neither pixel 4-adjacent to both carries the label
        out[i] = s[i] & ~s[i - 1] & ~s[(i + 1) % 8]
    return out


def _nodes_of(on: np.ndarray, deg: np.ndarray) -> np.ndarray:
    return np.where(on, np.where(deg == 0, 4, np.where(deg == 1, 1, np.where(deg == 2, 2, 3))), 0).astype(np.uint8)


def _measure_host(img: np.ndarray, k: int, d2: Optional[np.ndarray]) -> Dict[str, np.ndarray]:
    links = _links_host(img)
    deg = sum(l.astype(np.int64) for l in links)
    ys, xs = np.nonzero(img)
    idx = img[ys, xs].astype(np.int64) - 1
    cnt = lambda v: np.bincount(idx, weights=v[ys, xs].astype(np.int64), minlength=k).astype(np.int64)      # (sums below 2^53: exact in float64)
    out = {"pixels": np.bincount(idx, minlength=k).astype(np.int64), "end_points": cnt(deg == 1), "junctions": cnt(deg >= 3),
           "isolated": cnt(deg == 0), "links_orth": cnt(links[2].astype(np.int64) + links[4]), "links_diag": cnt(links[3].astype(np.int64) + links[5]),
           "degree_sum": cnt(deg)}
    if d2 is not None:
        v = d2[ys, xs].astype(np.int64)
        lo = np.bincount(idx, weights=v & 0xffff, minlength=k).astype(np.int64)
        hi = np.bincount(idx, weights=v >> 16, minlength=k).astype(np.int64)
        mn, mx = np.full((k,), INT_MAX, np.int64), np.full((k,), -1, np.int64)
        np.minimum.at(mn, idx, v)
        np.maximum.at(mx, idx, v)
        out.update(d2_sum=lo + (hi << 16), d2_min=mn.astype(np.int32), d2_max=mx.astype(np.int32))
    return out


# ---- the public functions -----------------------------------------------------------------------------------------------------------------------
def _int_in(v, name: str, lo: int, hi: int, what: str) -> int:
    v = D._integer(v, name, what)
    if not lo <= v <= hi:
        raise ValueError(f"{what}: {name} = {v} must lie in {lo}..{hi}")
    return v


def skeletonize_labels(labels, device=None, route: str = "auto", max_subiterations: int = MAX_SUBITERATIONS, block: Optional[int] = None) -> Skeleton:
    """Thin every instance of `labels` (int32 [H, W], 0 = background, any positive id an instance, 1 <= H, W <= 32767) by the rule of the module's
    text, all instances at once and each as if it were alone.  -> Skeleton(labels int32 [H, W]: the input with the deleted pixels set to 0,
    subiterations: one plus the index of the last sub-iteration that deleted a pixel, 0 if none did).  The skeleton keeps, per label, the
    8-connected components and the holes of the input; residual 2 x 2 blocks can survive, one-pixel thinness is not promised.
    max_subiterations (0..2^30): a thinning that needs more raises UllsamError, nothing is truncated; the default is one that an instance of a
    32767-wide frame cannot reach (see MAX_SUBITERATIONS).  Bad arguments raise ValueError before a pixel is read; a negative id raises ValueError
    on the host route and UllsamError on the device route (a status word; nothing is indexed with it).
    device None: where the labels are (numpy, CPU tensor: the numpy definition; a GPU tensor: csrc/skeleton.hip); "cpu" / a GPU device: that route.
    route (device only): "global" -- one sub-iteration per launch on the whole frame; "lds" -- ops.SKEL_TILE_STEPS sub-iterations per launch on
    tiles staged in LDS with a halo that deep; "auto" -- the faster one (tools/skeleton_bench.py).  block (device only; None = ops.SKEL_BLOCK): the
    sub-iterations launched between two read-backs of the counters, a multiple of ops.SKEL_TILE_STEPS.  The outputs depend on neither."""
    what = "skeletonize_labels"
    D._frame(labels, what)
    limit = _int_in(max_subiterations, "max_subiterations", 0, 2 ** 30, what)
    if route not in ROUTES:
        raise ValueError(f"{what}: route must be one of {ROUTES}, got {route!r}")
    dev = D._route(labels, device)
    if dev.type != "cuda":
        if block is not None:
            _int_in(block, "block", 1, 2 ** 16, what)
        img, n = _thin_host(D._host_labels(labels, what), limit)
        return Skeleton(D._t(img), n)
    from .. import ops
    block = ops.SKEL_BLOCK if block is None else _int_in(block, "block", 1, 2 ** 16, what)
    if block % ops.SKEL_TILE_STEPS:
        raise ValueError(f"{what}: block = {block} must be a multiple of {ops.SKEL_TILE_STEPS}")
    route = AUTO_ROUTE if route == "auto" else route
    cur = D._device_labels(labels, dev)
    bufs = [torch.empty_like(cur), torch.empty_like(cur)]
    state = torch.zeros((ops.SKEL_FLAGS + block,), dtype=torch.int32, device=dev)       # the status words, then one counter per sub-iteration
    flags, counts = state[:ops.SKEL_FLAGS], state[ops.SKEL_FLAGS:]
    done = last = launches = 0
    while done < last + 2:
        if done:
            counts.zero_()
        for j in range(0, block, ops.SKEL_TILE_STEPS if route == "lds" else 1):
            dst = bufs[launches & 1]
            if route == "lds":
                ops.skel_tile(cur, dst, done + j, limit, counts[j:j + ops.SKEL_TILE_STEPS], flags)
            else:
                ops.skel_step(cur, dst, done + j, limit, counts[j:j + 1], flags)
            cur, launches = dst, launches + 1
        st = state.cpu().tolist()                           # the one read-back of the block
        if st[0]:
            raise _lib.UllsamError(f"{what}: the label image holds a negative id")
        if st[1]:
            raise _lib.UllsamError(f"{what}: the thinning did not come to rest within max_subiterations = {limit}")
        for j, c in enumerate(st[ops.SKEL_FLAGS:]):
            if c:
                last = done + j + 1
        done += block
    return Skeleton(cur, last)


def _skeleton_args(skeleton_labels, num_ids, d2, what: str):
    h, w = D._frame(skeleton_labels, what)
    if d2 is not None:
        if tuple(getattr(d2, "shape", ())) != (h, w) or str(d2.dtype).replace("torch.", "") != "int32":
            raise ValueError(f"{what}: d2 must be int32 [{h}, {w}] (inner_distance of the label image), got {getattr(d2, 'dtype', None)} {tuple(getattr(d2, 'shape', ()))}")
    return None if num_ids is None else D._num(None, num_ids, what)


def measure_skeletons(skeleton_labels, num_ids: Optional[int] = None, d2=None, device=None) -> SkeletonTable:
    """The SkeletonTable of a skeleton image (int32 [H, W], what skeletonize_labels returns; any label image is taken as it is).  Two pixels of one
    label are LINKED when they are 4-adjacent, or diagonal with neither of the two pixels 4-adjacent to both carrying that label (an L-corner is no
    triangle); the degree of a pixel is its number of links.  Per id: pixels, end_points (degree 1), junctions (degree >= 3), isolated (degree 0),
    links_orth, links_diag (every link once), degree_sum (= 2 (links_orth + links_diag)); with d2 (int32 [H, W], inner_distance of the ORIGINAL
    label image: the squared local half-width) also d2_sum, d2_min, d2_max over the skeleton's pixels.  num_ids = K (default: the largest id, one
    read-back on the device route; 0..2^31 - 2); an id above K raises ValueError on the host route and UllsamError on the device route, as a
    negative one does.  device as in skeletonize_labels; on the device route d2 is taken where it lies and the tables stay on the device: one
    kernel over row tiles sends every skeleton pixel's contributions straight to the global tables with integer atomics (skeletons are sparse;
    no LDS table in front)."""
    what = "measure_skeletons"
    k = _skeleton_args(skeleton_labels, num_ids, d2, what)
    dev = D._route(skeleton_labels, device)
    if dev.type != "cuda":
        img = D._host_labels(skeleton_labels, what)
        k = D._num(img, None, what) if k is None else k
        if img.size and int(img.max()) > k:
            raise ValueError(f"{what}: the label image holds an id outside 0..{k}")
        dd = None if d2 is None else (d2.detach().cpu().numpy() if isinstance(d2, torch.Tensor) else np.asarray(d2))
        return SkeletonTable(**{n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in _measure_host(img, k, dd).items()})
    from .. import ops
    img = D._device_labels(skeleton_labels, dev)
    k = D._num(img, None, what) if k is None else k
    dd = None if d2 is None else torch.as_tensor(d2).to(device=dev, dtype=torch.int32).contiguous()
    t, _, flags = ops.skel_measure(img, k, dd, nodes=False)
    if int(flags.cpu()[0]):
        raise _lib.UllsamError(f"{what}: the label image holds an id outside 0..{k}")
    return SkeletonTable(**t)


def node_image(skeleton_labels, device=None) -> torch.Tensor:
    """uint8 [H, W]: 0 off, 1 an end point (degree 1), 2 an ordinary pixel (degree 2), 3 a junction (degree >= 3), 4 an isolated pixel (degree 0), by
    the links of measure_skeletons.  device as there."""
    what = "node_image"
    _skeleton_args(skeleton_labels, None, None, what)
    dev = D._route(skeleton_labels, device)
    if dev.type != "cuda":
        img = D._host_labels(skeleton_labels, what)
        return torch.from_numpy(_nodes_of(img > 0, sum(l.astype(np.int64) for l in _links_host(img))))
    from .. import ops
    img = D._device_labels(skeleton_labels, dev)
    _, nodes, flags = ops.skel_measure(img, None, None, nodes=True)
    if int(flags.cpu()[0]):
        raise _lib.UllsamError(f"{what}: the label image holds a negative id")
    return nodes


def derive_skeletons(table: SkeletonTable, pixel_size: float = 1.0) -> Dict[str, np.ndarray]:
    """float64 [K] on the host: length = (links_orth + sqrt(2) links_diag) pixel_size, and with d2 in the table mean_width, min_width, max_width =
    2 sqrt(d2) pixel_size of d2_sum / pixels (the root of the mean squared half-width), d2_min, d2_max.  NaN for an absent id.  Equality with
    another library's skeleton length is not claimed."""
    ps = float(pixel_size)
    host = lambda t: t.detach().cpu().numpy().astype(np.int64)
    px, lo, ld = host(table.pixels), host(table.links_orth), host(table.links_diag)
    there = px > 0
    nan = np.full(px.shape, np.nan, np.float64)
    out = {"length": np.where(there, (lo + math.sqrt(2.0) * ld) * ps, nan)}
    if table.d2_sum is not None:
        s, mn, mx = host(table.d2_sum), host(table.d2_min), host(table.d2_max)
        safe = np.maximum(px, 1)
        out["mean_width"] = np.where(there, 2.0 * np.sqrt(s / safe) * ps, nan)
        out["min_width"] = np.where(there, 2.0 * np.sqrt(np.where(there, mn, 0)) * ps, nan)
        out["max_width"] = np.where(there, 2.0 * np.sqrt(np.where(there, mx, 0)) * ps, nan)
    return out
