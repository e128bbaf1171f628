"""Splitting the touching objects of an instance label VOLUME with anisotropic voxels: utils.split's flood-free watershed with a third axis, on
every object's own depth map utils.distance3d.inner_distance3d.  This module is the definition (numpy, integers only) and the driver of the device
route (csrc/split3d.hip for the stages that know the volume's shape, csrc/split.hip's flat entry points for the rest); the two are equal bit for bit
(tests/test_split3d_*.py).  DESIGN.md "7b, continued (3-D splitting)" states the definition and its facts.

    volume = link_label_stack(planes, counts, mode="all", device="cuda")[0]   # nuclei stacked along z come out fused
    parts = split_labels3d(volume, min_depth=2, spacing=(5, 2, 2))            # planes 2.5 times as far apart as pixels; 2 = one pixel of xy
    parts.labels      # int32 [Z, H, W]: the parts, numbered 1..K' by (old id, raster index of the part's representative)
    parts.parent      # int32 [K']: the old id of every part
    parts.peak_r2     # int32 [K']: the largest inner_distance3d over the part -- the squared radius of its largest inscribed ball, in spacing units
    parts.peak_xyz    # int32 [K', 3]: (x, y, z) of the first voxel in (z, y, x) raster order that attains it
    parts.parts_of    # int32 [K]: how many parts every old id was cut into (0: the id is absent)

The definition is utils.split's with three changes: D2 = inner_distance3d(volume, spacing, edge) (edge a bool or a triple (ez, ey, ex)); p = the
(z, y, x) raster index (z * H + y) * W + x; "neighbours" are the 26 voxels of the 3 x 3 x 3 block around a voxel, and the passes run over its 13
forward offsets, so every 26-adjacent pair is counted once.  With key(p) = (D2[p], -p), a strict total order:
  ascent   up(p) = the voxel of greatest key among p and its 26 neighbours with p's label; a root has up(p) = p; basin(p) = the root p's chain reaches.
  passes   S(a, b) = the largest min(D2[p], D2[q]) over the 26-adjacent voxel pairs p in basin a, q in basin b (of one label).
  rounds   every basin starts as its own component; the representative of a component is its root of greatest key, its peak P the D2 there.  In one
           round every component X picks the pass to another component Y of greatest (S, -rep Y) and is absorbed into Y when key(rep X) <
           key(rep Y) and sqrt(P_X) - sqrt(S) <= min_depth (exactly, in 64-bit integers); all absorptions are decided on the state at the round's
           start and applied together.  Rounds repeat until none fires.
  numbers  the parts are numbered by their sorted words label << 32 | p of the representatives.
min_depth = h is in spacing units, like sqrt(D2): with spacing (5, 2, 2) one pixel of xy is h = 2 and one plane of z is h = 5.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from . import distance as D
from . import distance3d as D3
from .split import MAX_DEPTH, ROUTES, _flatten_host, _round_host

MAX_VOXELS = 32767 * 32767   # the bound of the flat split entry points; it keeps every neighbour index p +- (H W + W + 1) inside int32


class SplitLabels3d(NamedTuple):
    labels: torch.Tensor      # int32 [Z, H, W]
    parent: torch.Tensor      # int32 [K']
    peak_r2: torch.Tensor     # int32 [K']
    peak_xyz: torch.Tensor    # int32 [K', 3] as (x, y, z)
    parts_of: torch.Tensor    # int32 [K]


OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
FORWARD = [o for o in OFFSETS if o > (0, 0, 0)]           # the 13 offsets whose neighbour has the greater raster index: every pair once


# ---- the host form ------------------------------------------------------------------------------------------------------------------------------
def _shift(shape, off):
    """(dst, src): the voxels whose neighbour at `off` lies in the volume, and those neighbours; None where an axis is too short."""
    if any(n <= abs(d) for n, d in zip(shape, off)):
        return None
    dst = tuple(slice(max(0, -d), n - max(0, d)) for n, d in zip(shape, off))
    return dst, tuple(slice(s.start + d, s.stop + d) for s, d in zip(dst, off))


def _ascent_host(lab: np.ndarray, d2: np.ndarray) -> np.ndarray:
    """up int64 [Z * H * W]"""
    idx = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    bd, bq = d2.astype(np.int64), idx.copy()
    for off in OFFSETS:
        sh = _shift(lab.shape, off)
        if sh is not None:
            dst, src = sh
            same = (lab[dst] > 0) & (lab[src] == lab[dst])
            better = same & ((d2[src] > bd[dst]) | ((d2[src] == bd[dst]) & (idx[src] < bq[dst])))
            bd[dst] = np.where(better, d2[src], bd[dst])
            bq[dst] = np.where(better, idx[src], bq[dst])
    return bq.reshape(-1)


def _passes_host(lab: np.ndarray, d2: np.ndarray, root: np.ndarray):
    """(a, b, S) int64 [m]: the pairs of basins a < b of one label that touch, and their passes."""
    n = lab.size
    r3 = root.reshape(lab.shape)
    ks, ss = [], []
    for off in FORWARD:
        sh = _shift(lab.shape, off)
        if sh is not None:
            dst, src = sh
            m = (lab[dst] > 0) & (lab[src] == lab[dst]) & (r3[src] != r3[dst])
            ra, rb = r3[dst][m], r3[src][m]
            ks.append(np.minimum(ra, rb) * n + np.maximum(ra, rb))
            ss.append(np.minimum(d2[dst][m], d2[src][m]))
    key = np.concatenate(ks) if ks else np.zeros(0, np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    s = np.zeros(len(uniq), np.int64)
    if len(uniq):
        np.maximum.at(s, inv.reshape(-1), np.concatenate(ss).astype(np.int64))
    return uniq // n, uniq % n, s


def _split_host(lab: np.ndarray, d2: np.ndarray, k: int, h: int, max_pairs: int, max_rounds: int, stats: Optional[dict]):
    _, hh, w = lab.shape
    n = lab.size
    labf, d2f = lab.reshape(-1).astype(np.int64), d2.reshape(-1).astype(np.int64)
    up = _flatten_host(_ascent_host(lab, d2.astype(np.int64)))
    ea, eb, es = _passes_host(lab, d2.astype(np.int64), up)
    if len(ea) > max_pairs:
        raise _lib.UllsamError(f"split_labels3d: more than max_pairs = {max_pairs} pairs of touching basins")
    basins = int(((up == np.arange(n)) & (labf > 0)).sum()) if stats is not None else 0
    rounds = 0
    for _ in range(max_rounds):
        x, y = _round_host(ea, eb, es, d2f, up, h)          # (utils.split's round: it never looks at the shape)
        if not len(x):
            break
        up[x] = y
        up = _flatten_host(up)
        rounds += 1
    else:
        raise _lib.UllsamError(f"split_labels3d: the merging did not come to rest within max_rounds = {max_rounds} rounds")
    reps = np.flatnonzero((up == np.arange(n)) & (labf > 0))
    reps = reps[np.argsort(labf[reps], kind="stable")]                                            # (old label, index)
    newid = np.zeros(n, np.int64)
    newid[reps] = np.arange(1, len(reps) + 1)
    out = np.where(labf > 0, newid[up], 0).reshape(lab.shape)
    parent = labf[reps]
    parts_of = np.bincount(parent - 1, minlength=k)[:k] if k else np.zeros(0, np.int64)
    if stats is not None:
        stats.update(basins=basins, pairs=len(ea), rounds=rounds, parts=len(reps))
    return out, parent, d2f[reps], np.stack([reps % w, (reps // w) % hh, reps // (w * hh)], 1).reshape(-1, 3), parts_of


# ---- the public function ------------------------------------------------------------------------------------------------------------------------
def _int_in(v, name: str, lo: int, hi: int) -> int:
    v = D._integer(v, name, "split_labels3d")
    if not lo <= v <= hi:
        raise ValueError(f"split_labels3d: {name} = {v} must lie in {lo}..{hi}")
    return v


def split_labels3d(volume, min_depth=1, spacing=(1, 1, 1), edge=False, num: Optional[int] = None, max_pairs: int = 1 << 20, max_rounds: int = 256,
                   device=None, route: str = "auto", stats: Optional[dict] = None) -> SplitLabels3d:
    """Cut every object of `volume` (int32 [Z, H, W], 0 = background, ids 1..K, an object need not be connected) at the necks of its distance map
    inner_distance3d(volume, spacing, edge) -- the module's text states the rule, DESIGN.md its facts.  spacing = (sz, sy, sx), positive integers;
    edge a bool or a triple (ez, ey, ex).  min_depth = h, an integer in 0..32767, is in SPACING UNITS, like sqrt(D2): two neighbouring peaks stay
    one part when the map's square root falls by at most h from the lower peak to the pass between them; with spacing (5, 2, 2) one pixel of xy is
    h = 2.  h = 0 keeps every rise apart (plateaus still join); h = 32767 leaves the 26-connected components of every object wherever no part's
    sqrt(peak_r2) exceeds 32767 + min(spacing) (DESIGN.md has the exact condition).
    -> SplitLabels3d(labels int32 [Z, H, W], parent int32 [K'], peak_r2 int32 [K'], peak_xyz int32 [K', 3], parts_of int32 [K]): the parts are
    numbered 1..K' by (old id, raster index of the part's representative); the representative is the first voxel in (z, y, x) raster order among
    the part's deepest voxels, peak_r2 / peak_xyz describe it.  An object that is not cut keeps its voxels; its id may change, parent says how.
    Limits (ValueError, stating the number, before any voxel is read -- a stub with a .shape is enough): inner_distance3d's on sides, spacings and
    B; min_depth in 0..32767; Z * H * W <= 32767^2 = 1 073 676 289.
    K = num (default volume.max(): one more read-back on the device route); an id above K raises as a negative one does.
    max_pairs: the capacity of the table of touching basin pairs (more raise UllsamError); max_rounds: the merge rounds allowed (one that has not
    come to rest raises UllsamError, nothing is truncated).  A bad id raises ValueError on the host route and UllsamError on the device route (a
    status word; nothing is indexed with it, and the next call works).
    device None: where the volume is (numpy, CPU tensor: the numpy definition; a GPU tensor: the kernels, used where it is -- the volume of
    link_label_stack goes in without a host trip); "cpu" / a GPU device: that route.
    route (device only): "auto", "lds", "global" -- where the ascent reads its 3 x 3 x 3 neighbourhood from; the outputs do not depend on it.
    stats: a dict that receives basins, pairs, rounds, parts (the device route counts the basins with one more read-back when it is given).
    The device route reads back one word per round and the status word.  Its maps: the volume, g (2 bytes a voxel) and two int32 maps of the
    distance passes, then D2, up, best (8 bytes), and at the end newid and the output."""
    shape, s, e = D3._metric(volume, spacing, edge, "split_labels3d")
    if shape[0] * shape[1] * shape[2] > MAX_VOXELS:
        raise ValueError(f"split_labels3d: a volume of {shape[0]} x {shape[1]} x {shape[2]} = {shape[0] * shape[1] * shape[2]} voxels "
                         f"(at most 32767^2 = {MAX_VOXELS})")
    h = _int_in(min_depth, "min_depth", 0, MAX_DEPTH)
    max_pairs = _int_in(max_pairs, "max_pairs", 1, 2 ** 30)
    max_rounds = _int_in(max_rounds, "max_rounds", 1, 2 ** 20)
    if route not in ROUTES:
        raise ValueError(f"split_labels3d: route must be one of {ROUTES}, got {route!r}")
    dev = D._route(volume, device)
    if dev.type != "cuda":
        vol = D._host_labels(volume, "split_labels3d")
        k = D._num(vol, num, "split_labels3d")
        if vol.size and int(vol.max()) > k:
            raise ValueError(f"split_labels3d: the label volume holds an id outside 0..{k}")
        res = _split_host(vol, D3._inner_host(vol, s, e), k, h, max_pairs, max_rounds, stats)
        return SplitLabels3d(*(D._t(np.asarray(a)) for a in res))
    from .. import ops
    vol = D._device_labels(volume, dev)
    k = D._num(vol, num, "split_labels3d")
    flags = torch.zeros((ops.SPLIT_FLAGS,), dtype=torch.int32, device=dev)
    g, _, _ = ops.distance3d_z(vol, False, e[0], num=k, flags=flags[:ops.DISTANCE_FLAGS])
    hy, _ = ops.distance3d_y(vol, g, None, s, e)
    d2, _ = ops.distance3d_x(vol, hy, None, "inner", s, e, num=k, flags=flags[:ops.DISTANCE_FLAGS])
    del g, hy
    up, _ = ops.split3d_ascent(vol, d2, k, route, flags)
    ops.split_flatten(up, flags=flags)
    basins = 0
    if stats is not None:
        basins = int(ops.split_collect(vol, up, None, k)[4].cpu())
    keys, vals, _ = ops.split3d_passes(vol, d2, up, max_pairs, k, flags)
    best = torch.zeros((vol.numel(),), dtype=torch.int64, device=dev)
    changed = torch.zeros((max_rounds,), dtype=torch.int32, device=dev)
    rounds = 0
    for r in range(max_rounds):
        ops.split_round(keys, vals, vol, d2, up, h, best, changed[r:r + 1], k, flags)
        if not int(changed[r].cpu()):                     # the one read-back of the round
            break
        ops.split_flatten(up, flags=flags)
        rounds += 1
    else:
        raise _lib.UllsamError(f"split_labels3d: the merging did not come to rest within max_rounds = {max_rounds} rounds")
    del best
    ops.split_collect(vol, up, None, k, flags)
    fl = flags.cpu().tolist()                             # the status word, and K'
    if fl[0]:
        raise _lib.UllsamError(f"split_labels3d: the label volume holds an id outside 0..{k}")
    if fl[1] or fl[2] > max_pairs:
        raise _lib.UllsamError(f"split_labels3d: more than max_pairs = {max_pairs} pairs of touching basins")
    if fl[3]:
        raise _lib.UllsamError("split_labels3d: a chain of the ascent is longer than the volume has voxels")
    lst, _ = ops.split_collect(vol, up, fl[4], k, flags)
    out, parent, peak_r2, peak_xyz, parts_of, _ = ops.split3d_relabel(torch.sort(lst).values, vol, d2, up, k, flags)
    if stats is not None:
        stats.update(basins=basins, pairs=fl[2], rounds=rounds, parts=fl[4])
    return SplitLabels3d(out, parent, peak_r2, peak_xyz, parts_of)
