"""Point prompts, boxes and per-instance masks from one instance label image: what the reference's dataset derives per sample with four scipy
calls per instance (train_joint_v2.py:313-468) and hands to the model as `points`, `point_labels` and `masks`.

    ps = prompts_from_labels(labels)                       # numpy labels: the host route; a CUDA tensor or device=...: the kernels
    train_step_loss(model, pixel_values, input_ids, attention_mask, (ps.coords, ps.point_labels), ps.masks)

Definitions (DESIGN.md "7b, continued (prompts)"; all sets in row-major order, the order of np.where):
  M_i      = {p : labels[p] = i}, ids 1..65535, 0 = background.
  d1[p]    = city-block distance from p to the nearest pixel whose label differs from labels[p]; the outside of the frame differs.
  inner_i  = {p in M_i : d1[p] > inner_radius}            = ndimage.binary_erosion(M_i, iterations=inner_radius)            (:342)
  ring_i   = {p not in M_i : lo^2 <= D2_i[p] <= hi^2}, D2_i = squared Euclidean distance to the nearest pixel of M_i
                                                           = lo <= distance_transform_edt(~boundary) <= hi outside M_i      (:423-435)
  positives: num_pos distinct draws from inner_i; element j mod |inner_i| when 0 < |inner_i| < num_pos; the centroid (sum x // area,
             sum y // area) when inner_i is empty                                                                           (:361-377)
  negatives: num_neg distinct draws from ring_i; with fewer than num_neg ring pixels, from the pixels farther than inner_radius (city-block) from
             M_i (= outside binary_dilation(M_i, iterations=inner_radius)); with fewer than num_neg of those, from the pixels outside M_i (element
             j mod count when even those are fewer); no pixel outside M_i -- the reference loops forever there -- is an error        (:439-460)
  draw rule: the t-th of k distinct ranks out of m candidates is r = (w * (m - t)) >> 32 with w = word 0 of Philox4x32-10, key (seed & 0xffffffff,
             seed >> 32), counter (instance id, t + 16 * kind, 0, 0), kind 0 positive / 1 ring / 2, 3 the two fallbacks; r is the rank among the
             candidates not yet picked: walking the earlier picks in increasing order, r grows by one for each that is <= r.  (Replaces
             np.random.choice(.., replace=False): a draw depends on the seed, the instance id and the candidate set, nothing else.)
  choice:    the present ids in increasing order; more than max_instances of them: max_instances by the same rule with counter (0, t, 1, 0), kept in
             pick order.  Explicit `ids` override the choice; an id without pixels is an error.
  empty image (no id present, ids=None): the reference's default instance (_create_default_points, :584-602): id 0, a zero mask, num_pos times the
             centre (W // 2, H // 2), then the corners (10, 10), (W - 10, 10), (10, H - 10), (W - 10, H - 10) in turn (clipped to the frame).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .. import sampling

MAX_ID = 65535
MAX_POINTS = 16
MAX_RADIUS = 64                       # device route: inner_radius and ring[1] (the halo a tile of csrc/prompts.hip keeps in the LDS)
MAX_SCRATCH_BYTES = 1 << 30           # device route: the bit rows and row counts of all slots (1024^2: 3971 slots)
KIND_POS, KIND_RING, KIND_FAR, KIND_OUTSIDE = 0, 1, 2, 3


class PromptSet(NamedTuple):
    ids: object            # int32 [N]
    coords: object         # float32 [N, P, 2], (x, y); P = num_pos + num_neg
    point_labels: object   # int32 [N, P]: 1 x num_pos, then 0 x num_neg
    boxes: object          # float32 [N, 4], XYXY inclusive pixel box
    masks: object          # float32 [N, H, W] or None
    counts: object         # int32 [N, 2]: (|inner_i|, |ring_i|)


# ---- the draw rule ----------------------------------------------------------------------------------------------------------------
def draw_ranks(seed: int, k: int, m: int, counter) -> list:
    """k distinct ranks out of m (k <= m) in pick order; counter(t) -> the four Philox counter words of draw t."""
    seed = int(seed) % (1 << 64)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    picks, ordered = [], []
    for t in range(k):
        w = int(sampling.philox4x32_10(list(counter(t)), key)[0])
        r = (w * (m - t)) >> 32
        j = 0
        while j < len(ordered) and ordered[j] <= r:
            r += 1
            j += 1
        ordered.insert(j, r)
        picks.append(r)
    return picks


def draw_points(seed: int, inst: int, kind: int, k: int, m: int) -> list:
    return draw_ranks(seed, k, m, lambda t: (inst, t + 16 * kind, 0, 0))


def choose_instances(present, max_instances: int, seed: int) -> np.ndarray:
    present = np.asarray(present, dtype=np.int32)
    if len(present) <= max_instances:
        return present
    return present[draw_ranks(seed, max_instances, len(present), lambda t: (0, t, 1, 0))]


# ---- host route (numpy): the definition the kernels are tested against ---------------------------------------------------------------
def d1_truncated(labels: np.ndarray, radius: int) -> np.ndarray:
    """min(d1, radius + 1) as int32 [H, W]: a row pass (distance to the nearest different pixel of the row) and a column pass."""
    lab = np.asarray(labels)
    H, W = lab.shape
    R = int(radius)
    pad = np.full((H, W + 2 * R), -1, dtype=np.int64)
    pad[:, R:R + W] = lab
    h = np.full((H, W), R + 1, dtype=np.int32)
    for dx in range(R, 0, -1):
        differ = (pad[:, R - dx:R - dx + W] != lab) | (pad[:, R + dx:R + dx + W] != lab)
        h[differ] = dx
    best = h.copy()
    for dy in range(1, R + 1):
        up = np.full((H, W), dy, dtype=np.int32)
        dn = np.full((H, W), dy, dtype=np.int32)
        if dy < H:
            same = lab[dy:] == lab[:-dy]                    # pixel y (>= dy) against y - dy
            up[dy:][same] = dy + h[:-dy][same]
            dn[:-dy][same] = dy + h[dy:][same]
        best = np.minimum(best, np.minimum(up, dn))
    return np.minimum(best, R + 1)


def _box(m: np.ndarray):
    ys, xs = np.where(m)
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def ring_window(labels: np.ndarray, inst: int, box, lo: int, hi: int):
    """(ring bool [h, w] of the window, (wx0, wy0)): the window is the box grown by hi, clipped to the frame; exact wherever D2 <= hi^2."""
    H, W = labels.shape
    x0, y0, x1, y1 = box
    wx0, wy0, wx1, wy1 = max(x0 - hi, 0), max(y0 - hi, 0), min(x1 + hi, W - 1), min(y1 + hi, H - 1)
    h, w = wy1 - wy0 + 1, wx1 - wx0 + 1
    m = np.zeros((h + 2 * hi, w + 2 * hi), dtype=bool)       # the window with a margin of hi (outside the frame: no instance pixel)
    sy0, sx0 = max(wy0 - hi, 0), max(wx0 - hi, 0)
    sy1, sx1 = min(wy1 + hi, H - 1), min(wx1 + hi, W - 1)
    m[sy0 - (wy0 - hi):sy1 - (wy0 - hi) + 1, sx0 - (wx0 - hi):sx1 - (wx0 - hi) + 1] = labels[sy0:sy1 + 1, sx0:sx1 + 1] == inst
    big = np.int64(1 << 40)
    g = np.full((h, w + 2 * hi), big, dtype=np.int64)        # nearest instance pixel of the column within +- hi
    for dy in range(hi, -1, -1):
        hit = m[hi - dy:hi - dy + h] | m[hi + dy:hi + dy + h]
        g[hit] = dy
    d2 = np.full((h, w), big, dtype=np.int64)
    for dx in range(-hi, hi + 1):
        col = g[:, hi + dx:hi + dx + w]
        d2 = np.minimum(d2, np.where(col < big, col * col + dx * dx, big))
    ring = (~m[hi:hi + h, hi:hi + w]) & (d2 >= lo * lo) & (d2 <= hi * hi)
    return ring, (wx0, wy0)


def _far_from(m: np.ndarray, radius: int) -> np.ndarray:
    """pixels farther than `radius` (city-block) from the set m = outside binary_dilation(m, iterations=radius)"""
    d = m.copy()
    for _ in range(int(radius)):
        e = d.copy()
        e[1:] |= d[:-1]
        e[:-1] |= d[1:]
        e[:, 1:] |= d[:, :-1]
        e[:, :-1] |= d[:, 1:]
        d = e
    return ~d


def fallback_negatives(labels: np.ndarray, inst: int, num_neg: int, inner_radius: int, seed: int) -> np.ndarray:
    """The negatives of an instance whose ring holds fewer than num_neg pixels -> float32 [num_neg, 2]."""
    m = labels == inst
    ys, xs = np.where(_far_from(m, inner_radius))
    kind = KIND_FAR
    if len(ys) < num_neg:
        ys, xs = np.where(~m)
        kind = KIND_OUTSIDE
    if len(ys) == 0:
        raise ValueError(f"prompts_from_labels: instance {inst} fills the frame: there is no pixel for a negative point")
    ranks = draw_points(seed, inst, kind, num_neg, len(ys)) if len(ys) >= num_neg else [j % len(ys) for j in range(num_neg)]
    return np.array([[xs[r], ys[r]] for r in ranks], dtype=np.float32).reshape(num_neg, 2)


def _check_args(num_pos, num_neg, max_instances, inner_radius, ring, on_device=False):
    if not (0 <= int(num_pos) <= MAX_POINTS and 0 <= int(num_neg) <= MAX_POINTS):
        raise ValueError(f"prompts_from_labels: num_pos and num_neg must lie in 0..{MAX_POINTS}")
    if not 1 <= int(max_instances) <= MAX_ID:
        raise ValueError(f"prompts_from_labels: max_instances must lie in 1..{MAX_ID}")
    lo, hi = (int(v) for v in ring)
    if not (int(inner_radius) >= 0 and 0 <= lo <= hi):
        raise ValueError("prompts_from_labels: need inner_radius >= 0 and 0 <= ring[0] <= ring[1]")
    if on_device and (int(inner_radius) > MAX_RADIUS or hi > MAX_RADIUS):
        raise ValueError(f"prompts_from_labels: the device route needs inner_radius <= {MAX_RADIUS} and ring[1] <= {MAX_RADIUS} (the host route has no limit)")
    return lo, hi


def _check_scratch(slots: int, H: int, W: int):
    """The device route sizes its candidate-set scratch by the slots asked for (max_instances, or len(ids)), not by the instances present -- how
    many are present is only known after the one read-back -- so the limit on the slots is one of memory."""
    need = slots * (2 * H * ((W + 63) // 64) * 8 + 2 * H * 4 + 16)
    if need > MAX_SCRATCH_BYTES:
        raise ValueError(f"prompts_from_labels: {slots} instance slots of a {H} x {W} image need {need / 2 ** 30:.1f} GiB of device scratch (limit "
                         f"{MAX_SCRATCH_BYTES / 2 ** 30:.0f} GiB): the scratch is sized by max_instances / len(ids), not by the instances present; "
                         f"ask for at most {MAX_SCRATCH_BYTES // (need // slots)}")


def default_instance(H: int, W: int, num_pos: int, num_neg: int):
    """(coords float32 [1, P, 2], point_labels int32 [1, P]) of an image without instances (_create_default_points)."""
    cx = lambda v: min(max(v, 0), W - 1)
    cy = lambda v: min(max(v, 0), H - 1)
    corners = [(cx(10), cy(10)), (cx(W - 10), cy(10)), (cx(10), cy(H - 10)), (cx(W - 10), cy(H - 10))]
    pts = [(W // 2, H // 2)] * num_pos + [corners[i % 4] for i in range(num_neg)]
    return np.array(pts, dtype=np.float32).reshape(1, num_pos + num_neg, 2), _point_labels(1, num_pos, num_neg)


def _point_labels(n: int, num_pos: int, num_neg: int) -> np.ndarray:
    return np.tile(np.array([1] * num_pos + [0] * num_neg, dtype=np.int32), (n, 1)).reshape(n, num_pos + num_neg)


def candidate_sets_host(labels: np.ndarray, ids, inner_radius: int = 10, ring=(9, 11)):
    """(inner bool [N, H, W], ring bool [N, H, W]) of the given ids, by the host route."""
    labels = np.asarray(labels)
    lo, hi = (int(v) for v in ring)
    H, W = labels.shape
    d1 = d1_truncated(labels, inner_radius)
    inner = np.zeros((len(ids), H, W), dtype=bool)
    rng = np.zeros((len(ids), H, W), dtype=bool)
    for n, i in enumerate(ids):
        m = labels == int(i)
        if not m.any():
            continue
        inner[n] = m & (d1 > inner_radius)
        r, (wx0, wy0) = ring_window(labels, int(i), _box(m), lo, hi)
        rng[n, wy0:wy0 + r.shape[0], wx0:wx0 + r.shape[1]] = r
    return inner, rng


def _host_route(labels, num_pos, num_neg, max_instances, ids, seed, inner_radius, ring, return_masks) -> PromptSet:
    lo, hi = _check_args(num_pos, num_neg, max_instances, inner_radius, ring)
    labels = np.asarray(labels)
    if labels.ndim != 2 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("prompts_from_labels: labels must be an integer image [H, W]")
    if labels.size and (labels.min() < 0 or labels.max() > MAX_ID):
        raise ValueError(f"prompts_from_labels: labels must lie in 0..{MAX_ID}")
    H, W = labels.shape
    P = num_pos + num_neg
    if ids is None:
        present = np.unique(labels[labels > 0])
        if len(present) == 0:
            coords, pl = default_instance(H, W, num_pos, num_neg)
            return PromptSet(np.zeros(1, np.int32), coords, pl, np.zeros((1, 4), np.float32),
                             np.zeros((1, H, W), np.float32) if return_masks else None, np.zeros((1, 2), np.int32))
        chosen = choose_instances(present, max_instances, seed)
    else:
        chosen = np.asarray(ids, dtype=np.int64).reshape(-1)
    N = len(chosen)
    d1 = d1_truncated(labels, inner_radius)
    coords = np.zeros((N, P, 2), np.float32)
    boxes = np.zeros((N, 4), np.float32)
    counts = np.zeros((N, 2), np.int32)
    masks = np.zeros((N, H, W), np.float32) if return_masks else None
    for n, i in enumerate(int(v) for v in chosen):
        m = labels == i
        area = int(m.sum())
        if i < 1 or i > MAX_ID or area == 0:
            raise ValueError(f"prompts_from_labels: id {i} has no pixels in the label image")
        box = _box(m)
        iy, ix = np.where(m & (d1 > inner_radius))
        r, (wx0, wy0) = ring_window(labels, i, box, lo, hi)
        ry, rx = np.where(r)
        ry, rx = ry + wy0, rx + wx0
        if len(iy) >= num_pos:
            pos = [(ix[k], iy[k]) for k in draw_points(seed, i, KIND_POS, num_pos, len(iy))]
        elif len(iy) > 0:
            pos = [(ix[j % len(iy)], iy[j % len(iy)]) for j in range(num_pos)]
        else:
            ys, xs = np.where(m)
            pos = [(int(xs.sum()) // area, int(ys.sum()) // area)] * num_pos
        coords[n, :num_pos] = np.array(pos, dtype=np.float32).reshape(num_pos, 2)
        if len(ry) >= num_neg:
            coords[n, num_pos:] = np.array([(rx[k], ry[k]) for k in draw_points(seed, i, KIND_RING, num_neg, len(ry))], dtype=np.float32).reshape(num_neg, 2)
        else:
            coords[n, num_pos:] = fallback_negatives(labels, i, num_neg, inner_radius, seed)
        boxes[n] = box
        counts[n] = (len(iy), len(ry))
        if return_masks:
            masks[n] = m
    return PromptSet(chosen.astype(np.int32), coords, _point_labels(N, num_pos, num_neg), boxes, masks, counts)


# ---- device route -----------------------------------------------------------------------------------------------------------------
def _device_labels(labels, device):
    """int32 [H, W] on the device.  Wider integers are clamped to -1..65536 before the conversion, so a label outside 0..65535 stays outside it
    (the kernels report it) and cannot wrap into the range."""
    import torch
    if isinstance(labels, torch.Tensor):
        if device is None and not labels.is_cuda:
            raise ValueError("prompts_from_labels: a CPU tensor needs device=... for the kernels (or pass labels.numpy() for the host route)")
        if labels.dim() != 2 or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
            raise ValueError("prompts_from_labels: labels must be an integer image [H, W]")
        t = labels if device is None else labels.to(device)
        if not t.is_cuda:
            raise ValueError(f"prompts_from_labels: device {device!r} is not a GPU; pass numpy labels with device=None for the host route")
        if t.dtype != torch.int32:
            t = t.to(torch.int64).clamp(-1, MAX_ID + 1).to(torch.int32)
        return t.contiguous()
    a = np.asarray(labels)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("prompts_from_labels: labels must be an integer image [H, W]")
    if torch.device(device).type != "cuda":
        raise ValueError(f"prompts_from_labels: device {device!r} is not a GPU; pass numpy labels with device=None for the host route")
    return torch.from_numpy(np.ascontiguousarray(np.clip(a.astype(np.int64), -1, MAX_ID + 1).astype(np.int32))).to(device)


def _device_sets(t, slots, sel, info, seed, inner_radius, ring, max_instances, debug):
    """The kernels up to the candidate sets, on the current device; no host synchronisation."""
    from .. import ops
    areas, boxes_t = ops.label_stats(t, MAX_ID)            # the label image read as a transposed map: its boxes are (y0, x0, y1, x1)
    d1, _ = ops.label_d1(t, inner_radius, status=info[1:2])
    if sel is None:
        sel, _ = ops.prompt_choose(areas, max_instances, seed, info=info)
    else:
        info[:1].fill_(slots)
    bits, rowcnt, sums, dbg = ops.prompt_sets(t, d1, areas, boxes_t, sel, info, inner_radius, ring, debug=debug)
    return areas, boxes_t, sel, bits, rowcnt, sums, dbg


def _device_route(labels, num_pos, num_neg, max_instances, ids, seed, inner_radius, ring, device, return_masks) -> PromptSet:
    import torch
    from .. import ops
    lo, hi = _check_args(num_pos, num_neg, max_instances, inner_radius, ring, on_device=True)
    t = _device_labels(labels, device)
    H, W = t.shape
    P = num_pos + num_neg
    if H == 0 or W == 0:
        raise ValueError("prompts_from_labels: the label image is empty")
    with torch.cuda.device(t.device):
        sel = None
        slots = int(max_instances)
        if ids is not None:
            sel = (ids.to(device=t.device, dtype=torch.int64) if isinstance(ids, torch.Tensor)           # clamped like the labels: no id wraps into range
                   else torch.tensor([min(max(int(v), -1), MAX_ID + 1) for v in ids], dtype=torch.int64, device=t.device))
            sel = sel.clamp(-1, MAX_ID + 1).to(torch.int32).reshape(-1).contiguous()
            slots = sel.numel()
            if slots == 0:
                z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=t.device)
                return PromptSet(z(0, dt=torch.int32), z(0, P, 2), z(0, P, dt=torch.int32), z(0, 4), z(0, H, W) if return_masks else None, z(0, 2, dt=torch.int32))
        _check_scratch(slots, H, W)
        info = torch.zeros((2 + 4 * slots,), dtype=torch.int32, device=t.device)
        areas, boxes_t, sel, bits, rowcnt, sums, _ = _device_sets(t, slots, sel, info, seed, inner_radius, (lo, hi), max_instances, False)
        coords, boxes, counts = ops.prompt_points((H, W), areas, boxes_t, sel, info, bits, rowcnt, sums, hi, num_pos, num_neg, seed)
        host = info.cpu().numpy()                            # the one device-to-host copy: how many, the status, (id, area, |inner|, |ring|) per slot
        if host[1]:
            raise ValueError(f"prompts_from_labels: labels must lie in 0..{MAX_ID}")
        K = int(host[0])
        if K == 0:
            c, pl = default_instance(H, W, num_pos, num_neg)
            z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=t.device)
            return PromptSet(z(1, dt=torch.int32), torch.from_numpy(c).to(t.device), torch.from_numpy(pl).to(t.device), z(1, 4),
                             z(1, H, W) if return_masks else None, z(1, 2, dt=torch.int32))
        rec = host[2:2 + 4 * K].reshape(K, 4)
        for i, area in rec[:, :2]:
            if area == 0:
                raise ValueError(f"prompts_from_labels: id {int(i)} has no pixels in the label image")
        coords, boxes, counts, sel = coords[:K], boxes[:K], counts[:K], sel[:K]
        short = [s for s in range(K) if rec[s, 3] < num_neg]
        if short:                                            # an instance that nearly fills the frame: the fallbacks run on the host
            lab = t.cpu().numpy()
            for s in short:
                coords[s, num_pos:] = torch.from_numpy(fallback_negatives(lab, int(rec[s, 0]), num_neg, inner_radius, seed)).to(t.device)
        masks = ops.instance_masks(t, sel.contiguous()) if return_masks else None
        pl = torch.from_numpy(_point_labels(K, num_pos, num_neg)).to(t.device)
        return PromptSet(sel, coords, pl, boxes, masks, counts)


def candidate_sets(labels, ids, inner_radius: int = 10, ring=(9, 11), device=None):
    """The two candidate sets of the given ids as boolean images (inner [N, H, W], ring [N, H, W]): numpy labels with device=None take the host
    route, anything else the kernels' debug output."""
    import torch
    if device is None and not isinstance(labels, torch.Tensor):
        return candidate_sets_host(labels, ids, inner_radius, ring)
    _check_args(0, 0, 1, inner_radius, ring, on_device=True)
    t = _device_labels(labels, device)
    with torch.cuda.device(t.device):
        sel = torch.tensor([int(v) for v in ids], dtype=torch.int32, device=t.device)
        info = torch.zeros((2 + 4 * sel.numel(),), dtype=torch.int32, device=t.device)
        dbg = _device_sets(t, sel.numel(), sel, info, 0, inner_radius, tuple(int(v) for v in ring), 1, True)[-1]
        return dbg[0].bool(), dbg[1].bool()


def prompts_from_labels(labels, num_pos: int = 1, num_neg: int = 3, max_instances: int = 4, ids=None, seed: int = 0, inner_radius: int = 10,
                        ring=(9, 11), device=None, return_masks: bool = True) -> PromptSet:
    """Prompts and per-instance masks of (at most max_instances of) the instances of an int label image [H, W] (module docstring: definitions).
    A numpy `labels` with device=None takes the host route and returns numpy arrays; a CUDA tensor, or a given `device`, takes the kernels
    (csrc/prompts.hip) and returns tensors on that device after ONE device-to-host copy of a few integers.  Both routes return the same values.
    (coords, point_labels) and masks go into training.train_step_loss unchanged; boxes are XYXY inclusive pixel boxes.
    Limits of the device route, checked before anything is launched (ValueError): inner_radius and ring[1] <= 64; the candidate-set scratch is
    sized by max_instances (or len(ids)), not by the instances present, and may take 1 GiB -- 3971 slots at 1024^2; a CPU tensor needs `device`."""
    import torch
    if device is None and not isinstance(labels, torch.Tensor):
        return _host_route(labels, int(num_pos), int(num_neg), int(max_instances), ids, seed, int(inner_radius), ring, return_masks)
    return _device_route(labels, int(num_pos), int(num_neg), int(max_instances), ids, seed, int(inner_radius), ring, device, return_masks)
