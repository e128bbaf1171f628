"""Per-instance measurements and contacts from an instance label image: the table that comes after generate_label_map /
generate_tiled_label_map / InteractiveSegmenter.export_labels.  This module is the definition (vectorised numpy on int64, integers only) and
the driver of the device route (csrc/measure.hip); the two are equal bit for bit (tests/test_measure_*.py).  DESIGN.md "7b, continued:
measurements" states the definitions, the limits and what is out of scope.

    table = measure_instances(labels, intensity=image, device="cuda")     # InstanceTable of tensors on the device
    pairs = label_contacts(labels, device="cuda")                         # int64 [P, 3] = (a, b, shared pixel sides)
    props = derive(table, pixel_size=0.325)                               # float64 numpy: centroid, axes, orientation, mean, std, ...

labels int32 [H, W] with ids 0..K, 0 = background, 1 <= H, W <= 46340 (then x * x < 2^31, every area < 2^31 and every sum below stays under
2^62).  Row k - 1 of every table belongs to label k; ids without a pixel are allowed.  An id outside 0..K raises UllsamError.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib

MAX_SIDE = 46340
MAX_CHANNELS = 4
INT_MAX = 2 ** 31 - 1


class InstanceTable(NamedTuple):
    """area int64 [K]; box int32 [K, 4] inclusive XYXY, (INT_MAX, INT_MAX, -1, -1) for an absent label; moments int64 [K, 5] = sum x, sum y,
    sum x^2, sum y^2, sum xy over the instance's pixels in frame coordinates; perimeter int64 [K, 3] = (boundary_pixels, edges, contact_edges);
    isum / isum2 int64 [K, C] = sum v, sum v^2; imin / imax int32 [K, C], (INT_MAX, -1) for an absent label; the four are None without an image."""
    area: torch.Tensor
    box: torch.Tensor
    moments: torch.Tensor
    perimeter: torch.Tensor
    isum: Optional[torch.Tensor] = None
    isum2: Optional[torch.Tensor] = None
    imin: Optional[torch.Tensor] = None
    imax: Optional[torch.Tensor] = None


def _check_frame(shape, what: str):
    if len(shape) != 2:
        raise ValueError(f"{what}: labels must be [H, W], got {tuple(shape)}")
    h, w = (int(v) for v in shape)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise _lib.UllsamError(f"{what}: a frame of {h} x {w} (each side must lie in 1..{MAX_SIDE})")
    return h, w


def _check_intensity(intensity, h: int, w: int) -> int:
    """-> C.  uint8 / uint16, [H, W] or interleaved [H, W, C], C in 1..4."""
    dt = str(intensity.dtype).replace("torch.", "")
    if dt not in ("uint8", "uint16"):
        raise _lib.UllsamError(f"measure_instances: the intensity image must be uint8 or uint16, got {dt} (float sums depend on the order of arrival: out of scope)")
    shape = tuple(int(v) for v in intensity.shape)
    if len(shape) not in (2, 3) or shape[:2] != (h, w):
        raise ValueError(f"measure_instances: intensity {shape} for labels {(h, w)}")
    c = 1 if len(shape) == 2 else shape[2]
    if not 1 <= c <= MAX_CHANNELS:
        raise _lib.UllsamError(f"measure_instances: {c} channels (1..{MAX_CHANNELS}, interleaved [H, W, C])")
    return c


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _num(labels, num) -> int:
    if num is None:
        num = max(int(labels.max()), 0)                   # (one read-back on the device route)
    num = int(num)
    if not 0 <= num <= 2 ** 31 - 2:
        raise _lib.UllsamError(f"measure: num = {num} must lie in 0..2^31 - 2")
    return num


def _wsum(idx: np.ndarray, wgt: np.ndarray, k: int) -> np.ndarray:
    """sum of the integer weights wgt (0 <= wgt < 2^32) per index, exact: np.bincount adds in float64, which is exact while every partial sum is an
    integer below 2^53; larger weights go in two 16-bit halves (each half sums to less than 2^16 * 2^31)."""
    wgt = wgt.astype(np.int64)
    if wgt.size == 0 or int(wgt.max()) * wgt.size < 2 ** 53:
        return np.bincount(idx, weights=wgt, minlength=k).astype(np.int64)
    lo = np.bincount(idx, weights=wgt & 0xffff, minlength=k).astype(np.int64)
    hi = np.bincount(idx, weights=wgt >> 16, minlength=k).astype(np.int64)
    return lo + (hi << 16)


def _ext(idx: np.ndarray, val: np.ndarray, k: int, smallest: bool) -> np.ndarray:
    acc = np.full((k,), INT_MAX if smallest else -1, np.int64)
    (np.minimum if smallest else np.maximum).at(acc, idx, val)
    return acc.astype(np.int32)


def _check_ids(lab: np.ndarray, k: int, what: str):
    if lab.size and (int(lab.min()) < 0 or int(lab.max()) > k):
        raise _lib.UllsamError(f"{what}: the label image holds an id outside 0..{k}")


def _measure_host(lab: np.ndarray, img: Optional[np.ndarray], k: int) -> Dict[str, np.ndarray]:
    h, w = lab.shape
    _check_ids(lab, k, "measure_instances")
    ys, xs = np.nonzero(lab)
    idx = lab[ys, xs].astype(np.int64) - 1
    out = {"area": np.bincount(idx, minlength=k).astype(np.int64)}
    out["box"] = np.stack([_ext(idx, xs, k, True), _ext(idx, ys, k, True), _ext(idx, xs, k, False), _ext(idx, ys, k, False)], 1)
    out["moments"] = np.stack([_wsum(idx, xs, k), _wsum(idx, ys, k), _wsum(idx, xs * xs, k), _wsum(idx, ys * ys, k), _wsum(idx, xs * ys, k)], 1)
    pad = np.full((h + 2, w + 2), -1, np.int32)           # -1: the frame's outside is "not k" and is no instance
    pad[1:-1, 1:-1] = lab
    e = np.zeros((h, w), np.int32)
    ce = np.zeros((h, w), np.int32)
    for nb in (pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]):
        d = nb != lab
        e += d
        ce += d & (nb > 0)
    ef, cf = e[ys, xs], ce[ys, xs]
    out["perimeter"] = np.stack([_wsum(idx, ef > 0, k), _wsum(idx, ef, k), _wsum(idx, cf, k)], 1)
    if img is not None:
        v = img.reshape(h, w, -1)[ys, xs].astype(np.int64)                                  # [n, C]
        c = v.shape[1]
        out["isum"] = np.stack([_wsum(idx, v[:, j], k) for j in range(c)], 1)
        out["isum2"] = np.stack([_wsum(idx, v[:, j] * v[:, j], k) for j in range(c)], 1)
        out["imin"] = np.stack([_ext(idx, v[:, j], k, True) for j in range(c)], 1)
        out["imax"] = np.stack([_ext(idx, v[:, j], k, False) for j in range(c)], 1)
    return out


def measure_instances(labels, intensity=None, num=None, device=None, lds_slots=None) -> InstanceTable:
    """The InstanceTable of a label image.  Definitions, for label k with pixel set m (the frame's outside counts as "not k" throughout):
      area = |m|; box = the inclusive bounds of m; moments = sum x, sum y, sum x^2, sum y^2, sum xy over m;
      boundary_pixels = the pixels of m with at least one 4-neighbour outside m (= |m xor binary_erosion(m)| with scipy's defaults);
      edges = the pixel sides of m's pixels that face a pixel outside m (the crack-length perimeter);
      contact_edges = those of `edges` that face ANOTHER instance (neighbour > 0 and != k; the frame's outside does not count);
      isum, isum2, imin, imax = sum v, sum v^2, min v, max v per channel of `intensity` (uint8 / uint16, [H, W] or interleaved [H, W, C], C <= 4).
    labels: numpy, a CPU tensor or a device tensor; num = K (default labels.max(): one read-back on the device route).
    device None / "cpu": this definition in numpy (np.bincount on int64).  A GPU device: csrc/measure.hip on the labels and the image where they
    are; the tables stay on the device and the status word is read back once.  lds_slots (device route only; None = ops.MEASURE_LDS_SLOTS): the
    entries of the per-workgroup LDS table the runs of equal labels are summed in before they reach the global tables; 0 = every run straight to
    the global tables, the slower side of the A/B of tools/measure_bench.py (profiles/r16_measure.txt); the result does not depend on it.
    float intensity raises (float sums depend on the order of arrival), as do more than 4 channels, a side above 46340 and an id outside 0..K."""
    h, w = _check_frame(tuple(labels.shape), "measure_instances")
    if intensity is not None:
        _check_intensity(intensity, h, w)
    dev = torch.device("cpu" if device is None else device)
    if dev.type != "cuda":
        lab = _host(labels).astype(np.int32, copy=False)
        k = _num(lab, num)
        t = _measure_host(lab, None if intensity is None else _host(intensity), k)
        return InstanceTable(**{n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in t.items()})
    from .. import ops
    lab = torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()
    k = _num(lab, num)
    img = None if intensity is None else torch.as_tensor(intensity).to(dev).contiguous()
    t, flags = ops.measure_instances(lab, k, img, ops.MEASURE_LDS_SLOTS if lds_slots is None else lds_slots)
    if int(flags.cpu()[0]):
        raise _lib.UllsamError(f"measure_instances: the label image holds an id outside 0..{k}")
    return InstanceTable(**t)


def _contacts_host(lab: np.ndarray, k: int, max_pairs: int) -> np.ndarray:
    _check_ids(lab, k, "label_contacts")
    keys = []
    for a, b in ((lab[:, :-1], lab[:, 1:]), (lab[:-1, :], lab[1:, :])):                     # right and down: every adjacent pixel pair once
        m = (a > 0) & (b > 0) & (a != b)
        a, b = a[m].astype(np.int64), b[m].astype(np.int64)
        keys.append((np.minimum(a, b) << 32) | np.maximum(a, b))
    key, n = np.unique(np.concatenate(keys), return_counts=True)
    if len(key) > max_pairs:
        raise _lib.UllsamError(f"label_contacts: more than max_pairs = {max_pairs} distinct pairs of touching instances")
    return np.stack([key >> 32, key & 0xffffffff, n.astype(np.int64)], 1).reshape(-1, 3)


def label_contacts(labels, num=None, max_pairs: int = 1 << 20, device=None) -> torch.Tensor:
    """Which instances touch and along what length: int64 [P, 3], the rows (a, b, n) with 0 < a < b sorted by (a, b), n = the number of pixel sides
    shared by a pixel of a and a 4-neighbour pixel of b (every adjacent pixel pair is counted once, by looking right and down only).  For every k
    the sum of n over the rows naming k equals measure_instances(...).perimeter[k - 1, 2] (contact_edges).  More than max_pairs distinct pairs
    raise UllsamError (nothing is truncated).  device as in measure_instances; on the device route the pair table has the power of two
    >= 2 * max_pairs slots of 16 bytes and the status words are read back once."""
    h, w = _check_frame(tuple(labels.shape), "label_contacts")
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise ValueError(f"label_contacts: max_pairs must lie in 1..2^30, got {max_pairs}")
    dev = torch.device("cpu" if device is None else device)
    if dev.type != "cuda":
        lab = _host(labels).astype(np.int32, copy=False)
        return torch.from_numpy(np.ascontiguousarray(_contacts_host(lab, _num(lab, num), max_pairs)))
    from .. import ops
    lab = torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()
    k = _num(lab, num)
    rows, flags = ops.label_contacts(lab, k, max_pairs)
    fl = flags.cpu().numpy()
    if fl[0]:
        raise _lib.UllsamError(f"label_contacts: the label image holds an id outside 0..{k}")
    if fl[1] or fl[2] > max_pairs:
        raise _lib.UllsamError(f"label_contacts: more than max_pairs = {max_pairs} distinct pairs of touching instances")
    rows = rows[:int(fl[2])]
    rows = rows[torch.argsort(rows[:, 0])]                # keys are distinct: the order is the order of (a, b)
    return torch.stack([rows[:, 0] >> 32, rows[:, 0] & 0xffffffff, rows[:, 1]], 1)


def derive(table: InstanceTable, pixel_size: float = 1.0) -> Dict[str, np.ndarray]:
    """Region properties from an InstanceTable, in float64 on the host (shared by both routes: equal tables give equal values).  The numerators
    A sum x^2 - (sum x)^2, A sum y^2 - (sum y)^2, A sum xy - sum x sum y and A sum v^2 - (sum v)^2 exceed int64 and are formed in Python integers;
    one int / int division by A^2 gives the central moments u20, u02, u11 and the variance.
      area = A pixel_size^2; centroid = (sum x / A, sum y / A) pixel_size; equivalent_diameter = sqrt(4 A / pi) pixel_size;
      l1, l2 = (u20 + u02) / 2 +- sqrt(((u20 - u02) / 2)^2 + u11^2); major_axis_length, minor_axis_length = 4 sqrt(l1), 4 sqrt(l2) (x pixel_size);
      eccentricity = sqrt(1 - l2 / l1), 0 when l1 == 0; orientation = 0.5 atan2(2 u11, u20 - u02): the angle of the major axis to the +x axis, y down;
      perimeter = edges pixel_size, contact_length = contact_edges pixel_size; mean, std (population), min, max per channel [K, C] with an image.
    Absent labels give NaN.  These are the usual region-property formulas; scikit-image is not available where this is built, so equality with
    its regionprops is neither claimed nor tested."""
    ps = float(pixel_size)
    area = _host(table.area).astype(np.int64)
    mom = _host(table.moments).astype(np.int64)
    per = _host(table.perimeter).astype(np.int64)
    k = len(area)
    nan = lambda *s: np.full(s, np.nan, np.float64)
    out = {"area": nan(k), "centroid": nan(k, 2), "equivalent_diameter": nan(k), "major_axis_length": nan(k), "minor_axis_length": nan(k),
           "eccentricity": nan(k), "orientation": nan(k), "perimeter": nan(k), "contact_length": nan(k)}
    has_img = table.isum is not None
    if has_img:
        isum, isum2 = _host(table.isum).astype(np.int64), _host(table.isum2).astype(np.int64)
        imin, imax = _host(table.imin), _host(table.imax)
        c = isum.shape[1]
        out.update(mean=nan(k, c), std=nan(k, c), min=nan(k, c), max=nan(k, c))
    for i in range(k):
        a = int(area[i])
        if a == 0:
            continue
        sx, sy, sxx, syy, sxy = (int(v) for v in mom[i])
        u20, u02, u11 = (a * sxx - sx * sx) / (a * a), (a * syy - sy * sy) / (a * a), (a * sxy - sx * sy) / (a * a)
        mid, rad = (u20 + u02) / 2, math.sqrt(((u20 - u02) / 2) ** 2 + u11 ** 2)
        l1, l2 = mid + rad, max(mid - rad, 0.0)
        out["area"][i] = a * ps * ps
        out["centroid"][i] = (sx / a * ps, sy / a * ps)
        out["equivalent_diameter"][i] = math.sqrt(4 * a / math.pi) * ps
        out["major_axis_length"][i] = 4 * math.sqrt(l1) * ps
        out["minor_axis_length"][i] = 4 * math.sqrt(l2) * ps
        out["eccentricity"][i] = math.sqrt(max(1 - l2 / l1, 0.0)) if l1 > 0 else 0.0
        out["orientation"][i] = 0.5 * math.atan2(2 * u11, u20 - u02)
        out["perimeter"][i] = int(per[i, 1]) * ps
        out["contact_length"][i] = int(per[i, 2]) * ps
        if has_img:
            for j in range(c):
                s, s2 = int(isum[i, j]), int(isum2[i, j])
                out["mean"][i, j] = s / a
                out["std"][i, j] = math.sqrt((a * s2 - s * s) / (a * a))
                out["min"][i, j] = float(imin[i, j])
                out["max"][i, j] = float(imax[i, j])
    return out
