"""Per-object measurements and contacts from a label VOLUME -- utils.measure with a third axis: one row per 3-D object giving its size, place,
shape, brightness and neighbours; the table that comes after link_label_stack / generate_stack_label_volume, split_labels3d, expand_labels3d and
shrink_labels3d.  This module is the definition (vectorised numpy on int64, integers only) and the driver of the device route
(csrc/measure3d.hip); the two are equal bit for bit (tests/test_measure3d_*.py).  DESIGN.md "7b, continued (3-D measurements)" states the
definitions, the limits and what is out of scope.

    volume, records, objects = generator.generate_stack_label_volume(stack)   # int32 [Z, H, W] on the device
    table = measure_objects(volume, intensity=stack)                          # ObjectTable of tensors, on the device where the volume is
    pairs = object_contacts(volume)                                           # int64 [P, 5] = (a, b, nz, ny, nx): shared voxel faces per axis
    props = derive3d(table, spacing=(2.5, 1.0, 1.0))                          # float64 numpy: volume, centroid, axes, surface area, mean, ...

volume int32 [Z, H, W] with ids 0..K, 0 = background.  Limits (ValueError stating the number, before any voxel is read): 1 <= Z, H, W <= 32767 and
Z * H * W <= 2^31 - 1.  Row k - 1 of every table belongs to id k; absent ids are allowed.  An id outside 0..K raises UllsamError.

Bounds.  With N = Z * H * W <= 2^31 - 1 voxels and coordinates <= 32766 < 2^15, per column of the tables:
  voxels, boundary_voxels <= N < 2^31; every face count f_a, c_a <= 2 N < 2^32;
  sum x, sum y, sum z <= 32766 N < 2^46; sum x^2 .. sum yz <= 32766^2 N < 2^61;
  isum <= 65535 N < 2^47; isum2 <= 65535^2 N < 2^63 -- the largest of all, still inside int64;
  an object_contacts count <= N < 2^31 per axis.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from .distance import _route
from .measure import INT_MAX, MAX_CHANNELS, _check_ids, _ext, _host, _num, _wsum

MAX_SIDE = 32767
MAX_VOXELS = 2 ** 31 - 1


class ObjectTable(NamedTuple):
    """voxels int64 [K]; box int32 [K, 6] inclusive (x0, y0, z0, x1, y1, z1), (INT_MAX, INT_MAX, INT_MAX, -1, -1, -1) for an absent id; moments
    int64 [K, 9] = sum x, y, z, x^2, y^2, z^2, xy, xz, yz over the object's voxels in voxel indices; surface int64 [K, 7] = (boundary_voxels, fz,
    fy, fx, cz, cy, cx); isum / isum2 int64 [K, C] = sum v, sum v^2; imin / imax int32 [K, C], (INT_MAX, -1) for an absent id; the four are None
    without an image."""
    voxels: torch.Tensor
    box: torch.Tensor
    moments: torch.Tensor
    surface: torch.Tensor
    isum: Optional[torch.Tensor] = None
    isum2: Optional[torch.Tensor] = None
    imin: Optional[torch.Tensor] = None
    imax: Optional[torch.Tensor] = None


def _check_volume(volume, what: str):
    """-> (Z, H, W), every limit checked before any voxel is read (a stub with a .shape is enough)."""
    shape = tuple(volume.shape) if hasattr(volume, "shape") else ()
    if len(shape) != 3:
        raise ValueError(f"{what}: volume must be [Z, H, W], got {shape}")
    n = tuple(int(v) for v in shape)
    for v in n:
        if not 1 <= v <= MAX_SIDE:
            raise ValueError(f"{what}: a volume of {n[0]} x {n[1]} x {n[2]}: the side {v} must lie in 1..{MAX_SIDE}")
    if n[0] * n[1] * n[2] > MAX_VOXELS:
        raise ValueError(f"{what}: a volume of {n[0]} x {n[1]} x {n[2]} = {n[0] * n[1] * n[2]} voxels (at most 2^31 - 1)")
    return n


def _check_intensity(intensity, n) -> int:
    """-> C.  uint8 / uint16, [Z, H, W] or interleaved [Z, H, W, C], C in 1..4."""
    dt = str(intensity.dtype).replace("torch.", "")
    if dt not in ("uint8", "uint16"):
        raise _lib.UllsamError(f"measure_objects: the intensity image must be uint8 or uint16, got {dt} (float sums depend on the order of arrival: out of scope)")
    shape = tuple(int(v) for v in intensity.shape)
    if len(shape) not in (3, 4) or shape[:3] != tuple(n):
        raise ValueError(f"measure_objects: intensity {shape} for a volume {tuple(n)}")
    c = 1 if len(shape) == 3 else shape[3]
    if not 1 <= c <= MAX_CHANNELS:
        raise _lib.UllsamError(f"measure_objects: {c} channels (1..{MAX_CHANNELS}, interleaved [Z, H, W, C])")
    return c


def _measure_host(vol: np.ndarray, img: Optional[np.ndarray], k: int) -> Dict[str, np.ndarray]:
    z, h, w = vol.shape
    _check_ids(vol, k, "measure_objects")
    zs, ys, xs = np.nonzero(vol)
    idx = vol[zs, ys, xs].astype(np.int64) - 1
    out = {"voxels": np.bincount(idx, minlength=k).astype(np.int64)}
    out["box"] = np.stack([_ext(idx, xs, k, True), _ext(idx, ys, k, True), _ext(idx, zs, k, True),
                           _ext(idx, xs, k, False), _ext(idx, ys, k, False), _ext(idx, zs, k, False)], 1)
    out["moments"] = np.stack([_wsum(idx, v, k) for v in (xs, ys, zs, xs * xs, ys * ys, zs * zs, xs * ys, xs * zs, ys * zs)], 1)
    pad = np.full((z + 2, h + 2, w + 2), -1, np.int32)    # -1: the volume's outside is "not k" and is no object
    pad[1:-1, 1:-1, 1:-1] = vol
    mid = slice(1, -1)
    faces, touch = [], []
    for a in range(3):                                    # the two neighbours along z, then y, then x
        f = np.zeros((z, h, w), np.int32)
        c = np.zeros((z, h, w), np.int32)
        for side in (slice(None, -2), slice(2, None)):
            nb = pad[tuple(side if b == a else mid for b in range(3))]
            d = nb != vol
            f += d
            c += d & (nb > 0)
        faces.append(f[zs, ys, xs])
        touch.append(c[zs, ys, xs])
    bnd = (faces[0] + faces[1] + faces[2]) > 0
    out["surface"] = np.stack([_wsum(idx, bnd, k)] + [_wsum(idx, v, k) for v in faces + touch], 1)
    if img is not None:
        v = img.reshape(z, h, w, -1)[zs, ys, xs].astype(np.int64)                           # [n, C]
        c = v.shape[1]
        out["isum"] = np.stack([_wsum(idx, v[:, j], k) for j in range(c)], 1)
        out["isum2"] = np.stack([_wsum(idx, v[:, j] * v[:, j], k) for j in range(c)], 1)
        out["imin"] = np.stack([_ext(idx, v[:, j], k, True) for j in range(c)], 1)
        out["imax"] = np.stack([_ext(idx, v[:, j], k, False) for j in range(c)], 1)
    return out


def measure_objects(volume, intensity=None, num=None, device=None, lds_slots=None) -> ObjectTable:
    """The ObjectTable of a label volume.  Definitions, for id k with voxel set m (the volume's outside counts as "not k" throughout and is no
    object, as in utils.measure):
      voxels = |m|; box = the inclusive bounds of m, (x0, y0, z0, x1, y1, z1); moments = sum x, y, z, x^2, y^2, z^2, xy, xz, yz over m in voxel
      indices (spacing enters only in derive3d);
      boundary_voxels = the voxels of m with at least one of their 6 neighbours outside m;
      f_a (a = z, y, x) = the voxel faces of m's voxels normal to axis a that face a voxel outside m;
      c_a = those of f_a that face ANOTHER object (neighbour > 0 and != k);
      isum, isum2, imin, imax = sum v, sum v^2, min v, max v per channel of `intensity` (uint8 / uint16, [Z, H, W] or interleaved [Z, H, W, C],
      C <= 4).
    volume: numpy, a CPU tensor or a device tensor; num = K (default volume.max(): one read-back on the device route).
    device None: where the volume is (numpy, CPU tensor: this definition in numpy; a GPU tensor: csrc/measure3d.hip on the volume and the image
    where they are -- the volume of link_label_stack goes in without a host trip); "cpu" / a GPU device: that route.  The tables of the device
    route stay on the device and the status word is read back once.  lds_slots (device route only; None = ops.MEASURE3D_LDS_SLOTS): the entries of
    the per-workgroup LDS table the runs of equal labels are summed in before they reach the global tables, 0 or a power of two <= 128; 0 = every
    run straight to the global tables, the slower side of the A/B of tools/measure3d_bench.py (profiles/r25_measure3d.txt); the result does not
    depend on it.
    float intensity raises (float sums depend on the order of arrival), as do more than 4 channels and an id outside 0..K."""
    n = _check_volume(volume, "measure_objects")
    if intensity is not None:
        _check_intensity(intensity, n)
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host(volume).astype(np.int32, copy=False)
        k = _num(vol, num)
        t = _measure_host(vol, None if intensity is None else _host(intensity), k)
        return ObjectTable(**{name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in t.items()})
    from .. import ops
    vol = torch.as_tensor(volume).to(device=dev, dtype=torch.int32).contiguous()
    k = _num(vol, num)
    img = None if intensity is None else torch.as_tensor(intensity).to(dev).contiguous()
    t, flags = ops.measure_objects3d(vol, k, img, ops.MEASURE3D_LDS_SLOTS if lds_slots is None else lds_slots)
    if int(flags.cpu()[0]):
        raise _lib.UllsamError(f"measure_objects: the label volume holds an id outside 0..{k}")
    return ObjectTable(**t)


def _contacts_host(vol: np.ndarray, k: int, max_pairs: int) -> np.ndarray:
    _check_ids(vol, k, "object_contacts")
    keys, axes = [], []
    for axis in range(3):                                 # forward along z, y, x: every adjacent voxel pair once
        a = vol[tuple(slice(None, -1) if b == axis else slice(None) for b in range(3))]
        b = vol[tuple(slice(1, None) if c == axis else slice(None) for c in range(3))]
        m = (a > 0) & (b > 0) & (a != b)
        a, b = a[m].astype(np.int64), b[m].astype(np.int64)
        keys.append((np.minimum(a, b) << 32) | np.maximum(a, b))
        axes.append(np.full(len(a), axis, np.int64))
    keys, axes = np.concatenate(keys), np.concatenate(axes)
    key, inv = np.unique(keys, return_inverse=True)
    if len(key) > max_pairs:
        raise _lib.UllsamError(f"object_contacts: more than max_pairs = {max_pairs} distinct pairs of touching objects")
    n = np.zeros((len(key), 3), np.int64)
    np.add.at(n, (inv.reshape(-1), axes), 1)
    return np.concatenate([np.stack([key >> 32, key & 0xffffffff], 1).reshape(-1, 2), n], 1).astype(np.int64).reshape(-1, 5)


def object_contacts(volume, num=None, max_pairs: int = 1 << 20, device=None) -> torch.Tensor:
    """Which objects touch and over what faces: int64 [P, 5], the rows (a, b, nz, ny, nx) with 0 < a < b sorted by (a, b); n_a = the voxel faces
    normal to axis a shared by a voxel of a and its neighbour voxel of b (every adjacent voxel pair is counted once, by looking forward along each
    axis only).  For every k the sums of nz, ny, nx over the rows naming k equal measure_objects(...).surface[k - 1, 4:7] (cz, cy, cx).  More than
    max_pairs distinct pairs raise UllsamError (nothing is truncated).  device as in measure_objects; on the device route the pair table has the
    power of two >= 2 * max_pairs slots of 32 bytes and the status words are read back once."""
    _check_volume(volume, "object_contacts")
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise ValueError(f"object_contacts: max_pairs must lie in 1..2^30, got {max_pairs}")
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host(volume).astype(np.int32, copy=False)
        return torch.from_numpy(np.ascontiguousarray(_contacts_host(vol, _num(vol, num), max_pairs)))
    from .. import ops
    vol = torch.as_tensor(volume).to(device=dev, dtype=torch.int32).contiguous()
    k = _num(vol, num)
    rows, flags = ops.object_contacts3d(vol, k, max_pairs)
    fl = flags.cpu().numpy()
    if fl[0]:
        raise _lib.UllsamError(f"object_contacts: the label volume holds an id outside 0..{k}")
    if fl[1] or fl[2] > max_pairs:
        raise _lib.UllsamError(f"object_contacts: more than max_pairs = {max_pairs} distinct pairs of touching objects")
    rows = rows[:int(fl[2])]
    rows = rows[torch.argsort(rows[:, 0])]                # keys are distinct: the order is the order of (a, b)
    return torch.cat([torch.stack([rows[:, 0] >> 32, rows[:, 0] & 0xffffffff], 1), rows[:, 1:]], 1)


def derive3d(table: ObjectTable, spacing=(1.0, 1.0, 1.0)) -> Dict[str, np.ndarray]:
    """Object properties from an ObjectTable, in float64 on the host (shared by both routes: equal tables give equal values).  spacing = (sz, sy,
    sx), positive reals: the physical size of a voxel.  The numerators V sum ab - sum a sum b and V sum v^2 - (sum v)^2 exceed int64 and are formed
    in Python integers; one int / int division by V^2 gives the central moments and the variance.
      volume = V sz sy sx; centroid [K, 3] = (sum x / V sx, sum y / V sy, sum z / V sz); equivalent_diameter = (6 volume / pi)^(1/3);
      covariance [K, 3, 3] in (x, y, z) order: cov_ab = (V sum ab - sum a sum b) / V^2 s_a s_b;
      eigenvalues [K, 3] descending (np.linalg.eigvalsh, clamped at 0); axis_lengths = 2 sqrt(5 l): the full axes of the solid ellipsoid with the
      same second moments; principal_axis [K, 3] = the unit eigenvector of l1 in (x, y, z), its sign chosen so that the component of largest
      magnitude is positive (meaningful only where l1 is separated from l2);
      surface_area = fz sy sx + fy sz sx + fx sz sy, contact_area the same on (cz, cy, cx).  This is the CRACK area, the sum of the exposed voxel
      faces: it overestimates the area of a smooth surface (by up to 3 / 2 for a sphere on an isotropic grid), as the 2-D crack length
      overestimates a perimeter;
      mean, std (population), min, max per channel [K, C] with an image.
    Absent ids give NaN.  Equality with scikit-image's regionprops is neither claimed nor tested."""
    try:
        sz, sy, sx = (float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"derive3d: spacing must be a triple (sz, sy, sx) of positive reals, got {spacing!r}") from None
    if not all(math.isfinite(v) and v > 0 for v in (sz, sy, sx)):
        raise ValueError(f"derive3d: spacing must be a triple (sz, sy, sx) of positive reals, got {spacing!r}")
    s = (sx, sy, sz)
    vox = _host(table.voxels).astype(np.int64)
    mom = _host(table.moments).astype(np.int64)
    surf = _host(table.surface).astype(np.int64)
    k = len(vox)
    nan = lambda *shape: np.full(shape, np.nan, np.float64)
    out = {"volume": nan(k), "centroid": nan(k, 3), "equivalent_diameter": nan(k), "covariance": nan(k, 3, 3), "eigenvalues": nan(k, 3),
           "axis_lengths": nan(k, 3), "principal_axis": nan(k, 3), "surface_area": nan(k), "contact_area": nan(k)}
    has_img = table.isum is not None
    if has_img:
        isum, isum2 = _host(table.isum).astype(np.int64), _host(table.isum2).astype(np.int64)
        imin, imax = _host(table.imin), _host(table.imax)
        c = isum.shape[1]
        out.update(mean=nan(k, c), std=nan(k, c), min=nan(k, c), max=nan(k, c))
    second = ((3, 6, 7), (6, 4, 8), (7, 8, 5))            # the column of sum ab in `moments`, (a, b) over (x, y, z)
    for i in range(k):
        v = int(vox[i])
        if v == 0:
            continue
        m = [int(t) for t in mom[i]]
        out["volume"][i] = v * sz * sy * sx
        out["centroid"][i] = [m[a] / v * s[a] for a in range(3)]
        out["equivalent_diameter"][i] = (6 * out["volume"][i] / math.pi) ** (1.0 / 3.0)
        cov = np.array([[(v * m[second[a][b]] - m[a] * m[b]) / (v * v) * s[a] * s[b] for b in range(3)] for a in range(3)], np.float64)
        out["covariance"][i] = cov
        out["eigenvalues"][i] = np.maximum(np.linalg.eigvalsh(cov)[::-1], 0.0)
        out["axis_lengths"][i] = 2.0 * np.sqrt(5.0 * out["eigenvalues"][i])
        axis = np.linalg.eigh(cov)[1][:, 2]
        axis = axis / np.linalg.norm(axis)
        out["principal_axis"][i] = -axis if axis[int(np.argmax(np.abs(axis)))] < 0 else axis
        fz, fy, fx, cz, cy, cx = (int(t) for t in surf[i, 1:])
        out["surface_area"][i] = fz * sy * sx + fy * sz * sx + fx * sz * sy
        out["contact_area"][i] = cz * sy * sx + cy * sz * sx + cx * sz * sy
        if has_img:
            for j in range(c):
                t1, t2 = int(isum[i, j]), int(isum2[i, j])
                out["mean"][i, j] = t1 / v
                out["std"][i, j] = math.sqrt((v * t2 - t1 * t1) / (v * v))
                out["min"][i, j] = float(imin[i, j])
                out["max"][i, j] = float(imax[i, j])
    return out
