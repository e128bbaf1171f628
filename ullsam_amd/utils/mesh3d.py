"""Surface meshes and Euler numbers of a label VOLUME -- the exit of the 3-D chain (link_label_stack, inner_distance3d / expand_labels3d /
shrink_labels3d, split_labels3d, measure_objects) to vector tools, as label_outlines / simplify_outlines / to_geojson are for label images: the
cuberille surface of every object as quads over shared vertices, and the one topological number of a region table.  This module is the definition
(vectorised numpy on int64, integers only) and the driver of the device route (csrc/mesh3d.hip); the two are equal bit for bit
(tests/test_mesh3d_*.py).  DESIGN.md "7b, continued (3-D surfaces)" states the definitions, the identities, the bounds and what is out of scope.

    volume = link_label_stack(planes, counts, device="cuda")[0]                # int32 [Z, H, W] on the device
    mesh = label_surfaces(volume)                                              # SurfaceMesh of tensors, on the device where the volume is
    topo = object_topology(volume)                                             # Topology(euler, pinch_edges), int64 [K] each
    to_obj(mesh, "nuclei.obj", spacing=(2.5, 1.0, 1.0))                        # one "o label_<k>" group per object
    vertices, faces, values = to_napari(mesh, spacing=(2.5, 1.0, 1.0))         # viewer.add_surface((vertices, faces, values))

volume int32 [Z, H, W] with ids 0..K, 0 = background.  Limits (ValueError stating the number, before any voxel is read): 1 <= Z, H, W <= 32767,
Z * H * W <= 2^31 - 1 and, for label_surfaces, K <= 2^29 - 1.  An id outside 0..K raises UllsamError.

Voxel (z, y, x) is the cube [x, x + 1] x [y, y + 1] x [z, z + 1] with raster index p = (z H + y) W + x; lattice corner (cx, cy, cz) has the id
c = (cz (H + 1) + cy) (W + 1) + cx.  Directions d: 0 = -z, 1 = +z, 2 = -y, 3 = +y, 4 = -x, 5 = +x.  Face (p, d) exists when voxel p has an id k > 0
and its neighbour towards d is not k (the volume's outside is not k: measure_objects' f_a); its id is 6 p + d.
Bounds: 6 p + d < 6 * 2^31 < 2^34; c < (Z + 1) (H + 1) (W + 1) <= 8 Z H W < 2^34; a key id | label << 34 with label < 2^29 stays below 2^63.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from .distance import _route
from .measure import _check_ids, _host, _num
from .measure3d import _check_volume

KEY_SHIFT = 34
ID_MASK = (1 << KEY_SHIFT) - 1
MAX_LABEL = 2 ** 29 - 1
INT_MAX = 2 ** 31 - 1
ROUTES = ("global",)
# the neighbour (dz, dy, dx) towards d
OFFSETS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
# the quad towards d: offsets (dx, dy, dz) from the voxel's corner (x, y, z), counter-clockwise seen from outside in the right-handed frame (x, y, z)
CORNERS = np.array([[(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)], [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],
                    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],
                    [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)], [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)]], np.int64)


class SurfaceMesh(NamedTuple):
    """vertices int32 [V, 3] = (x, y, z) lattice corners, the distinct pairs (label, corner id) ordered by them -- a corner used by two objects is
    two vertices, a corner used twice by one object is one; quads int32 [F, 4] = global vertex indices, counter-clockwise seen from outside, the
    faces ordered by (label, face id); source int64 [F] = the face id 6 p + d: the voxel and the side a face came from; fstart / vstart int64
    [K + 1]: label k owns quads[fstart[k - 1] : fstart[k]] and vertices[vstart[k - 1] : vstart[k]]."""
    vertices: torch.Tensor
    quads: torch.Tensor
    source: torch.Tensor
    fstart: torch.Tensor
    vstart: torch.Tensor


class Topology(NamedTuple):
    """euler, pinch_edges int64 [K]; row k - 1 belongs to id k, 0 for an absent id."""
    euler: torch.Tensor
    pinch_edges: torch.Tensor


def _label_count(volume, num, what: str, most: int) -> Optional[int]:
    """num checked before the volume is touched (None: not given)."""
    if num is None:
        return None
    k = _num(volume, num)
    if k > most:
        raise ValueError(f"{what}: num = {k} ids (at most 2^29 - 1 = {most}: a key holds the label above bit 34)")
    return k


def _only_ids(only, k: int) -> np.ndarray:
    ids = np.asarray(_host(only))
    if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
        raise ValueError(f"label_surfaces: only must be a 1-D list or tensor of integer ids, got shape {ids.shape} of {ids.dtype}")
    ids = ids.astype(np.int64)
    for i in ids.tolist():
        if not 1 <= i <= k:
            raise ValueError(f"label_surfaces: only names the id {i} outside 1..{k}")
    if len(np.unique(ids)) != len(ids):
        dup = sorted(i for i in set(ids.tolist()) if (ids == i).sum() > 1)
        raise ValueError(f"label_surfaces: only names the id {dup[0]} more than once")
    return ids


def _surfaces_host(vol: np.ndarray, k: int, ids: Optional[np.ndarray]):
    _check_ids(vol, k, "label_surfaces")
    z, h, w = vol.shape
    pad = np.full((z + 2, h + 2, w + 2), -1, np.int32)    # -1: the volume's outside is "not k"
    pad[1:-1, 1:-1, 1:-1] = vol
    on = vol > 0
    if ids is not None:
        sel = np.zeros(k + 1, bool)
        sel[ids] = True
        on &= sel[vol]
    flat, keys = vol.reshape(-1), []
    for d, (oz, oy, ox) in enumerate(OFFSETS):
        p = np.flatnonzero(on & (pad[1 + oz:1 + oz + z, 1 + oy:1 + oy + h, 1 + ox:1 + ox + w] != vol))
        keys.append((flat[p].astype(np.int64) << KEY_SHIFT) | (6 * p + d))
    fkeys = np.sort(np.concatenate(keys))
    if len(fkeys) > INT_MAX:
        raise _lib.UllsamError(f"label_surfaces: {len(fkeys)} faces (at most 2^31 - 1)")
    lab, fid = fkeys >> KEY_SHIFT, fkeys & ID_MASK
    p, d = fid // 6, fid % 6
    off = CORNERS[d]                                      # [F, 4, 3]
    cx, cy, cz = (p % w)[:, None] + off[..., 0], ((p // w) % h)[:, None] + off[..., 1], (p // (w * h))[:, None] + off[..., 2]
    ckeys = (lab[:, None] << KEY_SHIFT) | ((cz * (h + 1) + cy) * (w + 1) + cx)
    ukeys, inv = np.unique(ckeys.reshape(-1), return_inverse=True)
    if len(ukeys) > INT_MAX:
        raise _lib.UllsamError(f"label_surfaces: {len(ukeys)} vertices (at most 2^31 - 1)")
    c = ukeys & ID_MASK
    every = np.arange(k + 1, dtype=np.int64)
    return {"vertices": np.stack([c % (w + 1), (c // (w + 1)) % (h + 1), c // ((w + 1) * (h + 1))], 1).astype(np.int32).reshape(-1, 3),
            "quads": inv.reshape(-1, 4).astype(np.int32), "source": fid.astype(np.int64),
            "fstart": np.searchsorted(lab, every, "right").astype(np.int64), "vstart": np.searchsorted(ukeys >> KEY_SHIFT, every, "right").astype(np.int64)}


def label_surfaces(volume, num=None, only=None, device=None, route=None) -> SurfaceMesh:
    """The cuberille surface of every object of a label volume: each exposed voxel face (the module's text) is a quad whose corners are the table
    CORNERS, counter-clockwise seen from outside, over vertices shared per object.  Where two voxels of an object meet only along an edge or at a
    corner the mesh is pinched there and not manifold (the stance of connectivity=8 in label_outlines); object_topology counts those edges.  Per
    object the surface is closed (every directed quad edge meets its reverse) and sum det(v0, v1, v2) over triangles(mesh) is 6 x its voxels.
    volume: numpy, a CPU tensor or a device tensor; num = K (default volume.max(): one read-back on the device route), at most 2^29 - 1.
    only: None, or a 1-D list / tensor of distinct ids in 1..K (ValueError otherwise): faces of other ids are not produced, their rows are empty.
    device None: where the volume is (numpy, CPU tensor: this definition in numpy; a GPU tensor: csrc/mesh3d.hip on the volume where it is);
    "cpu" / a GPU device: that route.  The device route leaves its outputs on the device and reads back the two counts F and V and one status word;
    torch.sort orders the face keys and the corner keys.  route (device only): None or "global", the one route there is -- a voxel's six neighbours
    are read from global memory; a form that staged a workgroup's tile and its halo in LDS was measured against it, did not win and was taken out
    (profiles/r26_mesh3d.txt).
    More than 2^31 - 1 faces or vertices and an id outside 0..K raise UllsamError."""
    z, h, w = _check_volume(volume, "label_surfaces")
    if route is not None and route not in ROUTES:
        raise ValueError(f"label_surfaces: route must be None or 'global', got {route!r}")
    k = _label_count(volume, num, "label_surfaces", MAX_LABEL)
    ids = None if only is None or k is None else _only_ids(only, k)
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host(volume).astype(np.int32, copy=False)
        if k is None:
            k = _label_count(vol, _num(vol, None), "label_surfaces", MAX_LABEL)
            ids = None if only is None else _only_ids(only, k)
        return SurfaceMesh(**{name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in _surfaces_host(vol, k, ids).items()})
    from .. import ops
    vol = torch.as_tensor(volume).to(device=dev, dtype=torch.int32).contiguous()
    if k is None:
        k = _label_count(vol, _num(vol, None), "label_surfaces", MAX_LABEL)
        ids = None if only is None else _only_ids(only, k)
    sel = None
    if ids is not None:
        sel = torch.zeros((k + 1,), dtype=torch.uint8, device=dev)
        sel[torch.from_numpy(ids).to(dev)] = 1
    masks, tile_offsets, flags = ops.mesh3d_masks(vol, k, sel)
    nf = int(tile_offsets[-1])                            # read-back: F
    if int(flags.cpu()[0]):                               # read-back: the status word
        raise _lib.UllsamError(f"label_surfaces: the label volume holds an id outside 0..{k}")
    if nf > INT_MAX:
        raise _lib.UllsamError(f"label_surfaces: {nf} faces (at most 2^31 - 1)")
    fkeys = torch.sort(ops.mesh3d_faces(vol, masks, tile_offsets, nf)).values
    del masks
    corners = torch.sort(ops.mesh3d_corners(fkeys, h, w)).values
    block_offsets = ops.mesh3d_heads(corners)
    nv = int(block_offsets[-1])                           # read-back: V
    if nv > INT_MAX:
        raise _lib.UllsamError(f"label_surfaces: {nv} vertices (at most 2^31 - 1)")
    ukeys, vertices = ops.mesh3d_vertices(corners, block_offsets, nv, h, w)
    del corners
    return SurfaceMesh(vertices, ops.mesh3d_quads(fkeys, ukeys, h, w), fkeys & ID_MASK, ops.mesh3d_starts(fkeys, k), ops.mesh3d_starts(ukeys, k))


def _topology_host(vol: np.ndarray, k: int):
    _check_ids(vol, k, "object_topology")
    n = vol.shape
    pad = np.zeros(tuple(v + 2 for v in n), np.int64)     # 0: the volume's outside is no object
    pad[1:-1, 1:-1, 1:-1] = vol

    def around(kind):
        """kind[a] = 0: the lattice cell extends along axis a (one voxel position), 1: it sits between two voxel positions -> the ids of the voxels
        around every such cell, [2^(number of 1s), cells...]"""
        out = []
        for o in np.ndindex(*(2 if t else 1 for t in kind)):
            out.append(pad[tuple(slice(o[a], o[a] + n[a] + 1) if kind[a] else slice(1, n[a] + 1) for a in range(3))])
        return np.stack(out)

    euler = np.zeros(k, np.int64)
    for kind in np.ndindex(2, 2, 2):                      # corners (1, 1, 1), edges, faces, the voxels (0, 0, 0)
        s = np.sort(around(kind), axis=0)
        first = np.ones(s.shape, bool)
        first[1:] = s[1:] != s[:-1]                       # every id once per cell it touches
        count = np.bincount(s[first & (s > 0)], minlength=k + 1)[1:].astype(np.int64)
        euler += count if sum(kind) % 2 else -count       # dimension 3 - sum(kind): corners and faces +, edges and voxels -
    pinch = np.zeros(k, np.int64)
    for kind in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):        # the edges along z, y, x
        a, b, d, c = around(kind)                         # (0, 0), (0, 1), (1, 0), (1, 1): a - b - c - d goes round the edge
        for p, q, r, s in ((a, b, c, d), (b, c, d, a)):
            pinch += np.bincount(p[(p > 0) & (p == r) & (q != p) & (s != p)], minlength=k + 1)[1:]
    return euler, pinch


def object_topology(volume, num=None, device=None) -> Topology:
    """euler[k - 1]: with m = the union of the closed voxel cubes of id k (26-connectivity), V - E + F - C of the cubical complex of m: V = the
    lattice corners touched by a voxel of k (any of the 8 around the corner), E = the lattice edges touched (any of 4), F = the lattice faces
    touched (any of 2), C = the voxels.  That is components - tunnels + cavities: 1 for a solid ball, 2 for a hollow one, 0 for a ring.
    pinch_edges[k - 1]: the lattice edges whose four voxels are k, not k, k, not k around the edge (the outside is not k) -- exactly the edges of
    label_surfaces' mesh that carry four quads of k instead of two.  volume, num, device as in label_surfaces (num up to 2^31 - 2); the device
    route (one pass of csrc/mesh3d.hip with integer atomics) leaves both tables on the device and reads back one status word."""
    _check_volume(volume, "object_topology")
    k = None if num is None else _num(volume, num)
    dev = _route(volume, device)
    if dev.type != "cuda":
        vol = _host(volume).astype(np.int32, copy=False)
        return Topology(*(torch.from_numpy(np.ascontiguousarray(v)) for v in _topology_host(vol, _num(vol, k))))
    from .. import ops
    vol = torch.as_tensor(volume).to(device=dev, dtype=torch.int32).contiguous()
    k = _num(vol, k)
    euler, pinch, flags = ops.mesh3d_topology(vol, k)
    if int(flags.cpu()[0]):
        raise _lib.UllsamError(f"object_topology: the label volume holds an id outside 0..{k}")
    return Topology(euler, pinch)


# ---- exits -------------------------------------------------------------------------------------------------------------------------------------
def triangles(mesh: SurfaceMesh) -> torch.Tensor:
    """[2 F, 3]: quad q as (q0, q1, q2), (q0, q2, q3), face-major; the dtype and the place of mesh.quads."""
    q = mesh.quads
    return torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)


def _label_of(mesh: SurfaceMesh, k) -> int:
    n, k = len(mesh.fstart) - 1, int(k)
    if not 1 <= k <= n:
        raise ValueError(f"the mesh has the ids 1..{n}, got {k}")
    return k


def submesh(mesh: SurfaceMesh, k: int):
    """(vertices [v, 3], quads [f, 4]) of the one id k, the quads in indices local to these vertices."""
    k = _label_of(mesh, k)
    f0, f1, v0, v1 = (int(t) for t in (mesh.fstart[k - 1], mesh.fstart[k], mesh.vstart[k - 1], mesh.vstart[k]))
    return mesh.vertices[v0:v1], mesh.quads[f0:f1] - v0


def _triple(v, name: str, positive: bool):
    try:
        out = tuple(float(t) for t in v)
    except (TypeError, ValueError):
        out = ()
    if len(out) != 3 or not all(np.isfinite(t) and (t > 0 or not positive) for t in out):
        raise ValueError(f"{name} must be a triple (z, y, x) of {'positive ' if positive else ''}reals, got {v!r}")
    return out


def _world(vertices: np.ndarray, spacing, origin) -> np.ndarray:
    """float64 [V, 3] in (x, y, z): origin + spacing x corner, per axis"""
    sz, sy, sx = _triple(spacing, "spacing", True)
    oz, oy, ox = _triple(origin, "origin", False)
    v = vertices.astype(np.float64)
    return np.stack([ox + sx * v[:, 0], oy + sy * v[:, 1], oz + sz * v[:, 2]], 1).reshape(-1, 3)


def to_obj(mesh: SurfaceMesh, file_or_path, spacing=(1, 1, 1), origin=(0, 0, 0), only=None) -> int:
    """Wavefront OBJ: per present id k (of `only`, when given) a group "o label_<k>", its "v x y z" lines with x = origin_x + sx cx, y and z
    alike (spacing = (sz, sy, sx) and origin = (oz, oy, ox), as elsewhere in the 3-D chain; float64, printed with repr), and its quads as "f" lines
    of four 1-based indices into the file's vertices.  file_or_path: a path or an object with write().  -> the number of groups written."""
    vs, fs = _host(mesh.vstart), _host(mesh.fstart)
    xyz = _world(_host(mesh.vertices), spacing, origin)
    quads = _host(mesh.quads).astype(np.int64)
    ids = range(1, len(fs)) if only is None else [_label_of(mesh, k) for k in only]
    lines, base, groups = [], 0, 0
    for k in ids:
        f0, f1, v0, v1 = int(fs[k - 1]), int(fs[k]), int(vs[k - 1]), int(vs[k])
        if f1 == f0:
            continue
        lines.append(f"o label_{k}")
        lines.extend(f"v {x!r} {y!r} {z!r}" for x, y, z in xyz[v0:v1].tolist())
        lines.extend("f %d %d %d %d" % tuple(q) for q in (quads[f0:f1] - v0 + base + 1).tolist())
        base += v1 - v0
        groups += 1
    text = "\n".join(lines) + ("\n" if lines else "")
    if isinstance(file_or_path, (str, os.PathLike)):
        with open(file_or_path, "w") as f:
            f.write(text)
    else:
        file_or_path.write(text)
    return groups


def to_napari(mesh: SurfaceMesh, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """(vertices float64 [V, 3] in napari's (z, y, x) order, faces int64 [2 F, 3], values float32 [V] = the vertex's label) for
    viewer.add_surface.  Every triangle of triangles(mesh) is reversed: swapping the x and z axes mirrors space, so the normals point outward
    again.  spacing and origin as in to_obj."""
    xyz = _world(_host(mesh.vertices), spacing, origin)
    faces = _host(triangles(mesh)).astype(np.int64)[:, ::-1]
    vs = _host(mesh.vstart).astype(np.int64)
    values = np.repeat(np.arange(1, len(vs), dtype=np.float32), np.diff(vs))
    return np.ascontiguousarray(xyz[:, ::-1]), np.ascontiguousarray(faces), values
