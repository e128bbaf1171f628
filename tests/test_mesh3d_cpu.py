"""Surface meshes and Euler numbers of label volumes, the numpy route of utils.mesh3d: against the per-voxel loops of tests/mesh3d_ref.py, against
identities of its own output (closed surfaces, the edges that carry four quads, the divergence theorem, measure_objects' face counts, the volume
rebuilt from the faces), named shapes, only=, the OBJ and napari exits, limits, and the ABI.  Integer work: every assertion is equality."""
import io
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest
import torch

from tests import mesh3d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [name for name, _, _ in R.cases()]
IDENTITY_CASES = [n for n in CASES if "random" in n or "contact" in n or "wall" in n or "six sides" in n or n.startswith("blobs seed 1")]


def _case(name):
    return next((vol, k) for n, vol, k in R.cases() if n == name)


@pytest.mark.parametrize("name", CASES)
def test_numpy_route_equals_the_loops(name):
    from ullsam_amd.utils import mesh3d as M
    vol, k = _case(name)
    got, want = M.label_surfaces(vol, num=k), R.mesh(vol, k)
    assert [str(getattr(got, n).dtype) for n in got._fields] == ["torch.int32", "torch.int32", "torch.int64", "torch.int64", "torch.int64"]
    assert tuple(got.vertices.shape) == (len(want["vertices"]), 3) and tuple(got.quads.shape) == (len(want["quads"]), 4)
    assert tuple(got.fstart.shape) == tuple(got.vstart.shape) == (k + 1,)
    for n, v in R.as_lists(got).items():
        assert v == want[n], (name, n)
    topo = M.object_topology(vol, num=k)
    euler, pinch = R.topology(vol, k)
    assert topo.euler.dtype == topo.pinch_edges.dtype == torch.int64 and tuple(topo.euler.shape) == tuple(topo.pinch_edges.shape) == (k,)
    assert topo.euler.tolist() == euler and topo.pinch_edges.tolist() == pinch, name
    if name == "4x5x6 random":                             # (not vacuous: pinches exist, and tensors and num=None go the same way)
        assert min(pinch) > 0
        again = M.label_surfaces(torch.from_numpy(vol))
        assert all(torch.equal(a, b) for a, b in zip(again, got))
        assert all(torch.equal(a, b) for a, b in zip(M.object_topology(torch.from_numpy(vol)), topo))


def _edge_counts(quads):
    """Counter of the directed edges (a, b) of a list of quads"""
    c = Counter()
    for q in quads:
        for j in range(4):
            c[(q[j], q[(j + 1) % 4])] += 1
    return c


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_identities_of_the_meshes_own_output(name):
    from ullsam_amd.utils import measure3d as M3
    from ullsam_amd.utils import mesh3d as M
    vol, k = _case(name)
    mesh, topo = M.label_surfaces(vol, num=k), M.object_topology(vol, num=k)
    table = M3.measure_objects(vol, num=k)
    tri = M.triangles(mesh)
    assert tuple(tri.shape) == (2 * len(mesh.quads), 3)
    xyz = mesh.vertices.numpy().astype(np.int64)
    src = mesh.source.numpy()
    for i in range(1, k + 1):
        f0, f1 = int(mesh.fstart[i - 1]), int(mesh.fstart[i])
        quads = mesh.quads[f0:f1].tolist()
        assert all(int(mesh.vstart[i - 1]) <= v < int(mesh.vstart[i]) for q in quads for v in q)
        directed = _edge_counts(quads)
        assert all(directed[(b, a)] == n for (a, b), n in directed.items()), (name, i, "the surface is not closed")
        undirected = Counter()
        for (a, b), n in directed.items():
            undirected[(min(a, b), max(a, b))] += n
        assert set(undirected.values()) <= {2, 4}
        assert sum(1 for n in undirected.values() if n == 4) == int(topo.pinch_edges[i - 1]), (name, i)
        t = xyz[tri[2 * f0:2 * f1].numpy().astype(np.int64)]                         # [2 f, 3 corners, 3]: integer determinants
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        det = (a * np.cross(b, c)).sum(1)
        assert int(det.sum()) == 6 * int(table.voxels[i - 1]), (name, i)
        d = src[f0:f1] % 6
        assert [int(((d == 0) | (d == 1)).sum()), int(((d == 2) | (d == 3)).sum()), int(((d == 4) | (d == 5)).sum())] == table.surface[i - 1, 1:4].tolist()
    # a -x face opens a run of its label along the row, a +x face closes it
    z, h, w = vol.shape
    delta = np.zeros((z * h, w + 1), np.int64)
    lab = np.repeat(np.arange(1, k + 1), np.diff(mesh.fstart.numpy()))
    p, d = src // 6, src % 6
    np.add.at(delta, (p[d == 4] // w, p[d == 4] % w), lab[d == 4])
    np.add.at(delta, (p[d == 5] // w, p[d == 5] % w + 1), -lab[d == 5])
    assert np.array_equal(np.cumsum(delta, 1)[:, :w].reshape(z, h, w), vol), name


def test_topology_of_named_shapes():
    from ullsam_amd.utils import mesh3d as M
    assert [e for _, _, e in R.shapes()] == [1, 2, 0, 2]
    for name, vol, euler in R.shapes():
        topo, mesh = M.object_topology(vol, num=1), M.label_surfaces(vol, num=1)
        assert topo.euler.tolist() == [euler] and topo.pinch_edges.tolist() == [0], name
        assert len(mesh.vertices) - len(mesh.quads) == 2 * euler, name                # E = 2 F on a closed quad surface: chi = V - F = 2 chi(solid)
        assert mesh.vstart.tolist() == [0, len(mesh.vertices)] and mesh.fstart.tolist() == [0, len(mesh.quads)]


def test_only_gives_the_rows_of_the_full_call():
    from ullsam_amd.utils import mesh3d as M
    vol, k = _case("4x5x6 random")
    full = M.label_surfaces(vol, num=k)
    part = M.label_surfaces(vol, num=k, only=[2])
    f0, f1, v0, v1 = int(full.fstart[1]), int(full.fstart[2]), int(full.vstart[1]), int(full.vstart[2])
    assert f1 > f0 and part.fstart.tolist() == [0, 0, f1 - f0, f1 - f0] and part.vstart.tolist() == [0, 0, v1 - v0, v1 - v0]
    assert torch.equal(part.vertices, full.vertices[v0:v1]) and torch.equal(part.quads, full.quads[f0:f1] - v0) and torch.equal(part.source, full.source[f0:f1])
    sv, sq = M.submesh(full, 2)
    assert torch.equal(sv, part.vertices) and torch.equal(sq, part.quads)
    every = M.label_surfaces(vol, num=k, only=torch.tensor([3, 1, 2]))
    assert all(torch.equal(a, b) for a, b in zip(every, full))
    none = M.label_surfaces(vol, num=k, only=[])
    assert none.fstart.tolist() == [0] * (k + 1) and tuple(none.quads.shape) == (0, 4) and tuple(none.vertices.shape) == (0, 3)
    for bad in ([0], [k + 1], [2, 2], [[1, 2]], [-1]):
        with pytest.raises(ValueError):
            M.label_surfaces(vol, num=k, only=bad)
    with pytest.raises(ValueError):
        M.submesh(full, 0)
    with pytest.raises(ValueError):
        M.submesh(full, k + 1)


def _parse_obj(text):
    groups, verts, faces = [], [], []
    for line in text.splitlines():
        tag, *rest = line.split()
        if tag == "o":
            groups.append(rest[0])
        elif tag == "v":
            verts.append([float(v) for v in rest])
        elif tag == "f":
            faces.append([int(v) for v in rest])
        else:
            raise AssertionError(line)
    return groups, verts, faces


def test_obj_and_napari_exits(tmp_path):
    from ullsam_amd.utils import measure3d as M3
    from ullsam_amd.utils import mesh3d as M
    vol, k = _case("an absent id in the middle")
    mesh = M.label_surfaces(vol, num=k)
    out = io.StringIO()
    assert M.to_obj(mesh, out, spacing=(2.5, 1.0, 0.5), origin=(10, 20, 30)) == 2
    groups, verts, faces = _parse_obj(out.getvalue())
    assert groups == ["label_1", "label_3"]                                         # (the absent id 2 has no group)
    assert (np.array(faces) - 1).tolist() == mesh.quads.tolist()
    want = mesh.vertices.numpy().astype(np.float64) * np.array([0.5, 1.0, 2.5]) + np.array([30.0, 20.0, 10.0])
    assert np.array_equal(np.array(verts), want)
    path = tmp_path / "one.obj"
    assert M.to_obj(mesh, path, only=[3]) == 1
    groups, verts, faces = _parse_obj(path.read_text())
    sv, sq = M.submesh(mesh, 3)
    assert groups == ["label_3"] and (np.array(faces) - 1).tolist() == sq.tolist() and np.array_equal(np.array(verts), sv.numpy().astype(np.float64))
    for bad in ((1, 1), (1, 0, 1), "abc", (1, 1, float("nan"))):
        with pytest.raises(ValueError):
            M.to_obj(mesh, io.StringIO(), spacing=bad)
    # napari: (z, y, x), reversed winding, the label as the value; the signed volume under spacing (5, 2, 2) is 20 x voxels
    vertices, tris, values = M.to_napari(mesh, spacing=(5, 2, 2))
    assert vertices.dtype == np.float64 and tris.dtype == np.int64 and values.dtype == np.float32
    assert vertices.shape == (len(mesh.vertices), 3) and tris.shape == (2 * len(mesh.quads), 3) and values.shape == (len(mesh.vertices),)
    assert np.array_equal(vertices, mesh.vertices.numpy()[:, ::-1] * np.array([5.0, 2.0, 2.0]))
    assert np.array_equal(tris, M.triangles(mesh).numpy()[:, ::-1])
    assert values.tolist() == [1.0] * int(mesh.vstart[1]) + [3.0] * int(mesh.vstart[3] - mesh.vstart[2])
    voxels = M3.measure_objects(vol, num=k).voxels.tolist()
    for i in range(1, k + 1):
        t = vertices[tris[2 * int(mesh.fstart[i - 1]):2 * int(mesh.fstart[i])]]
        det = (t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum(1)
        assert det.sum() == 6 * 20 * voxels[i - 1]
    moved = M.to_napari(mesh, origin=(1, 2, 3))[0]
    assert np.array_equal(moved, mesh.vertices.numpy()[:, ::-1] + np.array([1.0, 2.0, 3.0]))


class _Stub:
    def __init__(self, *shape):
        self.shape = shape


def test_limits_and_argument_checks():
    from ullsam_amd import _lib
    from ullsam_amd.utils import mesh3d as M
    for fn in (M.label_surfaces, M.object_topology):
        for shape, number in (((32768, 1, 1), "32768"), ((1, 32768, 1), "32768"), ((1, 1, 32768), "32768"), ((2048, 1024, 1024), str(2 ** 31)),
                              ((0, 4, 4), "0")):
            with pytest.raises(ValueError, match=number):                            # before any voxel is read: the stub has none
                fn(_Stub(*shape))
        for shape in ((4, 4), (1, 2, 3, 4)):
            with pytest.raises(ValueError):
                fn(_Stub(*shape))
    with pytest.raises(ValueError, match=str(2 ** 29)):
        M.label_surfaces(_Stub(4, 4, 4), num=2 ** 29)
    with pytest.raises(ValueError, match="route"):
        M.label_surfaces(_Stub(4, 4, 4), num=3, route="staged")
    with pytest.raises(ValueError, match="id 4"):
        M.label_surfaces(_Stub(4, 4, 4), num=3, only=[4])
    with pytest.raises(ValueError, match="id 2 more than once"):
        M.label_surfaces(_Stub(4, 4, 4), num=3, only=[2, 1, 2])
    for fn in (M.label_surfaces, M.object_topology):
        with pytest.raises(_lib.UllsamError):
            fn(_Stub(4, 4, 4), num=-1)
    vol = np.zeros((3, 6, 8), np.int32)
    vol[1, 2:4, 2:5] = 1
    for bad in (2, -7, 2 ** 31 - 1):                                                 # an id outside 0..K, then a good call
        b = vol.copy()
        b[1, 3, 3] = bad
        with pytest.raises(_lib.UllsamError):
            M.label_surfaces(b, num=1)
        with pytest.raises(_lib.UllsamError):
            M.object_topology(b, num=1)
    assert M.label_surfaces(vol, num=1).fstart.tolist() == [0, 2 * (6 + 3 + 2)] and M.object_topology(vol, num=1).euler.tolist() == [1]
    empty = M.label_surfaces(np.zeros((2, 2, 2), np.int32))                          # K = 0
    assert empty.fstart.tolist() == [0] and empty.vstart.tolist() == [0] and tuple(empty.quads.shape) == (0, 4) and tuple(empty.source.shape) == (0,)
    assert tuple(M.object_topology(np.zeros((2, 2, 2), np.int32)).euler.shape) == (0,)


# ---- ABI and resources -------------------------------------------------------------------------------------------------------------------------------
NAMES = ["ullsam_mesh3d_masks", "ullsam_mesh3d_faces", "ullsam_mesh3d_corners", "ullsam_mesh3d_heads", "ullsam_mesh3d_vertices", "ullsam_mesh3d_quads",
         "ullsam_mesh3d_starts", "ullsam_mesh3d_topology"]


def test_abi_symbols_and_constants():
    from ullsam_amd import _lib, build, ops
    from ullsam_amd.utils import mesh3d as M
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert _lib.ABI_VERSION == 14 == lib.ullsam_abi_version() == int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1))
    tree = open(os.path.join(ROOT, "ullsam_amd", "ops.py")).read()
    for s in NAMES:
        assert s in _lib.SIGNATURES and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr) and '"%s"' % s in tree, s
        assert hasattr(ops, s.replace("ullsam_", "")), s
    src = open(os.path.join(ROOT, "ullsam_amd", "csrc", "mesh3d.hip")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert define("MS_TILE_X") == ops.MESH3D_TILE_X == 64 and define("MS_TILE_Y") == ops.MESH3D_TILE_Y and define("MS_TILE_Z") == ops.MESH3D_TILE_Z
    assert define("MS_MAX_SIDE") == 32767 and define("MS_KEY_SHIFT") == ops.MESH3D_KEY_SHIFT == M.KEY_SHIFT == 34
    assert define("MS_MAX_LABEL") == ops.MESH3D_MAX_LABEL == M.MAX_LABEL == 2 ** 29 - 1 and 256 * define("MS_ITEMS") == ops.MESH3D_BLOCK_KEYS
    assert 6 * (2 ** 31 - 1) < 2 ** 34 and 3 * 32768 ** 2 < 2 ** 34 and ((2 ** 29 - 1) << 34 | (2 ** 34 - 1)) == 2 ** 63 - 1
    assert not re.search(r"\b(float|double)\b", re.sub(r"//[^\n]*", "", src))         # integer work only
    # the corner table of the kernels is the table of the definition
    quad = re.findall(r"MS_Q\(MS_C\((\d), (\d), (\d)\), MS_C\((\d), (\d), (\d)\), MS_C\((\d), (\d), (\d)\), MS_C\((\d), (\d), (\d)\)\)", src)
    assert [[[int(v) for v in q[3 * j:3 * j + 3]] for j in range(4)] for q in quad] == M.CORNERS.tolist() == [[list(c) for c in q] for q in R.QUAD]


def test_mesh3d_kernels_have_no_spill_and_no_scratch():
    from ullsam_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    assert not any(pat in KR.HOT_BF16 for pat in KR.HOT_MESH3D)                      # a list of its own, in no aggregate
    ks = {n: r for n, r in KR.kernels().items() if any(re.search(h, n) for h in KR.HOT_MESH3D)}
    assert len(ks) == len(KR.HOT_MESH3D) + 1, sorted(ks)                             # the heads kernel in two forms: counting and writing
    assert all("mesh3d_" in n for n in ks) and not any(re.search(h, n) for n in ks for h in KR.HOT_BF16)
    for n, r in ks.items():
        assert not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0) and not r.get("private_segment_fixed_size", 0), (n, r)
        assert r.get("group_segment_fixed_size", 0) <= 128, n                        # (the scans' per-wave totals)
