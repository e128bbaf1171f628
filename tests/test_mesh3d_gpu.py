"""Surface meshes and Euler numbers of label volumes on the GPU (csrc/mesh3d.hip through utils.mesh3d.label_surfaces / object_topology): the device
route against the numpy route (itself checked against per-voxel loops in tests/test_mesh3d_cpu.py) field by field, with only=, host inputs, views
inside guarded buffers, the status word, the named shapes and a linked stack that never leaves the device.  Integer work: every assertion is
equality."""
import numpy as np
import pytest
import torch

from tests import distance3d_ref as R3
from tests import mesh3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUTES = ("global",)                                                                # (the staged form lost its A/B and was taken out)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _whole_rows():
    """3 x 5 x 300: one run per row across the 64-column tile seams, the 64-voxel segments of the topology kernel, and whole rows."""
    vol = np.zeros((3, 5, 300), np.int32)
    runs = [(193, 63), (192, 64), (192, 65), (128, 130), (224, 64), (126, 130), (0, 63), (0, 64), (0, 65), (0, 130), (0, 300), (64, 192), (191, 66),
            (255, 2), (170, 130)]
    for i, (x0, n) in enumerate(runs):
        vol[i // 5, i % 5, x0:x0 + n] = 1 + i % 4
    return vol


def _volumes():
    from ullsam_amd import ops
    rng = np.random.default_rng(2)
    ty, tz, tx = ops.MESH3D_TILE_Y, ops.MESH3D_TILE_Z, ops.MESH3D_TILE_X
    tiles = R3.blobs(11, 2 * tz + 1, 2 * ty + 3, tx + 36, n=40, ids=40)              # three tiles along z, three along y, two along x
    assert len(np.unique(tiles)) - 1 < 40                                            # (ids up to 40, at least one absent)
    return {
        "1x1x1": (np.array([[[1]]], np.int32), 1),
        "1x1x200 runs of 5": (np.repeat(rng.integers(0, 6, 40), 5).astype(np.int32).reshape(1, 1, 200), 6),
        "3x5x300 whole-row runs": (_whole_rows(), 5),
        "tiles along z, y and x": (tiles, 40),
        "edge-only contact": (R.contact("edge"), 1),
        "corner-only contact": (R.contact("corner"), 1),
        "one object filling the volume": (np.ones((5, 6, 70), np.int32), 1),
        "4x5x6 random": next((vol, k) for n, vol, k in R.cases() if n == "4x5x6 random"),
    }


NAMES = ["1x1x1", "1x1x200 runs of 5", "3x5x300 whole-row runs", "tiles along z, y and x", "edge-only contact", "corner-only contact",
         "one object filling the volume", "4x5x6 random"]
VOLUMES, WANT = None, {}


def _get(name):
    """(volume, K, the numpy route's mesh, the numpy route's topology), computed once"""
    global VOLUMES
    from ullsam_amd.utils import mesh3d as M
    if VOLUMES is None:
        VOLUMES = _volumes()
    vol, k = VOLUMES[name]
    if name not in WANT:
        WANT[name] = (M.label_surfaces(vol, num=k), M.object_topology(vol, num=k))
    return (vol, k) + WANT[name]


def _same(got, want, what):
    assert type(got) is type(want), what
    for n in got._fields:
        g, w_ = getattr(got, n), getattr(want, n)
        assert g.is_cuda and g.dtype == w_.dtype and tuple(g.shape) == tuple(w_.shape) and torch.equal(g.cpu(), w_), (what, n)


@pytest.mark.parametrize("name", NAMES)
def test_device_route_equals_the_numpy_route(name):
    from ullsam_amd.utils import mesh3d as M
    vol, k, mesh, topo = _get(name)
    vol_d = T(vol)
    for route in ROUTES + (None,):
        got = M.label_surfaces(vol_d, num=k, route=route)
        _same(got, mesh, (name, route))
        again = M.label_surfaces(vol_d, num=k, route=route)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), (name, route, "two runs differ")
    got = M.object_topology(vol_d, num=k)
    _same(got, topo, name)
    assert all(torch.equal(a, b) for a, b in zip(got, M.object_topology(vol_d, num=k))), (name, "two runs differ")
    # host input sent to the device, num left to volume.max()
    _same(M.label_surfaces(vol, device=DEV), M.label_surfaces(vol), (name, "host input"))
    _same(M.object_topology(vol, device=DEV), M.object_topology(vol), (name, "host input"))
    if name == "one object filling the volume":                                      # every face lies on the volume's border
        z, h, w = vol.shape
        assert len(mesh.quads) == 2 * (z * h + z * w + h * w) and topo.euler.tolist() == [1]


def test_only_with_one_id_all_ids_and_an_absent_id():
    from ullsam_amd.utils import mesh3d as M
    vol, k, mesh, _ = _get("tiles along z, y and x")
    present = np.unique(vol[vol > 0]).tolist()
    absent = next(i for i in range(1, k + 1) if i not in present)
    vol_d = T(vol)
    for route in ROUTES:
        for only in ([present[3]], list(range(1, k + 1)), [absent], torch.tensor([present[0], absent, present[-1]], device=DEV)):
            _same(M.label_surfaces(vol_d, num=k, only=only, route=route), M.label_surfaces(vol, num=k, only=only.cpu() if torch.is_tensor(only) else only),
                  (route, only))
    _same(M.label_surfaces(vol_d, num=k, only=list(range(1, k + 1))), mesh, "all ids")
    assert len(M.label_surfaces(vol_d, num=k, only=[absent]).quads) == 0
    with pytest.raises(ValueError):
        M.label_surfaces(vol_d, num=k, only=[k + 1])


def test_views_inside_guarded_buffers_and_a_view_with_strides():
    """The volume 4 bytes off a 16-byte boundary with ids around it that would make faces disappear if they were read as neighbours; the topology
    tables as views inside guarded buffers; a non-contiguous view of a larger volume."""
    from ullsam_amd import ops
    from ullsam_amd.utils import mesh3d as M
    vol, k, mesh, topo = _get("tiles along z, y and x")
    pad, guard = 64, -123456789
    first = int(vol.reshape(-1)[0]) or 1
    vbuf = np.full((pad + vol.size + pad,), first, np.int32)
    vbuf[pad + 1:pad + 1 + vol.size] = vol.reshape(-1)
    buf_d = T(vbuf)
    vol_d = buf_d[pad + 1:pad + 1 + vol.size].view(vol.shape)
    assert vol_d.data_ptr() % 16 == 4
    for route in ROUTES:
        _same(M.label_surfaces(vol_d, num=k, route=route), mesh, route)
    assert np.array_equal(buf_d.cpu().numpy(), vbuf)                                 # the volume and its surroundings are only read
    bufs = {n: torch.full((pad + k + pad,), guard, dtype=torch.int64, device=DEV) for n in ("euler", "pinch_edges")}
    out = {n: b[pad + 1:pad + 1 + k] for n, b in bufs.items()}
    fbuf = torch.full((pad + ops.MEASURE_FLAGS + pad,), guard, dtype=torch.int32, device=DEV)
    euler, pinch, flags = ops.mesh3d_topology(vol_d, k, out=out, flags=fbuf[pad:pad + ops.MEASURE_FLAGS])
    assert euler.data_ptr() == out["euler"].data_ptr() and flags.cpu().tolist()[0] == 0
    assert torch.equal(euler.cpu(), topo.euler) and torch.equal(pinch.cpu(), topo.pinch_edges)
    for b in bufs.values():
        assert bool((b[:pad + 1] == guard).all()) and bool((b[pad + 1 + k:] == guard).all())
    assert bool((fbuf[:pad] == guard).all()) and bool((fbuf[pad + ops.MEASURE_FLAGS:] == guard).all())
    big = np.zeros(tuple(2 * n for n in vol.shape), np.int32)
    big[::2, ::2, ::2] = vol
    view = T(big)[::2, ::2, ::2]
    assert not view.is_contiguous()
    _same(M.label_surfaces(view, num=k), mesh, "strided view")
    _same(M.object_topology(view, num=k), topo, "strided view")


def test_ids_outside_the_range_raise_and_the_next_call_is_correct():
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import mesh3d as M
    vol, k, mesh, topo = _get("tiles along z, y and x")
    where = (4, 9, 50)
    clean = vol.copy()
    clean[where] = 0                                                                 # a bad id reads as background
    want = M.object_topology(clean, num=k)
    for value in (k + 1, -1):
        bad = vol.copy()
        bad[where] = value
        for route in ROUTES:
            with pytest.raises(_lib.UllsamError):
                M.label_surfaces(T(bad), num=k, route=route)
        with pytest.raises(_lib.UllsamError):
            M.object_topology(T(bad), num=k)
        euler, pinch, flags = ops.mesh3d_topology(T(bad), k)
        assert flags.cpu().tolist()[0] == 1 and torch.equal(euler.cpu(), want.euler) and torch.equal(pinch.cpu(), want.pinch_edges)
        masks, offsets, flags = ops.mesh3d_masks(T(bad), k)
        assert flags.cpu().tolist()[0] == 1 and int(offsets[-1]) == len(M.label_surfaces(clean, num=k).quads)
        _same(M.label_surfaces(T(vol), num=k), mesh, value)                           # the next call is correct
        _same(M.object_topology(T(vol), num=k), topo, value)
    with pytest.raises(ValueError, match=str(2 ** 29)):
        M.label_surfaces(T(vol), num=2 ** 29)
    with pytest.raises(_lib.UllsamError):
        ops.mesh3d_masks(T(vol), 2 ** 29)
    with pytest.raises(_lib.UllsamError):
        ops.mesh3d_topology(torch.zeros((32768, 1, 1), dtype=torch.int32, device=DEV), 0)


def test_topology_of_named_shapes():
    from ullsam_amd.utils import mesh3d as M
    for name, vol, euler in R.shapes():
        topo, mesh = M.object_topology(T(vol), num=1), M.label_surfaces(T(vol), num=1)
        assert topo.euler.is_cuda and topo.euler.tolist() == [euler] and topo.pinch_edges.tolist() == [0], name
        assert len(mesh.vertices) - len(mesh.quads) == 2 * euler, name
        _same(mesh, M.label_surfaces(vol, num=1), name)


def test_a_linked_stack_goes_in_without_a_host_trip():
    """link_label_stack's device volume straight into label_surfaces; the face counts per axis against measure_objects, on device outputs."""
    from ullsam_amd.utils import measure3d as M3
    from ullsam_amd.utils import mesh3d as M
    from ullsam_amd.utils import synthetic as S
    from ullsam_amd.utils.stack import link_label_stack
    planes, counts = S.label_stack(1, 6, 96, 96, 12, (5.0, 12.0), 2.5)
    volume = link_label_stack(torch.from_numpy(planes).to(DEV), counts, device=DEV)[0]
    assert volume.is_cuda and volume.dtype == torch.int32
    k = int(volume.max())
    assert k >= 2
    mesh, table = M.label_surfaces(volume, num=k), M3.measure_objects(volume, num=k)
    assert all(t.is_cuda for t in mesh)
    d = mesh.source % 6
    label = torch.repeat_interleave(torch.arange(k, device=DEV), mesh.fstart[1:] - mesh.fstart[:-1])
    per_axis = torch.zeros((k, 3), dtype=torch.int64, device=DEV)
    per_axis.index_put_((label, d // 2), torch.ones_like(d), accumulate=True)
    assert torch.equal(per_axis, table.surface[:, 1:4]) and int(mesh.fstart[-1]) == len(mesh.quads) == int(table.surface[:, 1:4].sum())
    _same(mesh, M.label_surfaces(volume.cpu(), num=k), "stack")
    _same(M.object_topology(volume, num=k), M.object_topology(volume.cpu(), num=k), "stack")
