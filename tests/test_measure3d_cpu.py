"""utils.measure3d without a GPU: the numpy route against the per-voxel loops and the exact rational definitions of tests/measure3d_ref.py, the 2-D
module on one-plane volumes, closed forms, the invariant that ties the tables to the contact list, the linker's own tables, derive3d, the argument
checks and the ABI.  Integer work: every integer assertion is equality."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import measure3d_ref as R
from tests import measure_ref as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


def test_numpy_route_equals_the_loops():
    from ullsam_amd.utils import measure3d as M
    seen_contacts = 0
    for name, vol, k in R.cases():
        for dtype, c in R.IMAGES:
            img = R.image(vol, dtype, c)
            got = M.measure_objects(vol, img, num=k)
            assert got.voxels.dtype == torch.int64 and got.box.dtype == torch.int32 and got.moments.dtype == torch.int64 and got.surface.dtype == torch.int64
            assert tuple(got.voxels.shape) == (k,) and tuple(got.box.shape) == (k, 6) and tuple(got.moments.shape) == (k, 9) and tuple(got.surface.shape) == (k, 7)
            if img is None:
                assert got.isum is None and got.isum2 is None and got.imin is None and got.imax is None
            else:
                cc = max(c, 1)
                assert got.isum.dtype == torch.int64 and got.isum2.dtype == torch.int64 and got.imin.dtype == torch.int32 and got.imax.dtype == torch.int32
                assert all(tuple(t.shape) == (k, cc) for t in (got.isum, got.isum2, got.imin, got.imax))
            assert R.as_lists(got) == R.tables(vol, k, img), (name, dtype, c)
        want = R.contacts(vol)
        pairs = M.object_contacts(vol, num=k)
        assert pairs.dtype == torch.int64 and tuple(pairs.shape) == (len(want), 5) and pairs.tolist() == [list(r) for r in want], name
        seen_contacts += len(want)
        # the same through a CPU tensor and with num left to volume.max()
        kmax = max(int(vol.max()), 0)
        assert R.as_lists(M.measure_objects(torch.from_numpy(vol))) == R.tables(vol, kmax), name
        assert M.object_contacts(torch.from_numpy(vol)).tolist() == [list(r) for r in want], name
    assert seen_contacts >= 10                                                      # (the cases do hold touching objects)


def test_one_plane_volumes_equal_the_2d_module():
    from ullsam_amd.utils import measure as M2
    from ullsam_amd.utils import measure3d as M
    for name, (lab, k) in R2.frames().items():
        h, w = lab.shape
        for dtype, c in ((None, 0), (np.uint8, 3), (np.uint16, 0)):
            img = None if dtype is None else R2.intensity(h, w, c, dtype)
            t2 = M2.measure_instances(lab, img, num=k)
            t3 = M.measure_objects(lab[None], None if img is None else img[None], num=k)
            assert torch.equal(t3.voxels, t2.area), name
            assert torch.equal(t3.box[:, [0, 1, 3, 4]], t2.box), name
            present = t2.area > 0
            assert t3.box[present][:, [2, 5]].tolist() == [[0, 0]] * int(present.sum()) and t3.box[~present][:, [2, 5]].tolist() == [[INT_MAX, -1]] * int((~present).sum())
            assert torch.equal(t3.moments[:, [0, 1, 3, 4, 6]], t2.moments) and not t3.moments[:, [2, 5, 7, 8]].any(), name   # sum z, z^2, xz, yz = 0
            s = t3.surface
            assert torch.equal(s[:, 2] + s[:, 3], t2.perimeter[:, 1]) and torch.equal(s[:, 1], 2 * t2.area) and torch.equal(s[:, 0], t2.area), name
            assert torch.equal(s[:, 5] + s[:, 6], t2.perimeter[:, 2]) and not s[:, 4].any(), name
            if img is not None:
                for f in ("isum", "isum2", "imin", "imax"):
                    assert torch.equal(getattr(t3, f), getattr(t2, f)), (name, f)
        p2, p3 = M2.label_contacts(lab, num=k), M.object_contacts(lab[None], num=k)
        assert torch.equal(p3[:, :2], p2[:, :2]) and not p3[:, 2].any() and torch.equal(p3[:, 3] + p3[:, 4], p2[:, 2]), name


def _s1(lo, n):
    return sum(range(lo, lo + n))


def _s2(lo, n):
    return sum(v * v for v in range(lo, lo + n))


def test_closed_forms_of_a_box_object():
    from ullsam_amd.utils import measure3d as M
    for (Z, H, W), (z0, y0, x0), (c, b, a) in (((9, 11, 13), (2, 3, 4), (4, 5, 6)), ((4, 5, 6), (0, 0, 0), (4, 5, 6)), ((5, 6, 7), (1, 2, 3), (1, 1, 1)),
                                               ((3, 8, 70), (1, 1, 2), (2, 3, 66)), ((6, 1, 9), (2, 0, 0), (3, 1, 9))):
        vol = np.zeros((Z, H, W), np.int32)
        vol[z0:z0 + c, y0:y0 + b, x0:x0 + a] = 2
        t = M.measure_objects(vol, num=2)
        sx, sy, sz = _s1(x0, a), _s1(y0, b), _s1(z0, c)
        inner = max(a - 2, 0) * max(b - 2, 0) * max(c - 2, 0)
        assert t.voxels.tolist() == [0, a * b * c]
        assert t.box.tolist() == [[INT_MAX] * 3 + [-1] * 3, [x0, y0, z0, x0 + a - 1, y0 + b - 1, z0 + c - 1]]
        assert t.moments.tolist() == [[0] * 9, [b * c * sx, a * c * sy, a * b * sz, b * c * _s2(x0, a), a * c * _s2(y0, b), a * b * _s2(z0, c),
                                                 c * sx * sy, b * sx * sz, a * sy * sz]]
        assert t.surface.tolist() == [[0] * 7, [a * b * c - inner, 2 * a * b, 2 * a * c, 2 * b * c, 0, 0, 0]]      # the same whether it fills the volume or not
        assert tuple(M.object_contacts(vol, num=2).shape) == (0, 5)
    # two boxes sharing a face normal to each axis in turn
    for axis in range(3):
        vol = np.zeros((6, 6, 6), np.int32)
        lo, hi = [slice(1, 5)] * 3, [slice(1, 5)] * 3
        lo[axis], hi[axis] = slice(1, 3), slice(3, 5)
        vol[tuple(lo)], vol[tuple(hi)] = 1, 2
        want = [0, 0, 0]
        want[axis] = 16
        assert M.object_contacts(vol).tolist() == [[1, 2] + want]
        assert M.measure_objects(vol).surface[:, 4:].tolist() == [want, want]


def test_single_label_lines_of_the_longest_side():
    from ullsam_amd.utils import measure3d as M
    n = 32767
    s1, s2 = n * (n - 1) // 2, (n - 1) * n * (2 * n - 1) // 6
    for axis, shape in ((0, (1, 1, n)), (2, (n, 1, 1))):                             # along x, along z
        t = M.measure_objects(np.ones(shape, np.int32), np.full(shape, 65535, np.uint16), num=1)
        mom, box = [0] * 9, [0, 0, 0, 0, 0, 0]
        mom[axis], mom[3 + axis], box[3 + axis] = s1, s2, n - 1
        assert t.voxels.tolist() == [n] and t.box.tolist() == [box] and t.moments.tolist() == [mom]
        faces = [2 * n] * 3
        faces[2 - axis] = 2                                                          # (fz, fy, fx): the two end faces along the line
        assert t.surface.tolist() == [[n] + faces + [0, 0, 0]]
        assert t.isum.tolist() == [[n * 65535]] and t.isum2.tolist() == [[n * 65535 ** 2]] and t.imin.tolist() == [[65535]] and t.imax.tolist() == [[65535]]


def test_contacts_sum_to_the_contact_faces_of_the_tables():
    from ullsam_amd.utils import measure3d as M
    vols = [(name, vol, k) for name, vol, k in R.cases()]
    vols.append(("every voxel its own id", (np.arange(4 * 5 * 6, dtype=np.int32) + 1).reshape(4, 5, 6), 120))
    for name, vol, k in vols:
        t = M.measure_objects(vol, num=k)
        pairs = M.object_contacts(vol, num=k).numpy()
        surf = t.surface.numpy()
        want = np.zeros((k, 3), np.int64)
        np.add.at(want, pairs[:, 0] - 1, pairs[:, 2:])
        np.add.at(want, pairs[:, 1] - 1, pairs[:, 2:])
        assert np.array_equal(surf[:, 4:7], want), name
        assert (surf[:, 1:4] >= surf[:, 4:7]).all() and (6 * surf[:, 0] >= surf[:, 1:4].sum(1)).all() and (surf[:, 1:4].sum(1) >= surf[:, 0]).all(), name
        assert int(t.voxels.sum()) == int((vol > 0).sum()), name
        assert (pairs[:, 0] < pairs[:, 1]).all() and (pairs[:, 0] > 0).all() and (pairs[:, 2:].sum(1) > 0).all() and (pairs[:, 2:] >= 0).all()
        assert (np.diff(pairs[:, 0] * (k + 1) + pairs[:, 1]) > 0).all()
    z, h, w = 4, 5, 6
    assert len(pairs) == (z - 1) * h * w + z * (h - 1) * w + z * h * (w - 1) and (pairs[:, 2:].sum(1) == 1).all()


def test_tables_of_a_linked_stack_equal_the_linkers_and_the_per_plane_tables():
    from ullsam_amd.utils import measure as M2
    from ullsam_amd.utils import measure3d as M
    from ullsam_amd.utils import stack as K
    from ullsam_amd.utils import synthetic as S
    planes, counts = S.label_stack(5, 6, 60, 80, 14, (5.0, 13.0), 2.5)
    volume, log, voxels, zrange, boxes = K.link_label_stack(planes, counts, mode="mutual", device="cpu")
    k = len(voxels)
    assert k >= 5 and int(volume.max()) == k
    img = R.intensity(6, 60, 80, 3, np.uint8, seed=3)
    t = M.measure_objects(volume, img, num=k)
    assert torch.equal(t.voxels, voxels) and torch.equal(t.box[:, [0, 1, 3, 4]], boxes) and torch.equal(t.box[:, [2, 5]], zrange)
    table = K.track_table(log, counts).numpy()                                       # [K, Z]: the local id of object k + 1 in plane z
    want = np.zeros((k, 3), np.int64)
    for z in range(len(counts)):
        rows = M2.measure_instances(planes[z], img[z], num=int(counts[z])).isum.numpy()
        on = table[:, z] > 0
        want[on] += rows[table[on, z] - 1]
    assert np.array_equal(t.isum.numpy(), want) and (table > 0).sum() > k             # (objects do span planes)


def _close(a, b, rel):
    return a == b or abs(a - b) <= rel * max(abs(a), abs(b))


def test_derive3d_against_the_rational_definition():
    from fractions import Fraction
    from ullsam_amd.utils import measure3d as M
    vol, k = R.ellipsoid_scene()
    img = R.intensity(vol.shape[0], vol.shape[1], vol.shape[2], 3, np.uint16, seed=4)
    t = M.measure_objects(vol, img, num=k)
    assert int(t.voxels[3]) == 0 and int((t.voxels > 0).sum()) == k - 1               # id 4 is absent
    assert int(t.box[:, 3].max()) == vol.shape[2] - 1                                 # one object is cut by the volume
    assert tuple(M.object_contacts(vol, num=k).shape) == (0, 5)                       # well separated
    for spacing, exact in (((2.5, 1.0, 1.0), (Fraction(5, 2), 1, 1)), ((1.0, 1.0, 1.0), (1, 1, 1))):
        sz, sy, sx = spacing
        d = M.derive3d(t, spacing=spacing)
        ref, iref = R.shape_fraction(vol, k, exact), R.intensity_fraction(vol, k, img)
        axes_checked = 0
        for i in range(k):
            if ref[i] is None:
                assert all(np.isnan(v[i]).all() for v in d.values()), i
                continue
            v, cen, cov = ref[i]
            volume = v * sz * sy * sx
            assert _close(d["volume"][i], volume, 1e-9) and _close(d["equivalent_diameter"][i], (6 * volume / math.pi) ** (1 / 3), 1e-9)
            for a in range(3):
                assert _close(d["centroid"][i, a], float(cen[a]), 1e-9), (i, a)
                for b in range(3):
                    assert _close(d["covariance"][i, a, b], float(cov[a][b]), 1e-9), (i, a, b)
            lam = [float(x) for x in d["eigenvalues"][i]]
            l1 = lam[0]
            assert lam[0] >= lam[1] >= lam[2] >= 0.0
            e1, e2, e3 = (float(x) for x in R.invariants(cov))
            assert abs(lam[0] + lam[1] + lam[2] - e1) <= 1e-9 * l1, i
            assert abs(lam[0] * lam[1] + lam[0] * lam[2] + lam[1] * lam[2] - e2) <= 1e-9 * l1 ** 2, i
            assert abs(lam[0] * lam[1] * lam[2] - e3) <= 1e-9 * l1 ** 3, i
            for a in range(3):
                assert _close(d["axis_lengths"][i, a], 2 * math.sqrt(5 * lam[a]), 1e-12)
            assert l1 - lam[1] > 1e-3 * l1, (i, lam)                                  # the separation the scene promises, on every object asserted on
            axis = d["principal_axis"][i]
            cf = np.array([[float(x) for x in row] for row in cov])
            assert np.linalg.norm(cf @ axis - l1 * axis) <= 1e-9 * l1 and abs(np.linalg.norm(axis) - 1.0) <= 1e-12, i
            assert axis[int(np.argmax(np.abs(axis)))] > 0, i
            axes_checked += 1
            fz, fy, fx, cz, cy, cx = (int(x) for x in t.surface[i, 1:])
            assert _close(d["surface_area"][i], fz * sy * sx + fy * sz * sx + fx * sz * sy, 1e-12) and d["contact_area"][i] == 0.0
            for j in range(3):
                mean, var = iref[i][j]
                assert _close(d["mean"][i, j], float(mean), 1e-9) and _close(d["std"][i, j], math.sqrt(float(var)), 1e-9)
                assert d["min"][i, j] == int(t.imin[i, j]) and d["max"][i, j] == int(t.imax[i, j])
        assert axes_checked == k - 1
    # the long axis of the first ellipsoid lies along x; under a large z spacing it turns to z
    assert abs(M.derive3d(t)["principal_axis"][0, 0]) > 0.99 and abs(M.derive3d(t, spacing=(10.0, 1.0, 1.0))["principal_axis"][0, 2]) > 0.99
    # a contact area in physical units, a single voxel, an empty table, a table without an image
    two = np.zeros((3, 4, 5), np.int32)
    two[1, 1:3, 1:3], two[2, 1:3, 1:3] = 1, 2
    d = M.derive3d(M.measure_objects(two), spacing=(3.0, 2.0, 0.5))
    assert d["contact_area"].tolist() == [4 * 2.0 * 0.5] * 2 and d["surface_area"].tolist() == [2 * 4 * 1.0 + 4 * 3 * 0.5 + 4 * 3 * 2.0] * 2 and "mean" not in d
    one = M.derive3d(M.measure_objects(np.array([[[0, 1]]], np.int32), num=1), spacing=(2.0, 3.0, 4.0))
    assert one["volume"][0] == 24.0 and one["centroid"][0].tolist() == [4.0, 0.0, 0.0] and one["eigenvalues"][0].tolist() == [0.0] * 3
    assert one["axis_lengths"][0].tolist() == [0.0] * 3 and one["surface_area"][0] == 2 * (12.0 + 8.0 + 6.0)
    assert all(len(v) == 0 for v in M.derive3d(M.measure_objects(np.zeros((2, 2, 2), np.int32), num=0)).values())
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), 2.0, (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            M.derive3d(t, spacing=bad)


class _Stub:
    def __init__(self, *shape):
        self.shape = shape


def test_limits_and_argument_checks():
    from ullsam_amd import _lib
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import measure3d as M
    for fn in (M.measure_objects, M.object_contacts):
        for shape, number in (((32768, 1, 1), "32768"), ((1, 32768, 1), "32768"), ((1, 1, 32768), "32768"), ((2048, 1024, 1024), str(2 ** 31)),
                              ((0, 4, 4), "0")):
            with pytest.raises(ValueError, match=number):                            # before any voxel is read: the stub has none
                fn(_Stub(*shape))
        for shape in ((4, 4), (1, 2, 3, 4)):
            with pytest.raises(ValueError):
                fn(_Stub(*shape))
    vol = np.zeros((3, 6, 8), np.int32)
    vol[1, 2:4, 2:5] = 1
    with pytest.raises(_lib.UllsamError, match="must be uint8 or uint16"):
        M.measure_objects(vol, np.zeros((3, 6, 8), np.float32), num=1)               # float intensity: the 2-D message
    with pytest.raises(_lib.UllsamError):
        M.measure_objects(vol, np.zeros((3, 6, 8, 5), np.uint8), num=1)              # C = 5
    with pytest.raises(ValueError):
        M.measure_objects(vol, np.zeros((3, 6, 9), np.uint8), num=1)                 # shape mismatch
    with pytest.raises(ValueError):
        M.measure_objects(vol, np.zeros((6, 8, 3), np.uint8), num=1)
    with pytest.raises(_lib.UllsamError):
        M.measure_objects(vol, num=-1)
    for bad in (2, -7, 2 ** 31 - 1):                                                 # an id outside 0..K, then a good call
        b = vol.copy()
        b[1, 3, 3] = bad
        with pytest.raises(_lib.UllsamError):
            M.measure_objects(b, num=1)
        with pytest.raises(_lib.UllsamError):
            M.object_contacts(b, num=1)
    assert M.measure_objects(vol, num=1).voxels.tolist() == [6]
    three = np.array([[[1, 2, 3]]], np.int32)
    with pytest.raises(_lib.UllsamError):
        M.object_contacts(three, num=3, max_pairs=1)                                 # two distinct pairs: refused, not truncated
    assert M.object_contacts(three, num=3, max_pairs=2).tolist() == [[1, 2, 0, 0, 1], [2, 3, 0, 0, 1]]
    for bad in (0, 2 ** 30 + 1):
        with pytest.raises(ValueError):
            M.object_contacts(three, max_pairs=bad)
    gen = object.__new__(SamAutomaticMaskGenerator)                                  # (the check comes before the model is touched)
    with pytest.raises(ValueError, match="measure=True"):
        gen.generate_stack_label_volume(np.zeros((2, 6, 8, 3), np.float32), measure=True)
    with pytest.raises(ValueError, match="measure=True"):
        gen.generate_stack_label_volume([np.zeros((6, 8, 3), np.uint8), np.zeros((6, 8), np.uint8)], measure=True)


# ---- ABI and resources -------------------------------------------------------------------------------------------------------------------------------
NAMES = ["ullsam_measure_objects3d", "ullsam_object_contacts3d"]


def test_abi_symbols_and_constants():
    from ullsam_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert _lib.ABI_VERSION == 14 == lib.ullsam_abi_version() == int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1))
    for s in NAMES:
        assert s in _lib.SIGNATURES and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    src = open(os.path.join(ROOT, "ullsam_amd", "csrc", "measure3d.hip")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert define("M3_TILE_R") == ops.MEASURE3D_TILE_R and define("M3_TILE_P") == ops.MEASURE3D_TILE_P and define("M3_TILE_W") == 256
    assert define("M3_MAX_SIDE") == ops.MEASURE3D_MAX_SIDE == 32767 and define("M3_MAX_SLOTS") == ops.MEASURE_LDS_SLOTS == 128
    assert ops.MEASURE3D_LDS_SLOTS in (0, 128)
    assert define("M3_MAX_SLOTS") * (8 * (define("M3_NSUM") + 8) + 4 * (6 + 8) + 4) < 65536      # the largest LDS table: no function attribute needed
    tree = open(os.path.join(ROOT, "ullsam_amd", "ops.py")).read()
    assert '"ullsam_measure_objects3d"' in tree and '"ullsam_object_contacts3d"' in tree
    assert not re.search(r"\b(float|double)\b", re.sub(r"//[^\n]*", "", src))         # integer work only


def test_measure3d_kernels_have_no_spill_and_no_scratch():
    from ullsam_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = {n: r for n, r in KR.kernels().items() if any(re.search(h, n) for h in KR.HOT_MEASURE3D)}
    assert len(ks) == 9, sorted(ks)                                                  # five channel counts, contacts, two inits, the compaction
    for n, r in ks.items():
        assert not r.get("vgpr_spill_count", 0) and not r.get("sgpr_spill_count", 0) and not r.get("private_segment_fixed_size", 0), (n, r)
        assert r.get("group_segment_fixed_size", 0) == 0, n                          # the table is dynamic LDS
