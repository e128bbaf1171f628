"""utils.distance3d without a GPU: the numpy host form against the per-voxel brute force of tests/distance3d_ref.py, hand-made ties, the 2-D module on
one-plane volumes, the int32 bound, argument errors, the ABI, and scipy where it is installed.  Integer work: every assertion is equality."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import distance3d_ref as R
from tests import distance_ref as R2
from ullsam_amd import _lib
from ullsam_amd.utils import distance as D2
from ullsam_amd.utils import distance3d as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1


def N(t):
    return t.numpy().astype(np.int64)


@pytest.fixture(scope="module")
def cases():
    return R.cases()


def test_the_cases_cover_what_they_should(cases):
    shapes = [vol.shape for name, vol in cases if name.startswith("blobs")]
    assert (1, 1, 1) in shapes and max(max(s) for s in shapes) == 12 and all(vol.size <= 4000 for _, vol in cases)
    assert any(s[0] == 1 and min(s[1:]) > 1 for s in shapes) and any(s[1] == 1 and s[0] > 1 and s[2] > 1 for s in shapes)
    assert any(s[2] == 1 and min(s[:2]) > 1 for s in shapes)
    by = dict(cases)
    assert (by["one label filling the volume"] == 1).all() and not by["no labelled voxel"].any()
    assert sum(int(vol.max()) > 0 for _, vol in cases) >= 14
    assert D.INF == R.INF == INF and D.MAX_SIDE == 32767 and D.MAX_SPACING == 46340 and 46340 ** 2 <= INF < 46341 ** 2 and D.MAX_B == INF - 1


@pytest.mark.parametrize("spacing", R.SPACINGS)
@pytest.mark.parametrize("edge", R.EDGES)
def test_inner_shrink_and_depth_against_brute_force(cases, spacing, edge):
    for name, vol in cases:
        want = R.reference(name, "inner", spacing, edge)
        got = D.inner_distance3d(vol, spacing, edge)
        assert got.dtype == torch.int32 and tuple(got.shape) == vol.shape
        assert np.array_equal(N(got), want), name
        for r2 in (0, 1, 9, 30, 100):
            out = D.shrink_labels3d(vol, distance2=r2, spacing=spacing, edge=edge)
            assert out.dtype == torch.int32 and np.array_equal(N(out), R.shrink_labels(vol, r2, want)), (name, r2)
        for num in (None, int(vol.max()) + 3):              # absent ids, and num beyond the largest id
            k = int(vol.max()) if num is None else num
            d = D.object_depth(vol, num=num, spacing=spacing, edge=edge)
            wr2, wxyz = R.object_depth(vol, k, want)
            assert d.r2.dtype == d.xyz.dtype == torch.int32 and tuple(d.r2.shape) == (k,) and tuple(d.xyz.shape) == (k, 3)
            assert np.array_equal(N(d.r2), wr2) and np.array_equal(N(d.xyz), wxyz), (name, num)


@pytest.mark.parametrize("spacing", R.SPACINGS)
def test_feature_and_expand_against_brute_force(cases, spacing):
    for name, vol in cases:
        want = R.reference(name, "feature", spacing)
        for m in (None, 0, 1, 8, 25, 90):
            d2, near = D.background_feature3d(vol, spacing, max_distance2=m)
            w = want if m is None else R.bounded(want, m)
            assert d2.dtype == near.dtype == torch.int32 and tuple(d2.shape) == tuple(near.shape) == vol.shape
            assert np.array_equal(N(d2), w[0]) and np.array_equal(N(near), w[1]), (name, m)
        for r2 in (0, 1, 2, 9, 30, 100):
            out = D.expand_labels3d(vol, distance2=r2, spacing=spacing)
            assert out.dtype == torch.int32 and np.array_equal(N(out), R.expand_labels(vol, r2, want)), (name, r2)


def test_one_label_filling_the_volume_and_no_labelled_voxel():
    vol = np.full((4, 5, 6), 1, np.int32)
    assert (N(D.inner_distance3d(vol, (2, 3, 5))) == INF).all()
    zs, ys, xs = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
    want = np.minimum(np.minimum(2 * np.minimum(zs + 1, 4 - zs), 3 * np.minimum(ys + 1, 5 - ys)), 5 * np.minimum(xs + 1, 6 - xs)) ** 2
    assert np.array_equal(N(D.inner_distance3d(vol, (2, 3, 5), edge=True)), want)
    assert np.array_equal(N(D.inner_distance3d(vol, (2, 3, 5), edge=(True, False, False))), (2 * np.minimum(zs + 1, 4 - zs)) ** 2)
    assert np.array_equal(N(D.shrink_labels3d(vol, distance=50)), vol)
    d = D.object_depth(vol)
    assert d.r2.tolist() == [INF] and d.xyz.tolist() == [[0, 0, 0]]
    vol = np.zeros((3, 4, 5), np.int32)
    d2, near = D.background_feature3d(vol, (1, 1, 4))
    assert (N(d2) == INF).all() and (N(near) == 0).all()
    assert not N(D.inner_distance3d(vol)).any() and not N(D.expand_labels3d(vol, 3)).any() and not N(D.shrink_labels3d(vol, 3)).any()
    d = D.object_depth(vol)
    assert tuple(d.r2.shape) == (0,) and tuple(d.xyz.shape) == (0, 3)
    d = D.object_depth(vol, num=2)
    assert d.r2.tolist() == [0, 0] and d.xyz.tolist() == [[-1, -1, -1]] * 2


# ---- ties: the smaller id wins whichever pass meets it --------------------------------------------------------------------------------------------
def _voxels(shape, pts):
    vol = np.zeros(shape, np.int32)
    for (z, y, x), i in pts.items():
        vol[z, y, x] = i
    return vol


TIES = [((1, 1, 1), [(0, 0, 5), (0, 3, 4), (3, 4, 0), (4, 0, 3), (5, 0, 0), (0, 5, 0)], 25),      # from (0, 0, 0): on its row, in its plane, in other planes
        ((2, 1, 1), [(2, 0, 3), (0, 5, 0), (0, 3, 4), (2, 3, 0)], 25),
        ((2, 3, 5), [(5, 0, 0), (0, 0, 2), (4, 2, 0), (3, 0, 0)], None)]              # 100, 100, 64 + 36 = 100, and a nearer one: 36


def test_ties_go_to_the_smaller_id():
    for spacing, places, d2 in TIES:
        shape = tuple(max(p[a] for p in places) + 2 for a in range(3))
        if d2 is None:
            places, nearer = places[:-1], places[-1]
            vol = _voxels(shape, {nearer: 9, **{p: 2 + i for i, p in enumerate(places)}})
            got = D.background_feature3d(vol, spacing)
            assert int(got[0][0, 0, 0]) == 36 and int(got[1][0, 0, 0]) == 9                        # nearer beats smaller
            d2 = 100
        for first in range(len(places)):                     # the smallest id at every place in turn, larger ones at the others
            ids = {p: 3 + ((i - first) % len(places)) for i, p in enumerate(places)}
            assert ids[places[first]] == 3
            vol = _voxels(shape, ids)
            got = D.background_feature3d(vol, spacing)
            assert int(got[0][0, 0, 0]) == d2 and int(got[1][0, 0, 0]) == 3, (spacing, first)
            want = R.background_feature(vol, spacing)
            assert np.array_equal(N(got[0]), want[0]) and np.array_equal(N(got[1]), want[1]), (spacing, first)
            assert np.array_equal(N(D.expand_labels3d(vol, distance2=d2, spacing=spacing)), R.expand_labels(vol, d2, want))
            assert int(D.expand_labels3d(vol, distance2=d2 - 1, spacing=spacing)[0, 0, 0]) == 0


def test_object_depth_tie_takes_the_first_voxel():
    vol = np.zeros((6, 8, 9), np.int32)
    vol[1:5, 1:7, 2:8] = 1                                   # 4 x 6 x 6: the 2 x 4 x 4 voxels in the middle share D2 = 4 at spacing 1
    d = D.object_depth(vol)
    assert d.r2.tolist() == [4] and d.xyz.tolist() == [[3, 2, 2]]
    d = D.object_depth(vol, spacing=(1, 2, 2))
    want = R.object_depth(vol, 1, R.inner_distance(vol, (1, 2, 2)))
    assert np.array_equal(N(d.r2), want[0]) and np.array_equal(N(d.xyz), want[1])


# ---- the 2-D module on a one-plane volume ------------------------------------------------------------------------------------------------------------
def test_one_plane_equals_the_2d_module():
    for name, lab in R2.cases():
        vol = lab[None]
        same = lambda a, b: torch.equal(a[0], b)
        assert same(D.inner_distance3d(vol), D2.inner_distance(lab)), name
        assert same(D.inner_distance3d(vol, edge=(False, True, True)), D2.inner_distance(lab, edge=True)), name
        for m in (None, 0, 10):
            got, want = D.background_feature3d(vol, max_distance2=m), D2.background_feature(lab, max_distance2=m)
            assert same(got[0], want[0]) and same(got[1], want[1]), (name, m)
        for r2 in (0, 2, 30):
            assert same(D.expand_labels3d(vol, distance2=r2), D2.expand_labels(lab, distance2=r2)), (name, r2)
            assert same(D.shrink_labels3d(vol, distance2=r2), D2.shrink_labels(lab, distance2=r2)), (name, r2)
            assert same(D.shrink_labels3d(vol, distance2=r2, edge=(False, True, True)), D2.shrink_labels(lab, distance2=r2, edge=True)), (name, r2)
        for edge3, edge2 in ((False, False), ((False, True, True), True)):
            got, want = D.object_depth(vol, edge=edge3), D2.instance_depth(lab, edge=edge2)
            assert torch.equal(got.r2, want.r2) and torch.equal(got.xyz[:, :2], want.xy), name
            assert (got.xyz[:, 2] == torch.where(want.xy[:, 0] >= 0, 0, -1)).all(), name


# ---- near the int32 bound ------------------------------------------------------------------------------------------------------------------------
def near_bound_volume():
    vol = np.ones((1, 2, 50), np.int32)
    vol[0, 1, 49] = 2
    return vol


def test_near_the_int32_bound():
    vol = near_bound_volume()
    d2 = D.inner_distance3d(vol, (1, 46000, 100))
    assert int(d2[0, 0, 0]) == 46000 ** 2 + 4900 ** 2 == 2140010000 < INF
    assert np.array_equal(N(d2), R.inner_distance(vol, (1, 46000, 100)))
    got, want = D.background_feature3d(vol, (1, 46000, 100)), R.background_feature(vol, (1, 46000, 100))
    assert np.array_equal(N(got[0]), want[0]) and np.array_equal(N(got[1]), want[1])
    with pytest.raises(ValueError, match=str(46340 ** 2 + 4900 ** 2)):
        D.inner_distance3d(vol, (1, 46340, 100))
    with pytest.raises(ValueError, match=str(46000 ** 2 * 4 + 5000 ** 2 + 1)):    # the edges add a voxel to every axis
        D.inner_distance3d(vol, (1, 46000, 100), edge=True)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------
class _Shape:
    """Stands for a volume too large to allocate: the limits are checked before a voxel is read."""
    def __init__(self, *shape):
        self.shape = shape


def test_routing_and_argument_errors():
    vol = R.blobs(5, 6, 7, 8)
    assert int(vol.max()) >= 1
    want = R.inner_distance(vol, (2, 1, 1))
    for volume in (vol, torch.from_numpy(vol), torch.from_numpy(vol.astype(np.int64))):
        out = D.inner_distance3d(volume, (2, 1, 1), device="cpu")
        assert out.device.type == "cpu" and out.dtype == torch.int32 and np.array_equal(N(out), want)
    assert torch.equal(D.expand_labels3d(vol, distance=3, spacing=(2, 1, 1)), D.expand_labels3d(vol, distance2=9, spacing=(2, 1, 1)))
    assert torch.equal(D.shrink_labels3d(vol, distance=2), D.shrink_labels3d(vol, distance2=4))
    assert torch.equal(D.inner_distance3d(vol, (np.int64(2), 1, 1)), D.inner_distance3d(vol, [2, 1, 1]))
    neg = vol.copy()
    neg[0, 0, 0] = -1
    fns = [D.inner_distance3d, D.background_feature3d, D.expand_labels3d, D.shrink_labels3d, D.object_depth]
    for f in fns:
        bad = [lambda: f(vol[0]), lambda: f(vol[None]), lambda: f(vol, spacing=(0, 1, 1)), lambda: f(vol, spacing=(1, 2.0, 1)),
               lambda: f(vol, spacing=(1, 1)), lambda: f(vol, spacing=2), lambda: f(vol, spacing=(1, 1, 46341)), lambda: f(vol, spacing=(1, True, 1)),
               lambda: f(_Shape(32767, 32767, 3)), lambda: f(_Shape(1, 32768, 1)), lambda: f(_Shape(0, 4, 4)), lambda: f(neg)]
        for i, call in enumerate(bad):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match=str(32767 * 32767 * 3)):
        D.inner_distance3d(_Shape(32767, 32767, 3))
    more = [lambda: D.inner_distance3d(vol, edge=(True, False)), lambda: D.inner_distance3d(vol, edge=1), lambda: D.shrink_labels3d(vol, edge="z"),
            lambda: D.expand_labels3d(vol, distance=-1), lambda: D.expand_labels3d(vol, distance=1.5), lambda: D.expand_labels3d(vol, distance2=INF),
            lambda: D.shrink_labels3d(vol, distance2=2.5), lambda: D.background_feature3d(vol, max_distance2=-1),
            lambda: D.background_feature3d(vol, max_distance2=INF), lambda: D.object_depth(vol, num=-1), lambda: D.object_depth(vol, num=int(vol.max()) - 1)]
    for call in more:
        with pytest.raises(ValueError):
            call()


# ---- scipy, where it is installed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", R.SPACINGS)
def test_against_scipy(cases, spacing):
    ndi = pytest.importorskip("scipy.ndimage")
    sq = lambda m: np.rint(ndi.distance_transform_edt(m, sampling=spacing) ** 2).astype(np.int64)
    for name, vol in cases:
        d2 = N(D.inner_distance3d(vol, spacing))
        for i in np.unique(vol[vol > 0]):
            m = vol == i
            if not m.all():                                  # scipy has no INF: the filled volume is tested above
                assert np.array_equal(d2[m], sq(m)[m]), (name, i)
        if (vol > 0).any():
            assert np.array_equal(N(D.background_feature3d(vol, spacing)[0]), sq(vol == 0)), name


# ---- ABI and resources -------------------------------------------------------------------------------------------------------------------------------
NAMES = ["ullsam_distance3d_z", "ullsam_distance3d_y", "ullsam_distance3d_x", "ullsam_distance3d_depth_decode"]


def test_abi_and_symbols():
    from ullsam_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert _lib.ABI_VERSION == 14 == lib.ullsam_abi_version() == int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1))
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("ullsam_distance3d_")) == sorted(NAMES)
    for s in NAMES:
        assert hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s


def test_distance3d_kernels_have_no_spill_and_no_scratch():
    from ullsam_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels()
    for pat in KR.HOT_DISTANCE3D:
        assert pat in KR.HOT_BF16
    hot = {n: r for n, r in ks.items() if any(re.search(h, n) for h in KR.HOT_DISTANCE3D)}
    assert len(hot) == 10, sorted(hot)                        # z and y in both forms, the five modes of x, the decode
    for n, r in hot.items():
        assert not (r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)), (n, r)
        assert r.get("group_segment_fixed_size", 0) == 0, (n, r)
