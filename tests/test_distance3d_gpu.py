"""Distance transforms of label volumes on the GPU (csrc/distance3d.hip): the device route of utils.distance3d against the host form (itself checked
against the brute force of tests/distance3d_ref.py without a GPU), the raw outputs of the three passes through ops against that brute force, the
status word, and the shapes at which the kernels can go wrong.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance3d_ref as R
from tests.test_distance_gpu import _whole_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = 2 ** 31 - 1


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _same(got, want, what):
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want), what


def _all_five(vol, d, spacing, edge, radii=(0, 9, 100), what=""):
    """Every function on the device (d: the volume there) against the host form (vol)."""
    from ullsam_amd.utils import distance3d as D
    _same(D.inner_distance3d(d, spacing, edge), D.inner_distance3d(vol, spacing, edge), (what, "inner", spacing, edge))
    got, want = D.object_depth(d, spacing=spacing, edge=edge), D.object_depth(vol, spacing=spacing, edge=edge)
    _same(got.r2, want.r2, (what, "depth r2", spacing, edge))
    _same(got.xyz, want.xyz, (what, "depth xyz", spacing, edge))
    for r2 in radii:
        _same(D.shrink_labels3d(d, distance2=r2, spacing=spacing, edge=edge), D.shrink_labels3d(vol, distance2=r2, spacing=spacing, edge=edge),
              (what, "shrink", r2, spacing, edge))
    if edge is False:                                        # (the feature form has no edge: once per spacing)
        for m in (None,) + tuple(radii):
            got, want = D.background_feature3d(d, spacing, max_distance2=m), D.background_feature3d(vol, spacing, max_distance2=m)
            _same(got[0], want[0], (what, "feature D2", m, spacing))
            _same(got[1], want[1], (what, "feature nearest", m, spacing))
            if m is not None:
                _same(D.expand_labels3d(d, distance2=m, spacing=spacing), D.expand_labels3d(vol, distance2=m, spacing=spacing), (what, "expand", m, spacing))


# ---- the volumes -----------------------------------------------------------------------------------------------------------------------------------
def _whole_row_planes(w):
    """[3, 9, w]: rows that are one run each, the pattern of the 2-D tests' _whole_rows, its rows shifted from plane to plane."""
    a = _whole_rows(w)
    return np.stack([a, np.roll(a, 1, axis=0), a])


def _across_a_band():
    """[70, 5, 66]: the z pass works in bands of 64 planes.  One run spans all 70 planes, others start, end and change label around plane 64."""
    vol = np.zeros((70, 5, 66), np.int32)
    vol[:, 1, 3:9] = 1                                       # all 70 planes: both ends open
    vol[10:64, 2, 20:30] = 2                                 # ends with the first band
    vol[64:, 2, 20:30] = 3                                   # starts with the second
    vol[60:69, 3, 40:66] = 4                                 # across the band's end
    vol[1:66, 4, 50:60] = 5
    vol[30, 0, :] = 6                                        # one plane thick, whole rows
    return vol


def _long_y_run():
    vol = np.zeros((4, 300, 7), np.int32)
    vol[1:3, 2:298, 1:6] = 1
    vol[1:3, 150:160, 3] = 2
    vol[3, 40:300, :] = 3                                    # to the volume's end along y and x
    return vol


def _sparse():
    vol = np.zeros((6, 40, 420), np.int32)
    vol[0:2, 30:33, 5:9] = 1
    vol[4:6, 2:5, 400:405] = 2
    vol[2:4, 36:39, 200:204] = 3
    return vol


@pytest.fixture(scope="module")
def odd():
    """A volume whose voxel count is no multiple of 4, at an unaligned base: a slice of a larger tensor, contiguous at an odd offset."""
    vol = R.blobs(21, 5, 7, 9, n=6)
    assert vol.size % 4 != 0
    flat = torch.zeros((vol.size + 8,), dtype=torch.int32, device=DEV)
    flat[3:3 + vol.size] = T(vol).reshape(-1)
    d = flat[3:3 + vol.size].view(vol.shape)
    assert d.is_contiguous() and d.data_ptr() % 16 != 0
    return vol, d


# ---- the device route against the host form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", R.SPACINGS)
def test_device_route_equals_the_host_form_on_the_cpu_cases(spacing):
    for name, vol in R.cases():
        d = T(vol)
        for edge in R.EDGES:
            _all_five(vol, d, spacing, edge, what=name)


@pytest.mark.parametrize("w", [63, 64, 65, 130])
def test_whole_row_runs(w):
    vol = _whole_row_planes(w)
    d = T(vol)
    for spacing, edge in (((1, 1, 1), False), ((2, 3, 5), False), ((1, 1, 4), True), ((3, 1, 1), (True, False, False))):
        _all_five(vol, d, spacing, edge, radii=(4, 3000), what=f"whole rows {w}")


def _raw_passes_equal_the_host_passes(vol, d, s, e, what):
    """The z and y passes' raw outputs on a volume too large for brute force, against the host form's own passes (which
    tests/test_distance3d_cpu.py holds to brute force through their end result, and the small volumes below hold pass by pass)."""
    from ullsam_amd import ops
    from ullsam_amd.utils import distance3d as D
    voxels = lambda c: np.where(c >= INF, 0xFFFF, np.rint(np.sqrt(np.minimum(c, INF).astype(np.float64))).astype(np.int64))
    none = np.full(vol.shape, INF, np.int64)
    g, _, _ = ops.distance3d_z(d, False, e[0])
    assert np.array_equal(N(g), voxels(D._inner_pass(vol, none, 0, 1, e[0], None))), (what, "g", e)
    h, _ = ops.distance3d_y(d, g, None, s, e)
    want = D._inner_pass(vol, D._inner_pass(vol, none, 0, s[0] ** 2, e[0], None), 1, s[1] ** 2, e[1], None)
    assert np.array_equal(N(h), np.minimum(want, INF)), (what, "h", s, e)
    bd, bl = np.where(vol > 0, 0, INF).astype(np.int64), vol.astype(np.int64)
    g, near, _ = ops.distance3d_z(d, True)
    a, b = D._feature_pass(bd, bl, 0, 1, INF)
    assert np.array_equal(N(g), voxels(a)) and np.array_equal(N(near), np.where(a < INF, b, 0)), (what, "feature g")
    h, hl = ops.distance3d_y(d, g, near, s)
    a, b = D._feature_pass(*D._feature_pass(bd, bl, 0, s[0] ** 2, INF), 1, s[1] ** 2, INF)
    assert np.array_equal(N(h), np.minimum(a, INF)) and np.array_equal(N(hl), np.where(a < INF, b, 0)), (what, "feature h", s)


@pytest.mark.parametrize("make", [_across_a_band, _long_y_run, _sparse])
def test_bands_long_runs_and_a_sparse_volume(make):
    vol = make()
    d = T(vol)
    for spacing, edge in (((1, 1, 1), False), ((2, 3, 5), False), ((3, 1, 1), True), ((1, 1, 4), (True, False, False))):
        _all_five(vol, d, spacing, edge, radii=(16, 2500), what=make.__name__)
    _raw_passes_equal_the_host_passes(vol, d, (2, 3, 5), (False, False, False), make.__name__)
    _raw_passes_equal_the_host_passes(vol, d, (3, 1, 2), (True, True, False), make.__name__)


def test_unaligned_base_and_a_voxel_count_that_is_no_multiple_of_4(odd):
    vol, d = odd
    for spacing, edge in (((1, 1, 1), False), ((2, 3, 5), False), ((2, 3, 5), True)):
        _all_five(vol, d, spacing, edge, what="odd")


def test_near_the_int32_bound():
    from ullsam_amd import ops
    from ullsam_amd.utils import distance3d as D
    vol = np.ones((1, 2, 50), np.int32)
    vol[0, 1, 49] = 2
    d = T(vol)
    s = (1, 46000, 100)
    got = D.inner_distance3d(d, s)
    assert int(got[0, 0, 0]) == 46000 ** 2 + 4900 ** 2 == 2140010000
    _same(got, D.inner_distance3d(vol, s), "inner")
    assert np.array_equal(N(got), R.inner_distance(vol, s))
    f, want = D.background_feature3d(d, s), R.background_feature(vol, s)
    assert np.array_equal(N(f[0]), want[0]) and np.array_equal(N(f[1]), want[1])
    _all_five(vol, d, s, False, radii=(10 ** 4, 2140010000 - 1, 2140010000), what="near bound")
    with pytest.raises(ValueError):
        D.inner_distance3d(d, (1, 46340, 100))
    g, _, _ = ops.distance3d_z(d)
    with pytest.raises(ops._lib.UllsamError):                # the pass's own entry refuses it too
        ops.distance3d_y(d, g, None, (1, 46340, 100))
    _same(D.inner_distance3d(d, s), D.inner_distance3d(vol, s), "after the refused call")


def test_a_linked_stack_goes_straight_in():
    from ullsam_amd.utils import distance3d as D
    from ullsam_amd.utils import synthetic as S
    from ullsam_amd.utils.stack import link_label_stack
    planes, counts = S.label_stack(3, 12, 96, 130, 40, (6, 22), dz=2.5)
    volume = link_label_stack(planes, counts, device=DEV)[0]
    assert volume.is_cuda and volume.dtype == torch.int32 and tuple(volume.shape) == (12, 96, 130) and int(volume.max()) >= 10
    vol = volume.cpu().numpy()
    s = (5, 2, 2)
    _all_five(vol, volume, s, False, radii=(64,), what="stack")
    _same(D.inner_distance3d(volume, s, (True, False, False)), D.inner_distance3d(vol, s, (True, False, False)), "stack, clipped in z")
    run = lambda: (D.inner_distance3d(volume, s), *D.background_feature3d(volume, s), D.expand_labels3d(volume, 8, spacing=s),
                   D.shrink_labels3d(volume, 4, spacing=s, edge=True), *D.object_depth(volume, spacing=s))
    assert all(torch.equal(a, b) for a, b in zip(run(), run())), "two runs differ"
    _same(D.expand_labels3d(vol, 6, spacing=s, device=DEV), D.expand_labels3d(vol, 6, spacing=s), "numpy volume, device=")


# ---- the raw passes against brute force ---------------------------------------------------------------------------------------------------------------
def test_raw_pass_outputs_against_brute_force(odd):
    """Every ops wrapper called directly: the z pass's g (and nearest), the y pass's h (and its labels), every mode of the x pass, the decoded depths."""
    from ullsam_amd import ops
    extra = [("odd, unaligned", odd[0], odd[1])]
    for name, vol, d in [(n, v, T(v)) for n, v in R.cases()] + extra:
        z, h, w = vol.shape
        k = int(vol.max()) + 2
        for s, edge in (((1, 1, 1), False), ((2, 3, 5), True), ((2, 3, 5), (True, False, False))):
            e = R.edges(edge)
            g, none, flags = ops.distance3d_z(d, False, e[0], num=k)
            assert none is None and g.dtype == torch.uint16 and tuple(g.shape) == vol.shape and g.is_cuda
            assert np.array_equal(N(g), R.z_inner(vol, e[0])), (name, edge)
            hh, none = ops.distance3d_y(d, g, None, s, e)
            assert none is None and hh.dtype == torch.int32 and np.array_equal(N(hh), R.y_inner(vol, s, e)), (name, s, edge)
            want = R.inner_distance(vol, s, e) if name.startswith("odd") else R.reference(name, "inner", s, e)
            d2, _ = ops.distance3d_x(d, hh, None, "inner", s, e, flags=flags)
            assert d2.dtype == torch.int32 and np.array_equal(N(d2), want), (name, s, edge)
            for r2 in (0, 9, 50):
                hb, _ = ops.distance3d_y(d, g, None, s, e, limit=r2)
                out, _ = ops.distance3d_x(d, hb, None, "shrink", s, e, limit=r2, flags=flags)
                assert np.array_equal(N(out), R.shrink_labels(vol, r2, want)), (name, s, edge, r2)
            best, _ = ops.distance3d_x(d, hh, None, "depth", s, e, num=k, flags=flags)
            assert best.dtype == torch.int64 and tuple(best.shape) == (k,)
            r2s, xyz = ops.distance3d_depth_decode(best, h, w)
            wr2, wxyz = R.object_depth(vol, k, want)
            assert r2s.dtype == xyz.dtype == torch.int32 and np.array_equal(N(r2s), wr2) and np.array_equal(N(xyz), wxyz), (name, s, edge)
            assert flags.cpu().tolist() == [0, 0, 0, 0], name
        g, near, flags = ops.distance3d_z(d, True)
        wg, wnear = R.z_feature(vol)
        assert near.dtype == torch.int32 and np.array_equal(N(g), wg) and np.array_equal(N(near), wnear), name
        for s in ((1, 1, 1), (2, 3, 5)):
            hh, hl = ops.distance3d_y(d, g, near, s)
            wh, whl = R.y_feature(vol, s)
            assert hl.dtype == torch.int32 and np.array_equal(N(hh), wh) and np.array_equal(N(hl), whl), (name, s)
            want = R.background_feature(vol, s) if name.startswith("odd") else R.reference(name, "feature", s)
            for m in (None, 0, 9, 50):
                hb, hlb = ops.distance3d_y(d, g, near, s, limit=m)
                if m is not None:                            # beyond the limit the y pass owes only "above the limit"
                    assert np.array_equal(np.where(wh <= m, N(hb), -1), np.where(wh <= m, wh, -1)) and (N(hb)[wh > m] > m).all(), (name, s, m)
                    assert np.array_equal(np.where(wh <= m, N(hlb), -1), np.where(wh <= m, whl, -1)), (name, s, m)
                (d2, nl), _ = ops.distance3d_x(d, hb, hlb, "feature", s, limit=m, flags=flags)
                wf = want if m is None else R.bounded(want, m)
                assert np.array_equal(N(d2), wf[0]) and np.array_equal(N(nl), wf[1]), (name, s, m)
                if m is not None:
                    out, _ = ops.distance3d_x(d, hb, hlb, "expand", s, limit=m, flags=flags)
                    assert np.array_equal(N(out), R.expand_labels(vol, m, want)), (name, s, m)
        assert flags.cpu().tolist() == [0, 0, 0, 0], name


def test_ties_on_the_device():
    from tests.test_distance3d_cpu import TIES, _voxels
    from ullsam_amd.utils import distance3d as D
    for spacing, places, d2 in TIES:
        if d2 is None:
            places, d2 = places[:-1], 100
        shape = tuple(max(p[a] for p in places) + 2 for a in range(3))
        for first in range(len(places)):
            vol = _voxels(shape, {p: 3 + ((i - first) % len(places)) for i, p in enumerate(places)})
            got = D.background_feature3d(T(vol), spacing)
            assert int(got[0][0, 0, 0]) == d2 and int(got[1][0, 0, 0]) == 3, (spacing, first)
            want = D.background_feature3d(vol, spacing)
            _same(got[0], want[0], (spacing, first))
            _same(got[1], want[1], (spacing, first))
    full = torch.ones((3, 5, 70), dtype=torch.int32, device=DEV)
    d = D.object_depth(full, spacing=(2, 3, 5))
    assert d.r2.tolist() == [INF] and d.xyz.tolist() == [[0, 0, 0]]
    d = D.object_depth(full, spacing=(2, 3, 5), edge=True)  # z: 2, 4, 2; y: 3, 6, 9, 6, 3: the first voxel of (z, y) = (1, 1) with 5 (x + 1) >= 4
    assert d.r2.tolist() == [16] and d.xyz.tolist() == [[0, 1, 1]]


def test_an_id_out_of_range_raises_and_the_next_call_works():
    from ullsam_amd import ops
    from ullsam_amd.utils import distance3d as D
    vol = dict(R.cases())["absent ids"]                      # ids 2 and 5
    d = T(vol)
    s = (2, 3, 5)
    with pytest.raises(ops._lib.UllsamError):
        D.object_depth(d, num=4, spacing=s)
    g, _, flags = ops.distance3d_z(d, False, False, num=4)
    h, _ = ops.distance3d_y(d, g, None, s)
    best, _ = ops.distance3d_x(d, h, None, "depth", s, num=4, flags=flags)
    r2, xyz = ops.distance3d_depth_decode(best, vol.shape[1], vol.shape[2])
    without = np.where(vol == 5, 0, vol)                     # the id is skipped: the others are what they would be without it
    want = R.object_depth(without, 4, R.inner_distance(without, s))
    assert flags.cpu().tolist()[0] == 1 and np.array_equal(N(r2), want[0]) and np.array_equal(N(xyz), want[1])
    neg = vol.copy()
    neg[0, 0, 0] = -3
    for call in (lambda: D.inner_distance3d(T(neg)), lambda: D.background_feature3d(T(neg)), lambda: D.expand_labels3d(T(neg)),
                 lambda: D.shrink_labels3d(T(neg))):
        with pytest.raises(ops._lib.UllsamError):
            call()
    got, want = D.object_depth(d, num=5, spacing=s), D.object_depth(vol, num=5, spacing=s)
    _same(got.r2, want.r2, "the next call")
    _same(got.xyz, want.xyz, "the next call")
