"""Distance transforms of label images on the GPU (csrc/distance.hip): the device route of utils.distance against the host form (itself checked
against the brute-force loops of tests/distance_ref.py without a GPU), the kernels' raw outputs through ops against those loops, the status word,
and the shapes at which the kernels take another path.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = 2 ** 31 - 1
HALO = 128                                                # ops.DISTANCE_LDS_HALO: the row pass stages its segment in LDS up to this reach


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _whole_rows(w):
    """Rows that are one run each (and two that are not), as in the stack's cases: widths around the 64-lane segment."""
    lab = np.zeros((9, w), np.int32)
    lab[1] = 1
    lab[2] = 1
    lab[3] = 2
    lab[5, : w // 2] = 3
    lab[5, w // 2:] = 4
    lab[7, 1:w - 1] = 5
    lab[8] = 5
    return lab


def _wide():
    """One label over several 256-pixel row tiles, a second one inside it, background around."""
    lab = np.zeros((40, 700), np.int32)
    lab[4:33, 10:690] = 1
    lab[12:20, 300:420] = 2
    lab[36:39, 500:] = 3
    return lab


def _disc(h, w, cy, cx, r, i=1):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where((ys - cy) ** 2 + (xs - cx) ** 2 <= r * r, i, 0).astype(np.int32)


@pytest.fixture(scope="module")
def small():
    return R.cases()


@pytest.fixture(scope="module")
def shapes(small):
    from ullsam_amd.utils import synthetic as S
    frame = S.label_frame(7, 300, 517, 90, (6.0, 22.0))
    assert len(np.unique(frame)) > 40
    odd = R.blobs(21, 37, 63, n=9)
    assert odd.size % 4 != 0
    sparse = np.zeros((150, 420), np.int32)               # far apart: reaches of 128 and 129 columns matter
    sparse[70:75, 5:9] = 1
    sparse[20:24, 400:405] = 2
    sparse[140:145, 200:204] = 3
    return list(small) + [(f"whole rows, width {w}", _whole_rows(w)) for w in (63, 64, 65, 130)] + [
        ("one label over several row tiles", _wide()), ("H * W no multiple of 4", odd), ("sparse", sparse), ("label_frame 300 x 517", frame),
        ("one instance of thousands of pixels", _disc(150, 170, 70, 90, 61))]


def _same(got, want, what):
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want), what


def test_device_route_equals_the_host_form(shapes):
    from ullsam_amd.utils import distance as D
    for name, lab in shapes:
        d = T(lab)
        for edge in (False, True):
            _same(D.inner_distance(d, edge=edge), D.inner_distance(lab, edge=edge), (name, "inner", edge))
            for r2 in (0, 4, 30):
                _same(D.shrink_labels(d, distance2=r2, edge=edge), D.shrink_labels(lab, distance2=r2, edge=edge), (name, "shrink", r2, edge))
            got, want = D.instance_depth(d, edge=edge), D.instance_depth(lab, edge=edge)
            _same(got.r2, want.r2, (name, "depth r2", edge))
            _same(got.xy, want.xy, (name, "depth xy", edge))
        for m in (None, 0, 10):
            got, want = D.background_feature(d, max_distance2=m), D.background_feature(lab, max_distance2=m)
            _same(got[0], want[0], (name, "feature D2", m))
            _same(got[1], want[1], (name, "feature nearest", m))
        for r2 in (0, 1, 64):
            _same(D.expand_labels(d, distance2=r2), D.expand_labels(lab, distance2=r2), (name, "expand", r2))
        _same(D.expand_labels(lab, distance=3, device=DEV), D.expand_labels(lab, distance=3), (name, "numpy labels, device="))
        run = lambda: (D.inner_distance(d), *D.background_feature(d), D.expand_labels(d, distance=5), D.shrink_labels(d, distance=2, edge=True),
                       *D.instance_depth(d))
        assert all(torch.equal(a, b) for a, b in zip(run(), run())), (name, "two runs differ")


def test_reach_at_the_lds_cap_and_beyond(shapes):
    """floor(sqrt(limit)) = 128 is the last bounded call served from LDS, 129 the first served from global memory; both routes give the host form's answer,
    and where both can serve a call they agree."""
    from ullsam_amd import ops
    from ullsam_amd.utils import distance as D
    assert ops.DISTANCE_LDS_HALO == HALO
    by = dict(shapes)
    for name in ("sparse", "one label over several row tiles", "one instance of thousands of pixels"):
        lab = by[name]
        d = T(lab)
        for reach in (HALO, HALO + 1):
            r2 = reach * reach
            routes = ("auto", "lds", "global") if reach == HALO else ("auto", "global")
            want = D.expand_labels(lab, distance=reach), D.shrink_labels(lab, distance2=r2 + 5), D.background_feature(lab, max_distance2=r2)
            for route in routes:
                _same(D.expand_labels(d, distance=reach, route=route), want[0], (name, reach, route))
                _same(D.shrink_labels(d, distance2=r2 + 5, route=route), want[1], (name, reach, route))
                got = D.background_feature(d, max_distance2=r2, route=route)
                _same(got[0], want[2][0], (name, reach, route))
                _same(got[1], want[2][1], (name, reach, route))
        with pytest.raises(ops._lib.UllsamError):
            D.expand_labels(d, distance=HALO + 1, route="lds")
        _same(D.expand_labels(d, distance=2), D.expand_labels(lab, distance=2), (name, "after the refused route"))


def test_unaligned_base_pointer(shapes):
    from ullsam_amd.utils import distance as D
    # (the kernels move 2 or 4 bytes a lane and ask for no alignment; a route of wider accesses would have to pass here, at widths that are
    # multiples of 4 too)
    for name in ("H * W no multiple of 4", "whole rows, width 65", "whole rows, width 64", "one label over several row tiles", "label_frame 300 x 517"):
        lab = dict(shapes)[name]
        h, w = lab.shape
        for off in (1, 3):
            flat = torch.zeros((h * w + 8,), dtype=torch.int32, device=DEV)
            flat[off:off + h * w] = T(lab).reshape(-1)
            d = flat[off:off + h * w].view(h, w)
            assert d.is_contiguous() and d.data_ptr() % 16 != 0
            _same(D.inner_distance(d, edge=True), D.inner_distance(lab, edge=True), (name, off))
            _same(D.expand_labels(d, distance=4), D.expand_labels(lab, distance=4), (name, off))
            _same(D.shrink_labels(d, distance=2), D.shrink_labels(lab, distance=2), (name, off))
            _same(D.background_feature(d)[1], D.background_feature(lab)[1], (name, off))


def test_raw_kernel_outputs_against_the_loops(small):
    """Every ops wrapper called directly: the column pass's g (and nearest), every mode of the row pass, the decoded depths."""
    from ullsam_amd import ops
    extra = [("whole rows, width 65", _whole_rows(65)), ("blobs 37 x 63", R.blobs(21, 37, 63, n=9))]
    for name, lab in list(small) + extra:
        d = T(lab)
        h, w = lab.shape
        k = int(lab.max()) + 2
        for edge in (False, True):
            g, none, flags = ops.distance_columns(d, False, edge)
            assert none is None and g.dtype == torch.uint16 and tuple(g.shape) == (h, w) and g.is_cuda
            assert np.array_equal(N(g), R.column_inner(lab, edge)), (name, edge)
            d2, _ = ops.distance_rows(d, g, None, "inner", edge, flags=flags)
            want = R.inner_distance(lab, edge)
            assert d2.dtype == torch.int32 and np.array_equal(N(d2), want), (name, edge)
            for r2 in (0, 2, 9):
                for route in ("lds", "global"):
                    out, _ = ops.distance_rows(d, g, None, "shrink", edge, limit=r2, route=route, flags=flags)
                    assert np.array_equal(N(out), R.shrink_labels(lab, r2, edge)), (name, edge, r2, route)
            g, _, _ = ops.distance_columns(d, False, edge, num=k, flags=flags)
            best, _ = ops.distance_rows(d, g, None, "depth", edge, num=k, flags=flags)
            assert best.dtype == torch.int64 and tuple(best.shape) == (k,)
            r2s, xy = ops.distance_depth_decode(best, w)
            wr2, wxy = R.instance_depth(lab, k, edge)
            assert r2s.dtype == xy.dtype == torch.int32 and np.array_equal(N(r2s), wr2) and np.array_equal(N(xy), wxy), (name, edge)
            assert flags.cpu().tolist() == [0, 0, 0, 0], name
        g, near, flags = ops.distance_columns(d, True)
        wg, wnear = R.column_feature(lab)
        assert near.dtype == torch.int32 and np.array_equal(N(g), wg) and np.array_equal(N(near), wnear), name
        for m in (None, 0, 5, 25):
            for route in (("global",) if m is None else ("lds", "global")):
                (d2, nl), _ = ops.distance_rows(d, g, near, "feature", limit=m, route=route, flags=flags)
                want = R.background_feature(lab, m)
                assert np.array_equal(N(d2), want[0]) and np.array_equal(N(nl), want[1]), (name, m, route)
        for r2 in (0, 1, 2, 16):
            for route in ("lds", "global"):
                out, _ = ops.distance_rows(d, g, near, "expand", limit=r2, route=route, flags=flags)
                assert np.array_equal(N(out), R.expand_labels(lab, r2)), (name, r2, route)
        assert flags.cpu().tolist() == [0, 0, 0, 0], name


def test_ties_on_the_device():
    from ullsam_amd.utils import distance as D
    lab = np.zeros((6, 8), np.int32)
    lab[1, 6], lab[5, 4] = 9, 3                          # from (1, 1): (5, 0) and (3, 4), both 25, the larger id on the axis
    d2, near = D.background_feature(T(lab))
    assert int(d2[1, 1]) == 25 and int(near[1, 1]) == 3
    lab = np.zeros((9, 3), np.int32)
    lab[1, 1], lab[7, 1] = 5, 2                          # above and below at equal distance
    d2, near = D.background_feature(T(lab))
    assert int(d2[4, 1]) == 9 and int(near[4, 1]) == 2
    lab = np.zeros((8, 9), np.int32)
    lab[1:7, 2:8] = 1                                    # four centre pixels share the maximum: the first in row-major order
    d = D.instance_depth(T(lab))
    assert d.r2.tolist() == [9] and d.xy.tolist() == [[4, 3]]
    full = D.instance_depth(torch.ones((5, 70), dtype=torch.int32, device=DEV))
    assert full.r2.tolist() == [INF] and full.xy.tolist() == [[0, 0]]
    assert D.instance_depth(torch.ones((5, 70), dtype=torch.int32, device=DEV), edge=True).r2.tolist() == [9]


def test_depth_under_contention(shapes):
    """Thousands of pixels of one instance send their words to one slot: the maximum and its first pixel do not depend on the order of arrival."""
    from ullsam_amd.utils import distance as D
    lab = dict(shapes)["one instance of thousands of pixels"]
    assert int((lab == 1).sum()) > 10000
    want = D.instance_depth(lab, num=3)
    assert want.r2.tolist()[1:] == [0, 0] and want.xy.tolist() == [[90, 70], [-1, -1], [-1, -1]]      # the disc's centre; ids 2 and 3 are absent
    for _ in range(3):
        got = D.instance_depth(T(lab), num=3)
        _same(got.r2, want.r2, "r2")
        _same(got.xy, want.xy, "xy")


def test_an_id_out_of_range_raises_and_the_next_call_works(shapes):
    from ullsam_amd import ops
    from ullsam_amd.utils import distance as D
    lab = dict(shapes)["absent ids"]                     # ids 2 and 5
    d = T(lab)
    with pytest.raises(ops._lib.UllsamError):
        D.instance_depth(d, num=4)
    g, _, flags = ops.distance_columns(d, False, False, num=4)
    best, _ = ops.distance_rows(d, g, None, "depth", num=4, flags=flags)
    r2, xy = ops.distance_depth_decode(best, lab.shape[1])
    want = R.instance_depth(np.where(lab == 5, 0, lab), 4, False)    # the id is skipped: the others are what they would be without it
    assert flags.cpu().tolist()[0] == 1 and np.array_equal(N(r2), want[0]) and np.array_equal(N(xy), want[1])
    neg = lab.copy()
    neg[0, 0] = -3
    with pytest.raises(ops._lib.UllsamError):
        D.inner_distance(T(neg))
    got, want = D.instance_depth(d, num=5), D.instance_depth(lab, num=5)
    _same(got.r2, want.r2, "the next call")
    _same(got.xy, want.xy, "the next call")
