"""utils.distance without a GPU: the numpy host form against the per-pixel brute-force loops of tests/distance_ref.py, hand-made ties, bounds at
equality, argument errors, and scipy where it is installed.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance_ref as R
from ullsam_amd.utils import distance as D

INF = 2 ** 31 - 1


def N(t):
    return t.numpy().astype(np.int64)


@pytest.fixture(scope="module")
def cases():
    return R.cases()


def test_inf_and_limits():
    assert D.INF == R.INF == INF and D.MAX_SIDE == 32767 and 2 * 32766 ** 2 < INF


def test_the_cases_cover_what_they_should(cases):
    shapes = [lab.shape for name, lab in cases if name.startswith("blobs")]
    assert len(shapes) >= 12 and (1, 1) in shapes and any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes)
    assert max(max(s) for s in shapes) == 40 and sum(int(lab.max()) > 0 for _, lab in cases) >= 12


@pytest.mark.parametrize("edge", [False, True])
def test_inner_distance_against_the_loops(cases, edge):
    for name, lab in cases:
        got = D.inner_distance(lab, edge=edge)
        assert got.dtype == torch.int32 and tuple(got.shape) == lab.shape
        assert np.array_equal(N(got), R.inner_distance(lab, edge)), name


def test_frame_filling_instance():
    lab = np.full((7, 10), 1, np.int32)
    assert (N(D.inner_distance(lab)) == INF).all()
    ys, xs = np.mgrid[0:7, 0:10]
    want = np.minimum(np.minimum(xs + 1, 10 - xs), np.minimum(ys + 1, 7 - ys)) ** 2
    assert np.array_equal(N(D.inner_distance(lab, edge=True)), want)
    assert np.array_equal(N(D.shrink_labels(lab, distance=50)), lab)            # border_value = 1: nothing erodes
    d = D.instance_depth(lab)
    assert d.r2.tolist() == [INF] and d.xy.tolist() == [[0, 0]]


def test_background_feature_against_the_loops(cases):
    for name, lab in cases:
        for m in (None, 0, 1, 8, 25):
            d2, near = D.background_feature(lab, max_distance2=m)
            want = R.background_feature(lab, m)
            assert d2.dtype == near.dtype == torch.int32 and tuple(d2.shape) == tuple(near.shape) == lab.shape
            assert np.array_equal(N(d2), want[0]) and np.array_equal(N(near), want[1]), (name, m)


def test_no_labelled_pixel():
    lab = np.zeros((6, 5), np.int32)
    d2, near = D.background_feature(lab)
    assert (N(d2) == INF).all() and (N(near) == 0).all()
    assert (N(D.inner_distance(lab)) == 0).all() and (N(D.expand_labels(lab, 3)) == 0).all() and (N(D.shrink_labels(lab, 3)) == 0).all()
    d = D.instance_depth(lab)
    assert tuple(d.r2.shape) == (0,) and tuple(d.xy.shape) == (0, 2)
    d = D.instance_depth(lab, num=3)
    assert d.r2.tolist() == [0, 0, 0] and d.xy.tolist() == [[-1, -1]] * 3


@pytest.mark.parametrize("r2", [0, 1, 2, 9, 30])
def test_expand_and_shrink_against_the_loops(cases, r2):
    for name, lab in cases:
        assert np.array_equal(N(D.expand_labels(lab, distance2=r2)), R.expand_labels(lab, r2)), name
        for edge in (False, True):
            got = D.shrink_labels(lab, distance2=r2, edge=edge)
            assert got.dtype == torch.int32 and np.array_equal(N(got), R.shrink_labels(lab, r2, edge)), (name, edge)


@pytest.mark.parametrize("edge", [False, True])
def test_instance_depth_against_the_loops(cases, edge):
    for name, lab in cases:
        for num in (None, int(lab.max()) + 3):                                   # absent ids, and num beyond the largest id
            k = int(lab.max()) if num is None else num
            got = D.instance_depth(lab, num=num, edge=edge)
            want = R.instance_depth(lab, k, edge)
            assert got.r2.dtype == got.xy.dtype == torch.int32 and tuple(got.r2.shape) == (k,) and tuple(got.xy.shape) == (k, 2)
            assert np.array_equal(N(got.r2), want[0]) and np.array_equal(N(got.xy), want[1]), (name, num)
    lab = dict(cases)["absent ids"]
    d = D.instance_depth(lab)
    assert d.r2.tolist()[0] == 0 and d.xy.tolist()[0] == [-1, -1] and d.r2.tolist()[1] > 0 and d.r2.tolist()[4] > 0


# ---- ties: the smaller id wins, D2 is exact --------------------------------------------------------------------------------------------------
def _pixels(h, w, pts):
    lab = np.zeros((h, w), np.int32)
    for (x, y), i in pts.items():
        lab[y, x] = i
    return lab


def test_ties_go_to_the_smaller_id():
    lab = _pixels(3, 9, {(1, 1): 7, (7, 1): 4})                                  # midway on its row
    d2, near = D.background_feature(lab)
    assert int(d2[1, 4]) == 9 and int(near[1, 4]) == 4
    lab = _pixels(9, 3, {(1, 1): 2, (1, 7): 5})                                  # midway in its column, above and below
    d2, near = D.background_feature(lab)
    assert int(d2[4, 1]) == 9 and int(near[4, 1]) == 2
    lab = _pixels(9, 3, {(1, 1): 5, (1, 7): 2})
    assert int(D.background_feature(lab)[1][4, 1]) == 2
    lab = _pixels(6, 8, {(6, 1): 9, (4, 5): 3})                                  # from (1, 1): (5, 0) and (3, 4), both 25, the larger id on the axis
    d2, near = D.background_feature(lab)
    assert int(d2[1, 1]) == 25 and int(near[1, 1]) == 3
    lab = _pixels(6, 8, {(6, 1): 3, (4, 5): 9})
    d2, near = D.background_feature(lab)
    assert int(d2[1, 1]) == 25 and int(near[1, 1]) == 3
    lab = _pixels(8, 8, {(5, 0): 1, (3, 3): 2})                                  # from (0, 0): city-block 5 against 6, Euclidean 25 against 18
    d2, near = D.background_feature(lab)
    assert int(d2[0, 0]) == 18 and int(near[0, 0]) == 2
    for lab in (_pixels(3, 9, {(1, 1): 7, (7, 1): 4}), _pixels(6, 8, {(6, 1): 9, (4, 5): 3})):
        want = R.background_feature(lab)
        got = D.background_feature(lab)
        assert np.array_equal(N(got[0]), want[0]) and np.array_equal(N(got[1]), want[1])
        assert np.array_equal(N(D.expand_labels(lab, distance=5)), R.expand_labels(lab, 25))


def test_max_distance2_at_equality():
    lab = _pixels(1, 12, {(0, 0): 6})
    d2, near = D.background_feature(lab, max_distance2=25)
    assert d2[0].tolist() == [0, 1, 4, 9, 16, 25] + [INF] * 6 and near[0].tolist() == [6] * 6 + [0] * 6
    d2, near = D.background_feature(lab, max_distance2=24)
    assert int(d2[0, 5]) == INF and int(near[0, 5]) == 0 and int(d2[0, 4]) == 16


def test_radii():
    lab = R.blobs(3, 30, 34)
    assert np.array_equal(N(D.expand_labels(lab, distance=0)), lab) and np.array_equal(N(D.shrink_labels(lab, distance=0)), lab)
    assert np.array_equal(N(D.shrink_labels(lab, distance2=0, edge=True)), lab)
    assert torch.equal(D.expand_labels(lab, distance=3), D.expand_labels(lab, distance2=9))
    assert torch.equal(D.shrink_labels(lab, distance=3), D.shrink_labels(lab, distance2=9))
    one = _pixels(5, 5, {(2, 2): 1})
    assert int(D.expand_labels(one, distance2=1).sum()) == 5 and int(D.expand_labels(one, distance2=2).sum()) == 9   # the diagonal neighbours
    sq = np.zeros((7, 7), np.int32)
    sq[1:6, 1:6] = 1
    assert int(D.shrink_labels(sq, distance2=1).sum()) == 9 and int(D.shrink_labels(sq, distance2=2).sum()) == 9
    plus = sq.copy()
    plus[1, 1] = 0                                                                # a diagonal neighbour of (2, 2) is missing
    assert int(D.shrink_labels(plus, distance2=1)[2, 2]) == 1 and int(D.shrink_labels(plus, distance2=2)[2, 2]) == 0


def test_instance_depth_tie_takes_the_first_pixel():
    lab = np.zeros((8, 9), np.int32)
    lab[1:7, 2:8] = 1                                                             # 6 x 6: the four centre pixels share D2 = 9
    d = D.instance_depth(lab)
    d2 = R.inner_distance(lab, False)
    assert sorted(zip(*np.nonzero(d2 == d2.max()))) == [(3, 4), (3, 5), (4, 4), (4, 5)]
    assert d.r2.tolist() == [9] and d.xy.tolist() == [[4, 3]]


def test_routing_and_argument_errors():
    lab = R.blobs(5, 12, 12)
    for labels in (lab, torch.from_numpy(lab), torch.from_numpy(lab.astype(np.int64))):
        out = D.inner_distance(labels, device="cpu")
        assert out.device.type == "cpu" and out.dtype == torch.int32 and np.array_equal(N(out), R.inner_distance(lab, False))
    bad = [lambda: D.inner_distance(np.zeros((2, 3, 4), np.int32)), lambda: D.inner_distance(np.zeros((0, 4), np.int32)),
           lambda: D.inner_distance(np.zeros((1, 32768), np.int32)), lambda: D.inner_distance(-np.ones((2, 2), np.int32)),
           lambda: D.expand_labels(lab, distance=-1), lambda: D.expand_labels(lab, distance=1.5), lambda: D.expand_labels(lab, distance2=-1),
           lambda: D.expand_labels(lab, distance2=INF), lambda: D.shrink_labels(lab, distance=2.0), lambda: D.shrink_labels(lab, distance2=2.5),
           lambda: D.background_feature(lab, max_distance2=-1), lambda: D.background_feature(lab, max_distance2=INF),
           lambda: D.instance_depth(lab, num=-1), lambda: D.instance_depth(lab, num=2 ** 31 - 1), lambda: D.instance_depth(lab, num=int(lab.max()) - 1)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert int(lab.max()) >= 1


# ---- scipy, where it is installed ----------------------------------------------------------------------------------------------------------------
def test_against_scipy(cases):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, lab in cases:
        d2 = N(D.inner_distance(lab))
        for i in np.unique(lab[lab > 0]):
            m = lab == i
            if m.all():
                continue                                                          # scipy has no INF: the frame-filling case is tested above
            assert np.array_equal(d2[m], np.rint(ndi.distance_transform_edt(m) ** 2).astype(np.int64)[m]), name
            for r2 in (1, 2, 9):
                r = int(np.sqrt(r2))
                yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
                disc = yy ** 2 + xx ** 2 <= r2
                for edge in (False, True):
                    want = ndi.binary_erosion(m, disc, border_value=0 if edge else 1)
                    assert np.array_equal(N(D.shrink_labels(lab, distance2=r2, edge=edge)) == i, want), (name, r2, edge)
        if not (lab > 0).any():
            continue
        bd, near = (N(t) for t in D.background_feature(lab))
        edt, idx = ndi.distance_transform_edt(lab == 0, return_indices=True)
        assert np.array_equal(bd, np.rint(edt ** 2).astype(np.int64)), name
        at = lab[idx[0], idx[1]]                                                  # scipy's label: a valid minimiser, not always the smallest id
        ys, xs = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
        assert np.array_equal((idx[0] - ys) ** 2 + (idx[1] - xs) ** 2, bd) and (at > 0).all() and (near <= at).all(), name
