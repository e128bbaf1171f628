"""Outlines of label images without a GPU: the host form of utils.outline (numpy: side masks, scan, successors by lookup, doubling on arrays, ordered
compaction) against the plain loops of tests/outline_ref.py, the inverse operation, the sums measure_instances knows, the GeoJSON exit, the errors.
Integer work: every assertion is equality."""
import json

import numpy as np
import pytest
import torch

from tests import distance_ref as DR
from tests import outline_ref as R

CONN = (8, 4)


@pytest.fixture(scope="module")
def shapes():
    from ullsam_amd.utils import synthetic as S
    return list(R.shapes().items()) + DR.cases() + [("label_frame 120 x 157", S.label_frame(7, 120, 157, 30, (6.0, 14.0)))]


@pytest.fixture(scope="module")
def loops(shapes):
    """{(name, connectivity): the plain loops' answer}: computed once, shared, never changed."""
    return {(name, c): R.outlines(lab, c) for name, lab in shapes for c in CONN}


@pytest.fixture(scope="module")
def host(shapes):
    from ullsam_amd.utils import outline as O
    return {(name, c): O.label_outlines(lab, c) for name, lab in shapes for c in CONN}


def N(t):
    return t.numpy().astype(np.int64)


def test_the_shapes_are_what_they_claim(shapes, loops):
    d = dict(shapes)
    assert d["checkerboard 33 x 31"].shape == (33, 31) and d["noise 24 x 31"].max() == 2 and d["H * W no multiple of 4"].size % 4 != 0
    nest = loops[("nested rings 9 x 9", 8)]
    assert len(nest.label) == 5 and int((nest.area2 < 0).sum()) == 2
    assert len(loops[("noise 24 x 31", 8)].label) == 79 and len(loops[("noise 24 x 31", 4)].label) == 180
    board = int(d["checkerboard 33 x 31"].sum())
    four, eight = loops[("checkerboard 33 x 31", 4)], loops[("checkerboard 33 x 31", 8)]
    assert len(four.label) == board and (four.edges == 4).all()                     # one loop per pixel
    white = int((d["checkerboard 33 x 31"][1:-1, 1:-1] == 0).sum())                 # every inner white square is a hole
    assert int((eight.area2 < 0).sum()) == white and int((eight.area2 > 0).sum()) == 1
    for c in CONN:
        sp = loops[("spiral 64 x 64", c)]
        assert len(sp.label) == 1 and int(sp.edges[0]) > 2048                        # the doubling needs more than 11 rounds
    assert len(loops[("an empty frame", 8)].label) == 0 and loops[("absent ids", 8)].loops_of.tolist() == [0, 1, 0, 0, 1]


@pytest.mark.parametrize("c", CONN)
def test_host_form_equals_the_plain_loops(shapes, loops, host, c):
    dt = dict(label=torch.int32, start=torch.int32, edges=torch.int32, area2=torch.int64, parent=torch.int32, vertices=torch.int32, loops_of=torch.int32)
    for name, lab in shapes:
        got, want = host[(name, c)], loops[(name, c)]
        for f in R.FIELDS:
            g, w = getattr(got, f), getattr(want, f)
            assert not g.is_cuda and g.dtype == dt[f] and tuple(g.shape) == w.shape and np.array_equal(N(g), w), (name, c, f)


@pytest.mark.parametrize("c", CONN)
def test_fill_is_the_inverse(shapes, host, c):
    for name, lab in shapes:
        assert np.array_equal(R.fill(host[(name, c)], *lab.shape), np.maximum(lab, 0)), (name, c)


@pytest.mark.parametrize("c", CONN)
def test_sums_equal_measure_instances(shapes, host, c):
    from ullsam_amd.utils import measure as M
    for name, lab in shapes:
        out = host[(name, c)]
        k = int(lab.max())
        assert out.loops_of.numel() == k, name
        if not k:
            continue
        table = M.measure_instances(lab, num=k)
        area2, edges = np.zeros(k, np.int64), np.zeros(k, np.int64)
        np.add.at(area2, N(out.label) - 1, N(out.area2))
        np.add.at(edges, N(out.label) - 1, N(out.edges))
        assert np.array_equal(area2, 2 * N(table.area)) and np.array_equal(edges, N(table.perimeter)[:, 1]), (name, c)


@pytest.mark.parametrize("c", CONN)
def test_leaders_and_parents(shapes, loops, host, c):
    for name, lab in shapes:
        out = host[(name, c)]
        label, area2, parent = N(out.label), N(out.area2), N(out.parent)
        leaders = [cyc[0] for _, cyc in R.cycles(lab, c)]
        assert len(leaders) == len(label) and (area2 != 0).all(), name
        for i, e in enumerate(leaders):
            assert (e % 4 == 0) == (area2[i] > 0) and (e % 4 == 2) == (area2[i] < 0), (name, c, i)       # top side: outer; bottom side: hole
            assert area2[parent[i]] > 0 and label[parent[i]] == label[i] and (parent[i] == i) == (area2[i] > 0), (name, c, i)
            if area2[i] > 0:                                                                              # the leader's tail opens the ring
                p = e // 4
                assert N(out.vertices)[N(out.start)[i]].tolist() == [p % lab.shape[1], p // lab.shape[1]], (name, c, i)
        assert np.array_equal(N(out.start)[1:] - N(out.start)[:-1] >= 4, np.ones(len(label), bool)), name   # a loop has at least four corners
    board = host[("checkerboard 33 x 31", 8)]
    assert int((N(board.area2) < 0).sum()) > 400                                                          # parents found over chains of many hops


@pytest.mark.parametrize("c,structure", [(8, np.ones((3, 3), int)), (4, np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]))])
def test_outer_loops_are_scipy_components(shapes, host, c, structure):
    try:
        from scipy import ndimage
    except ImportError:
        return                                            # (the claim is about scipy: nothing to compare with where it is absent)
    for name, lab in shapes:
        out = host[(name, c)]
        outer = np.bincount(N(out.label)[N(out.area2) > 0] - 1, minlength=int(lab.max()))[:int(lab.max())]
        want = [ndimage.label(lab == k, structure)[1] for k in range(1, int(lab.max()) + 1)]
        assert outer.tolist() == want, (name, c)


def test_polygons_and_geojson(shapes, host):
    from ullsam_amd.utils import outline as O
    out = host[("nested rings 9 x 9", 8)]
    polys = O.polygons(out, 1)
    assert len(polys) == 2 and [len(h) for _, h in polys] == [1, 1] and all(e.dtype == np.float64 and e.shape[1] == 2 for e, _ in polys)
    assert polys[0][0].tolist() == [[1, 1], [8, 1], [8, 8], [1, 8]] and polys[0][1][0].tolist() == [[2, 2], [2, 7], [7, 7], [7, 2]]
    assert polys[1][0].tolist() == [[3, 3], [6, 3], [6, 6], [3, 6]] and polys[1][1][0].tolist() == [[5, 4], [4, 4], [4, 5], [5, 5]]
    assert [e.tolist() for e, _ in O.polygons(out, 2)] == [[[4, 4], [5, 4], [5, 5], [4, 5]]] and O.polygons(out, 3) == []
    gj = O.to_geojson(out, pixel_size=0.5, origin=(10.0, -2.0), properties=[{"name": "ring"}, {"name": "dot", "label": 2}])
    assert json.loads(json.dumps(gj)) == gj and gj["type"] == "FeatureCollection" and [f["id"] for f in gj["features"]] == [1, 2]
    one, two = gj["features"]
    assert one["type"] == "Feature" and one["geometry"]["type"] == "MultiPolygon" and one["properties"] == {"label": 1, "name": "ring"}
    assert two["properties"] == {"label": 2, "name": "dot"}
    coords = one["geometry"]["coordinates"]
    assert len(coords) == 2 and [len(p) for p in coords] == [2, 2]                  # one polygon per outer loop, its hole attached
    assert coords[0][0] == [[10.5, -1.5], [14.0, -1.5], [14.0, 2.0], [10.5, 2.0], [10.5, -1.5]]
    assert coords[1][1] == [[12.5, 0.0], [12.0, 0.0], [12.0, 0.5], [12.5, 0.5], [12.5, 0.0]]
    for name, lab in shapes:                                                        # closed rings, polygons = outer loops, holes = holes, everywhere
        for c in CONN:
            o = host[(name, c)]
            g = O.to_geojson(o)
            present = (np.flatnonzero(N(o.loops_of)) + 1).tolist()
            assert [f["id"] for f in g["features"]] == present, name
            n_outer = n_holes = 0
            for f in g["features"]:
                for poly in f["geometry"]["coordinates"]:
                    n_outer += 1
                    n_holes += len(poly) - 1
                    assert all(r[0] == r[-1] and len(r) >= 5 for r in poly), name
            assert n_outer == int((N(o.area2) > 0).sum()) and n_holes == int((N(o.area2) < 0).sum()), (name, c)
    lab = dict(shapes)["absent ids"]
    plain = O.to_geojson(host[("absent ids", 8)])
    assert [f["id"] for f in plain["features"]] == [2, 5] and plain["features"][1]["geometry"]["coordinates"] == [[[[6.0, 6.0], [11.0, 6.0], [11.0, 9.0], [6.0, 9.0], [6.0, 6.0]]]]
    assert lab[6, 6] == 5


def test_inputs_and_errors(shapes, host):
    from ullsam_amd import _lib
    from ullsam_amd.utils import outline as O
    lab = dict(shapes)["absent ids"]
    want = host[("absent ids", 8)]
    for form in (torch.from_numpy(lab), lab.astype(np.int64), np.asarray(lab.tolist())):
        got = O.label_outlines(form, device="cpu")
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert O.label_outlines(lab, num=7).loops_of.tolist() == [0, 1, 0, 0, 1, 0, 0]
    neg = lab.copy()
    neg[0, 0] = -3
    with pytest.raises(_lib.UllsamError):
        O.label_outlines(neg)
    with pytest.raises(_lib.UllsamError):
        O.label_outlines(lab, num=4)
    for bad in (6, 0, True, "8", 8.5):
        with pytest.raises(ValueError):
            O.label_outlines(lab, connectivity=bad)
    with pytest.raises(ValueError):
        O.label_outlines(lab[0])
    with pytest.raises(ValueError):
        O.label_outlines(np.zeros((0, 4), np.int32))
    huge = np.broadcast_to(np.zeros((1, 1), np.int32), (1 << 15, 1 << 14))          # 2^29 pixels behind one stored value: the shape alone decides
    with pytest.raises(_lib.UllsamError):
        O.label_outlines(huge)
    with pytest.raises(_lib.UllsamError):
        O.label_outlines(np.broadcast_to(np.zeros((1, 1), np.int32), (1, 1 << 29)))
    empty = O.label_outlines(np.zeros((6, 5), np.int32))
    assert [tuple(t.shape) for t in empty] == [(0,), (1,), (0,), (0,), (0,), (0, 2), (0,)] and empty.start.tolist() == [0]
    assert [t.dtype for t in empty] == [torch.int32, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32]
    assert O.to_geojson(empty) == {"type": "FeatureCollection", "features": []}
