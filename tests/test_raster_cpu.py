"""Polygons to label images without a GPU: the numpy form of utils.raster (row ranges, a scan, one key per crossing, a sort, spans) against the plain
loops of tests/raster_ref.py (Fractions, one counter per label and pixel), the round trip through utils.outline and GeoJSON, the sums
measure_instances knows, the header, the errors.  Integer work: every assertion is equality."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import outline_ref as OR
from tests import raster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONN = (8, 4)
SYMBOLS = ("ullsam_raster_scan", "ullsam_raster_edges", "ullsam_raster_keys", "ullsam_raster_covered", "ullsam_raster_paint", "ullsam_raster_finish")


def N(t):
    return t.numpy().astype(np.int64)


def run(c, **kw):
    from ullsam_amd.utils import raster as RA
    return RA.rasterize_polygons(c["vertices"], c["start"], c["ring_label"], c["size"], c["order"], c["num"], **kw)


@pytest.fixture(scope="module")
def cases():
    return R.cases()


@pytest.fixture(scope="module")
def loops(cases):
    """{name: the plain loops' answer}: computed once, shared, never changed."""
    return {name: R.rasterize(c["vertices"], c["start"], c["ring_label"], c["size"], c["order"], c["num"]) for name, c in cases.items()}


@pytest.fixture(scope="module")
def host(cases):
    return {name: run(c) for name, c in cases.items()}


@pytest.fixture(scope="module")
def images():
    from ullsam_amd.utils import synthetic as S
    return list(OR.shapes().items()) + [("label_frame 120 x 157", S.label_frame(7, 120, 157, 30, (6.0, 14.0)))]


def test_host_form_equals_the_plain_loops(cases, loops, host):
    for name, c in cases.items():
        got, want = host[name], loops[name]
        for f in R.FIELDS:
            g, w = getattr(got, f), getattr(want, f)
            assert not g.is_cuda and g.dtype == torch.int32 and tuple(g.shape) == w.shape and np.array_equal(N(g), w), (name, f)
        assert tuple(got.labels.shape) == tuple(c["size"]), name


def test_the_cases_are_what_they_claim(cases, loops, host):
    lab = lambda name: N(host[name].labels)
    d = lab("diamond")                                   # a centre on a left or top edge is inside, on a right or bottom edge outside
    rows = [(int(np.flatnonzero(r)[0]), int(r.sum())) if r.any() else None for r in d]
    assert rows == [None, (3, 2), (2, 4), (1, 6), (0, 8), (1, 6), (2, 4), (3, 2), None, None]
    assert all(np.array_equal(np.flatnonzero(r), np.arange(r.sum()) + np.flatnonzero(r)[0]) for r in d if r.any())
    want = np.zeros((11, 9), np.int64)
    want[3:8, 2:7] = 1                                    # integer corners: exactly x0..x1 - 1, y0..y1 - 1
    assert np.array_equal(lab("integer rectangle"), want)
    tri = lab("triangle: a vertex on a scanline, one on a centre")
    assert tri[2].sum() == 0 and tri[4].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0]    # the apex on a centre has no width; the vertex on row 4's line counts once
    assert tri.sum() == N(host["triangle: a vertex on a scanline, one on a centre"].covered)[0] > 10
    ring = np.zeros((13, 14), np.int64)
    ring[1:12, 1:12] = 1
    ring[4:9, 4:8] = 0
    assert np.array_equal(lab("hole, same orientation"), ring) and np.array_equal(lab("hole, other orientation"), ring)
    bow = lab("bow-tie")
    assert bow[1].tolist() == bow[7].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0] and bow[4].tolist() == [0] + [1] * 8 + [0]   # two lobes that meet in (5, 4.5)
    assert bow[0].sum() == bow[8].sum() == 0 and np.array_equal(bow, bow[::-1]) and np.array_equal(bow, bow[:, ::-1])
    twice = host["a ring twice cancels"]
    assert N(twice.covered).tolist() == [0, 6] and (lab("a ring twice cancels") == 1).sum() == 0
    sides = host["out of every side, and outside"]
    assert N(sides.covered).tolist() == [6, 6, 9, 6, 0, 0] and N(sides.box).tolist()[:4] == [[0, 2, 1, 4], [4, 0, 6, 1], [9, 3, 11, 5], [5, 8, 7, 9]]
    assert N(sides.box).tolist()[4:] == [[R.INT_MAX, R.INT_MAX, -1, -1]] * 2
    by_label, by_area = host["overlaps, by label"], host["overlaps, by area"]
    assert N(by_label.covered).tolist() == N(by_area.covered).tolist() == [25, 25, 48]
    assert N(by_label.labels)[5, 5] == 3 and N(by_area.labels)[5, 5] == 2 and N(by_area.labels)[3, 3] == 1    # 3 is the largest: at the bottom; the tie: 2 over 1
    assert N(by_label.area).tolist() == [9, 5, 48] and N(by_area.area).tolist() == [21, 25, 16]
    absent = host["absent ids"]
    assert absent.covered.numel() == 7 and N(absent.covered)[[0, 2, 3, 5, 6]].tolist() == [0] * 5 and N(absent.covered)[1] == 12 and N(absent.covered)[4] > 8
    assert lab("1 x 1").tolist() == [[1]] and lab("1 x 17").shape == (1, 17) and lab("23 x 1").shape == (23, 1)
    assert lab("1 x 17")[0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 0, 1]
    assert lab("23 x 1")[:, 0].tolist() == [2] * 5 + [0] * 2 + [1] * 12 + [0] * 4      # the triangle narrows to the right of the one centre column
    for name, k in (("no rings", 0), ("no rings, num = 3", 3)):
        got = host[name]
        assert not got.labels.any() and [tuple(t.shape) for t in got] == [tuple(cases[name]["size"]), (k,), (k,), (k, 4)], name
    assert N(host["no rings, num = 3"].box).tolist() == [[R.INT_MAX, R.INT_MAX, -1, -1]] * 3


def test_a_shared_edge_is_watertight(cases, host):
    c, got = cases["cut rectangle"], host["cut rectangle"]
    h, w = c["size"]
    assert len(c["vertices"]) == 2 * 40 + 4 and not np.array_equal(c["vertices"] * 256, np.round(c["vertices"] * 256))
    assert int(got.covered.sum()) == h * w and torch.equal(got.area, got.covered) and int((got.labels == 0).sum()) == 0
    assert min(N(got.covered).tolist()) > 100


@pytest.mark.parametrize("conn", CONN)
def test_outlines_and_back(images, conn):
    """label_outlines -> rasterize_polygons returns the label image, straight and through a GeoJSON text with a pixel size and an origin."""
    from ullsam_amd.utils import outline as O
    from ullsam_amd.utils import raster as RA
    assert len(images) == 15
    for name, lab in images:
        out = O.label_outlines(lab, conn)
        k = int(lab.max())
        back = RA.rasterize_polygons(out.vertices, out.start, out.label, lab.shape, num=k)
        assert np.array_equal(N(back.labels), lab), (name, conn)
        text = json.dumps(O.to_geojson(out, 0.325, (1234.5, -77.25)))
        again = RA.labels_from_geojson(json.loads(text), lab.shape, 0.325, (1234.5, -77.25), num=k)
        assert np.array_equal(N(again.labels), lab) and all(torch.equal(a, b) for a, b in zip(again, back)), (name, conn)
        assert np.array_equal(N(back.covered), np.bincount(lab.reshape(-1), minlength=k + 1)[1:]) and torch.equal(back.area, back.covered), (name, conn)


def test_area_and_box_equal_measure_instances(cases, host, images):
    from ullsam_amd.utils import measure as M
    for name, c in cases.items():
        got = host[name]
        k = got.covered.numel()
        if not k:
            continue
        table = M.measure_instances(got.labels, num=k)
        assert np.array_equal(N(got.area), N(table.area)) and np.array_equal(N(got.box), N(table.box)), name


def test_from_geojson():
    from ullsam_amd.utils import raster as RA
    sq = [[1.0, 1.0], [5.0, 1.0], [5.0, 4.0], [1.0, 4.0], [1.0, 1.0]]
    hole = [[2.0, 2.0], [2.0, 3.0], [3.0, 3.0], [3.0, 2.0], [2.0, 2.0]]
    tri = [[6.0, 6.0], [9.0, 6.0], [6.0, 9.0]]                                       # not closed: nothing is stripped
    fc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "id": 9, "properties": {"label": 4, "name": "a"}, "geometry": {"type": "Polygon", "coordinates": [sq, hole]}},
        {"type": "Feature", "id": 2, "properties": {"name": "b"}, "geometry": {"type": "MultiPolygon", "coordinates": [[tri], [sq]]}},
        {"type": "Feature", "properties": None, "geometry": {"type": "Polygon", "coordinates": [tri]}}]}
    v, start, label, props = RA.from_geojson(fc)
    assert v.dtype == np.float64 and v.shape == (4 + 4 + 3 + 4 + 3, 2) and start.tolist() == [0, 4, 8, 11, 15, 18] and label.tolist() == [4, 4, 2, 2, 3]
    assert start.dtype == np.int32 and label.dtype == np.int32 and v[:4].tolist() == sq[:4] and v[8:11].tolist() == tri
    assert props == [{}, {"name": "b"}, {}, {"label": 4, "name": "a"}]
    v2, _, label2, _ = RA.from_geojson(fc, pixel_size=0.5, origin=(1.0, -1.0), label_key="cell")
    assert v2[:2].tolist() == [[0.0, 4.0], [8.0, 4.0]] and label2.tolist() == [9, 9, 2, 2, 3]          # no such key: the id, else the place
    one = RA.from_geojson(fc["features"][0])
    assert one[1].tolist() == [0, 4, 8] and one[2].tolist() == [4, 4]
    geom = RA.from_geojson({"type": "MultiPolygon", "coordinates": [[sq, hole]]})
    assert geom[1].tolist() == [0, 4, 8] and geom[2].tolist() == [1, 1] and geom[3] == [{}]
    got = RA.labels_from_geojson(fc, (10, 10))
    want = np.zeros((10, 10), np.int64)
    want[6, 6:8], want[7, 6] = 3, 3                                                   # the triangle twice: label 2's copy under label 3's; a centre on the slanted (right) edge is outside
    want[1:4, 1:5] = 4                                                                # label 2's square under label 4's ...
    want[2, 2] = 2                                                                    # ... and seen through its hole
    assert np.array_equal(N(got.labels), want) and N(got.covered).tolist() == [0, 15, 3, 11]
    empty = RA.from_geojson({"type": "FeatureCollection", "features": []})
    assert empty[0].shape == (0, 2) and empty[1].tolist() == [0] and empty[2].shape == (0,) and empty[3] == []
    assert not RA.labels_from_geojson({"type": "FeatureCollection", "features": []}, (3, 4)).labels.any()
    for bad in ({"type": "Point", "coordinates": [1, 2]}, {"type": "Feature", "geometry": {"type": "LineString", "coordinates": [[0, 0], [1, 1]]}}, [sq],
                {"type": "Feature", "properties": {"label": "x"}, "geometry": {"type": "Polygon", "coordinates": [sq]}}):
        with pytest.raises(ValueError):
            RA.from_geojson(bad)
    with pytest.raises(ValueError):
        RA.from_geojson(fc, pixel_size=0.0)


def test_inputs_and_errors(cases, host):
    from ullsam_amd import _lib
    from ullsam_amd.utils import raster as RA
    c = cases["absent ids"]
    want = host["absent ids"]
    v, s, l = c["vertices"], c["start"], c["ring_label"]
    for form in ((torch.from_numpy(v), torch.from_numpy(s), torch.from_numpy(l)), (v.tolist(), s.tolist(), l.tolist()), (v.astype(np.float32) * 1.0, s.astype(np.int64), l)):
        got = RA.rasterize_polygons(*form, c["size"], num=7, device="cpu")
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    ints = RA.rasterize_polygons(np.array(R.rect(2, 3, 7, 8), np.int32), [0, 4], [1], (11, 9))          # integer vertices: times 256, no rounding
    assert torch.equal(ints.labels, host["integer rectangle"].labels)
    assert [t.dtype for t in want] == [torch.int32] * 4
    for bad in (dict(ring_label=[2, 8]), dict(ring_label=[0, 5]), dict(ring_label=[-1, 5]), dict(num=4), dict(vertices=np.where(v == v.max(), 65535.6, v)),
                dict(vertices=np.where(v == v.max(), -65536.0, v)), dict(ring_label=[2, 70000], num=None)):
        kw = dict(vertices=v, start=s, ring_label=l, size=c["size"], num=7)
        kw.update(bad)
        with pytest.raises(_lib.UllsamError):
            RA.rasterize_polygons(**kw)
    edge = RA.rasterize_polygons(np.where(v == v.max(), 65535.0, v), s, l, c["size"], num=7)           # the range's last value is inside it
    assert int(edge.covered[1]) == 12
    nan = v.copy()
    nan[3, 0] = np.nan
    inf = v.copy()
    inf[0, 1] = np.inf
    for bad in (dict(vertices=nan), dict(vertices=inf), dict(start=[0, 2, 8]), dict(start=[0, 5, 4, 8]), dict(start=[1, 4, 8]), dict(start=[0, 4, 7]),
                dict(start=[0, 4, 8, 8]), dict(start=[]), dict(ring_label=[2]), dict(size=(10, 0)), dict(size=(0, 12)), dict(size=(32768, 4)), dict(size=(4, 32768)),
                dict(size=(10.0, 12)), dict(size=10), dict(order="record"), dict(order=None), dict(num=-1), dict(num=65536), dict(num=7.0), dict(num=True),
                dict(vertices=v.reshape(-1)), dict(vertices=np.zeros((8, 3))), dict(paint="lanes")):
        kw = dict(vertices=v, start=s, ring_label=l, size=c["size"], num=7)
        kw.update(bad)
        with pytest.raises(ValueError):
            RA.rasterize_polygons(**kw)
    big = RA.rasterize_polygons(np.array(R.rect(1, 1, 3, 32766.5), np.float64), [0, 4], [65535], (32767, 4), num=65535)   # both limits themselves
    assert int(big.covered[-1]) == 2 * 32765 and N(big.box)[-1].tolist() == [1, 1, 2, 32765] and big.covered.numel() == 65535


def _arg_count(decl):
    return len([a for a in decl.split(",") if a.strip()])


def test_header_declares_the_raster_entry_points_and_the_abi_stays_14():
    from ullsam_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(ullsam_raster_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(SYMBOLS) == sorted(s for s in _lib.SIGNATURES if s.startswith("ullsam_raster_"))
    for s in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code)
        assert m and _arg_count(m.group(1)) == len(_lib.SIGNATURES[s]), s
        assert re.search(r"\b%s:" % s.replace("ullsam_", ""), src.split("int ullsam_raster_scan")[0]), f"{s}: no comment states what it computes"
        assert callable(getattr(ops, s.replace("ullsam_", "")))
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", src).group(1)) == 14 == _lib.ABI_VERSION
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.ullsam_abi_version() == 14
    assert os.path.exists(os.path.join(ROOT, "ullsam_amd", "csrc", "raster.hip"))
    with pytest.raises(_lib.UllsamError):                 # the kernels' wrappers take GPU tensors only; the host form lives in utils.raster
        ops.raster_scan(torch.zeros((4,), dtype=torch.int32))
