"""Simplified outlines without a GPU: the numpy form of utils.simplify against the plain definition of tests/simplify_ref.py (recursive
Douglas-Peucker on fractions), and the three facts of DESIGN.md "7b, continued (simplifying)": tolerance 0, the guarantee, watertightness.  Integer
work: every comparison with the reference is equality."""
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import outline_ref as R
from tests import simplify_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONN = (8, 4)
TS = (0, 128, 256, 640)
FIELDS = R.FIELDS
DTYPES = (torch.int32, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32)
SYMBOLS = ("ullsam_simplify_flags", "ullsam_simplify_candidates", "ullsam_simplify_anchors", "ullsam_simplify_segments", "ullsam_simplify_rounds",
           "ullsam_simplify_rings")


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _equal(res, ref, what):
    for name, g, dt in zip(FIELDS, res.outlines, DTYPES):
        want = getattr(ref, name)
        assert g.dtype == dt and tuple(g.shape) == tuple(want.shape) and np.array_equal(N(g), want), (what, name)
    assert res.source.dtype == torch.int32 and np.array_equal(N(res.source), ref.source), (what, "source")


@pytest.fixture(scope="module")
def images():
    return SR.all_images()


@pytest.fixture(scope="module")
def refs(images):
    """{(name, connectivity, T): the plain definition's result}: computed once, shared, never changed."""
    return {(name, c, t): SR.simplify(lab, t, c) for name, lab in images.items() for c in CONN for t in TS}


def simplify(lab, t, c=8, **kw):
    from ullsam_amd.utils import simplify as S
    return S.simplify_outlines(lab, t / 256, c, **kw)


@pytest.mark.parametrize("c", CONN)
def test_the_numpy_form_equals_the_plain_definition(images, refs, c):
    for name, lab in images.items():
        for t in TS:
            _equal(simplify(lab, t, c), refs[(name, c, t)], (name, c, t))
    big = refs[("spiral 64 x 64", c, 256)]
    assert len(big.cands[0]) > 100 and sum(len(r.source) < len(r.src.label) for r in refs.values()) > 10      # long loops, and loops that drop


@pytest.mark.parametrize("c", CONN)
def test_tolerance_zero_keeps_label_outlines_vertices(images, c):
    for name, lab in images.items():
        SR.check_tolerance_zero(simplify(lab, 0, c), lab, c)


@pytest.mark.parametrize("c", CONN)
def test_every_candidate_lies_within_the_tolerance(images, refs, c):
    for name, lab in images.items():
        for t in TS:
            SR.check_guarantee(simplify(lab, t, c), refs[(name, c, t)], t)


@pytest.mark.parametrize("c", CONN)
def test_shared_borders_are_watertight(images, refs, c):
    shared = 0
    for name, lab in images.items():
        for t in TS:
            shared += SR.check_watertight(refs[(name, c, t)], lab)
    assert shared > 2000
    for name in ("a tiling without background 41 x 39", "a frame-filling instance 7 x 10"):
        lab = images[name]
        assert lab.min() > 0
        for t in TS:
            res = simplify(lab, t, c)
            assert len(res.source) == len(R.outlines(lab, c).label), "nothing drops here: the result holds every ring"
            inner = SR.check_reversal(res.outlines, *lab.shape)
            assert inner > 20 or name.startswith("a frame")
    wavy = simplify(images["two labels on a wavy border"], 256, c).outlines
    seg = SR.segments_of(wavy)
    assert sum(1 for (p, q) in seg if (q, p) in seg) >= 4               # the border of 1 and 2 is there, in both directions


def test_a_loop_runs_straight_through_a_junction(images, refs):
    lab = images["a T-junction passed straight"]
    ref = refs[("a T-junction passed straight", 8, 640)]
    assert SR.is_fixed(lab, 6, 4) and (6, 4) in ref.cands[0] and (6, 4) not in SR._rows(R.outlines(lab))[0]     # a candidate of loop 1, no corner of it
    rows = SR._rows(simplify(lab, 640).outlines)
    assert all((6, 4) in r for r in rows) and len(rows) == 3


def test_tied_farthest_anchors(images, refs):
    lab = images["tied farthest anchors"]
    cand = refs[("tied farthest anchors", 8, 0)].cands[0]
    d = sorted(((x - 1) ** 2 + (y - 1) ** 2, -y, -x) for x, y in cand)
    assert d[-1][0] == d[-2][0] == d[-3][0] == 50                       # three candidates tie; the smallest (y, x) is (8, 2)
    rows = SR._rows(simplify(lab, 255 * 256).outlines)                  # at the largest tolerance only what no rule removes is left
    assert rows == [] and refs[("tied farthest anchors", 8, 640)].rings[0][0] == cand.index((1, 1))
    ring = [cand[i] for i in SR.simplify(lab, 255 * 256).rings[0]]
    assert ring == [(1, 1), (8, 2)]


def test_a_loop_with_one_fixed_point(images, refs):
    lab = images["loops with one fixed point"]
    ref = refs[("loops with one fixed point", 4, 256)]
    assert len(ref.cands) == 2 and all(sum(SR.is_fixed(lab, *p) for p in c) == 1 for c in ref.cands)
    rows = SR._rows(simplify(lab, 256, 4).outlines)
    assert len(rows) == 2 and all((4, 4) in r and len(r) == 4 for r in rows)
    one = refs[("loops with one fixed point", 8, 256)]                 # connectivity 8: one loop that passes the saddle twice
    assert len(one.cands) == 1 and one.cands[0].count((4, 4)) == 2


def test_the_threshold_is_strict(images):
    lab = images["a bump at distance 1"]
    at = lambda t: SR._rows(simplify(lab, t).outlines)[0]
    assert sorted(at(256)) == [(1, 1), (1, 4), (13, 1), (13, 4)]       # a bump at exactly the tolerance goes
    assert (6, 5) in at(255) and len(at(255)) == 5                      # just below it, its first corner in (y, x) order stays


def test_equal_distances_go_to_the_smaller_yx(images, refs):
    lab = images["two equal bumps on a shared border"]
    rows = SR._rows(simplify(lab, 200).outlines)
    assert len(rows) == 2 and all((4, 5) in r and (12, 5) not in r for r in rows)           # (mirror images of each other)
    SR.check_watertight(SR.simplify(lab, 200), lab)
    inner = [s for s in SR.segments_of(simplify(lab, 200).outlines) if s[0][1] >= 4 and s[1][1] >= 4 and s[0][1] <= 5 and s[1][1] <= 5]
    assert all((q, p) in inner for p, q in inner) and len(inner) >= 4


def test_the_distance_cases_and_the_64_bit_bounds():
    from ullsam_amd.utils import simplify as S
    m = 32767
    pts = [((5, 5), (0, 0), (0, 0)), ((-3, 1), (0, 0), (7, 0)), ((9, 2), (0, 0), (7, 0)), ((3, 2), (0, 0), (7, 0)), ((0, m), (m, 0), (0, 0)),
           ((m, m), (0, 0), (m, 0)), ((0, m), (m, m), (0, 0)), ((m, 0), (0, m), (0, m)), ((0, 0), (m, m), (m, m - 1)), ((m, 0), (0, 0), (0, m))]
    rng = np.random.default_rng(3)
    pts += [tuple(tuple(int(v) for v in rng.integers(0, m + 1, 2)) for _ in range(3)) for _ in range(300)]
    pts += [tuple(tuple(int(v) for v in rng.integers(0, 6, 2)) for _ in range(3)) for _ in range(300)]
    arr = np.array(pts, np.int64)
    num, den = S._num_host(arr[:, 0, 0], arr[:, 0, 1], arr[:, 1, 0], arr[:, 1, 1], arr[:, 2, 0], arr[:, 2, 1])
    cases = set()
    for (p, a, b), n, d in zip(pts, num.tolist(), den.tolist()):
        length = (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
        t = (p[0] - a[0]) * (b[0] - a[0]) + (p[1] - a[1]) * (b[1] - a[1])
        cases.add("zero" if length == 0 else "before" if t <= 0 else "after" if t >= length else "inside")
        assert d == (length or 1) and 0 <= n < 2 ** 62 and Fraction(n, d) == SR.dist2(p, a, b), (p, a, b)
        assert (255 * 256) ** 2 * d < 2 ** 63
    assert cases == {"zero", "before", "after", "inside"} and int(num.max()) > 2 ** 59


def test_candidates_beyond_the_chords_ends(images, refs):
    """Both outer cases of the distance occur among the candidates the recursion measures on these images, and the numpy form equals the plain
    definition on exactly them."""
    seen = set()
    for name in ("candidates beyond the chord's ends", "spiral 64 x 64", "noise 24 x 31"):
        ref = refs[(name, 8, 640)]
        _equal(simplify(images[name], 640), ref, name)
        for cand, ring in zip(ref.cands, ref.rings):
            n = len(cand)
            for i, j in zip(ring, ring[1:] + [ring[0] + n]):
                a, b = cand[i], cand[j % n]
                length = (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
                for m in range(i + 1, j):
                    t = (cand[m % n][0] - a[0]) * (b[0] - a[0]) + (cand[m % n][1] - a[1]) * (b[1] - a[1])
                    seen.add("before" if t <= 0 else "after" if t >= length else "inside")
    assert seen == {"before", "after", "inside"}, seen


def test_dropped_loops(images, refs):
    cell = simplify(images["a 2 x 1 cell"], 512)                        # the ring has two vertices
    assert cell.source.numel() == 0 and cell.outlines.loops_of.tolist() == [0] and cell.outlines.start.tolist() == [0]
    assert tuple(cell.outlines.vertices.shape) == (0, 2) and simplify(images["a 2 x 1 cell"], 128).source.tolist() == [0]
    lab = images["a hole whose parent drops"]
    assert R.outlines(lab).parent.tolist() == [0, 0] and simplify(lab, 128).source.tolist() == [0, 1]
    assert simplify(lab, 768).source.numel() == 0                       # the outer ring has two vertices (here the hole's ring degenerates as well)
    lab = images["a valid hole whose parent drops"]
    for c in CONN:
        ref = SR.simplify(lab, 7 * 256, c)
        assert ref.src.label.tolist()[:2] == [1, 1] and ref.src.parent.tolist()[:2] == [0, 0] and ref.src.area2.tolist()[:2] == [120, -8]
        outer, hole = ([ref.cands[i][j] for j in ref.rings[i]] for i in (0, 1))
        area2 = lambda r: sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(r, r[1:] + r[:1]))
        assert outer == [(13, 8), (8, 8), (3, 8)] and area2(outer) == 0                   # the parent: three collinear fixed points
        assert hole == [(7, 5), (8, 6), (9, 5)] and area2(hole) == -2                     # the hole alone is valid: 3 vertices, the source's strict sign
        res = simplify(lab, 7 * 256, c)
        _equal(res, ref, c)
        assert res.source.tolist() == [2, 3, 5, 6] and res.outlines.parent.tolist() == [0, 1, 2, 3]   # gone by the parent rule alone (4 collapses by itself)
        assert simplify(lab, 128, c).source.tolist() == list(range(7))
    lab = images["three collinear fixed points"]
    ref = SR.simplify(lab, 512)
    one = list(ref.src.label).index(1)
    assert [ref.cands[one][i] for i in ref.rings[one]] == [(9, 3), (6, 3), (3, 3)]       # area2 = 0
    res = simplify(lab, 512)
    assert one not in res.source.tolist() and res.outlines.loops_of.tolist() == [0, 1, 1] and res.outlines.label.tolist() == [2, 3]
    assert res.outlines.parent.tolist() == [0, 1]


def test_a_one_row_frame_of_full_width():
    lab = np.ones((1, 32767), np.int32)
    lab[0, 20000:] = 2
    lab[0, 30000] = 0
    for t in (0, 256, 255 * 256):
        _equal(simplify(lab, t), SR.simplify(lab, t), t)
    assert SR._rows(simplify(lab, 0).outlines)[0] == [(0, 0), (20000, 0), (20000, 1), (0, 1)]


def test_argument_errors(images):
    from ullsam_amd import _lib
    from ullsam_amd.utils import simplify as S
    lab = images["absent ids"]
    bad = [lambda: S.simplify_outlines(lab, -0.01), lambda: S.simplify_outlines(lab, 255.01), lambda: S.simplify_outlines(lab, float("nan")),
           lambda: S.simplify_outlines(lab, "1"), lambda: S.simplify_outlines(lab, True), lambda: S.simplify_outlines(lab, 1, connectivity=6),
           lambda: S.simplify_outlines(lab[0], 1), lambda: S.simplify_outlines(np.zeros((1, 32768), np.int32), 1),
           lambda: S.simplify_outlines(np.zeros((0, 4), np.int32), 1), lambda: S.simplify_outlines(lab, 1, num=-1)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(_lib.UllsamError):
        S.simplify_outlines(lab, 1, num=4)
    neg = lab.copy()
    neg[0, 0] = -2
    with pytest.raises(_lib.UllsamError):
        S.simplify_outlines(neg, 1)
    assert S.simplify_outlines(lab, 255).source.numel() >= 0 and S.simplify_outlines(lab, 0.001).outlines.vertices.shape[0] == 8   # T snaps to 0
    assert S._tolerance(0.5) == 128 and S._tolerance(1 / 512) == 1 and S._tolerance(np.float32(2)) == 512 and S._tolerance(3) == 768
    got = S.simplify_outlines(torch.from_numpy(lab), 1, num=7)
    assert got.outlines.loops_of.tolist() == [0, 1, 0, 0, 1, 0, 0] and not got.outlines.vertices.is_cuda


def test_geojson_round_trip(images):
    from ullsam_amd.utils import outline as O
    from ullsam_amd.utils import raster as RS
    for name in ("noise 24 x 31", "a tiling without background 41 x 39", "nested rings 9 x 9"):
        res = simplify(images[name], 256)
        doc = json.loads(json.dumps(O.to_geojson(res.outlines)))
        assert doc["type"] == "FeatureCollection" and [f["id"] for f in doc["features"]] == (np.flatnonzero(N(res.outlines.loops_of)) + 1).tolist()
        for f in doc["features"]:
            polys = O.polygons(res.outlines, f["id"])
            assert len(f["geometry"]["coordinates"]) == len(polys)
            for coords, (ext, holes) in zip(f["geometry"]["coordinates"], polys):
                assert len(coords) == 1 + len(holes) and all(r[0] == r[-1] and len(r) >= 4 for r in coords)
                assert np.array_equal(np.array(coords[0][:-1]), ext)
        verts, start, ring_label, _ = RS.from_geojson(doc)              # the same rings, grouped by polygon: exterior, then its holes
        rows = SR._rows(res.outlines)
        back = [[tuple(int(c) for c in v) for v in np.asarray(verts)[a:b]] for a, b in zip(np.asarray(start)[:-1], np.asarray(start)[1:])]
        assert sorted(back) == sorted(rows) and sorted(np.asarray(ring_label).tolist()) == sorted(N(res.outlines.label).tolist())


def test_c_abi_and_bindings():
    from ullsam_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ullsam_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ullsam_simplify_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(SYMBOLS) == sorted(s for s in _lib.SIGNATURES if s.startswith("ullsam_simplify_"))
    for s in SYMBOLS:
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, src, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[s]), s
        assert hasattr(ops, s[len("ullsam_"):])
    assert _lib.ABI_VERSION == 14 and "#define ULLSAM_ABI_VERSION 14" in open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    with pytest.raises((_lib.UllsamError, TypeError, ValueError)):
        ops.simplify_flags(torch.zeros((4, 4), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32), torch.zeros((0,), dtype=torch.uint8))
