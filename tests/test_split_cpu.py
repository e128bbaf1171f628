"""utils.split without a GPU: the numpy host form against the plain loops of tests/split_ref.py, hand-made objects with their part counts, the shallow
test at equality, the properties the definition promises, the ABI, the kernels' resources, argument errors.  Integer work: every assertion is equality."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import distance_ref as R
from tests import split_ref as SR
from ullsam_amd import _lib
from ullsam_amd.utils import distance as D
from ullsam_amd.utils import split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1
DEPTHS = (0, 1, 2, 32767)


def N(t):
    return t.numpy().astype(np.int64)


def _equal(got, want, what):
    assert isinstance(got, S.SplitLabels) and all(t.dtype == torch.int32 for t in got), what
    for name, g, w in zip(got._fields, got, want):
        assert tuple(g.shape) == tuple(w.shape) and np.array_equal(N(g), w), (what, name)


@pytest.fixture(scope="module")
def cases():
    """distance_ref's cases (14 random images with sides 1..40, H = 1, W = 1 and 1 x 1 among them, and the named ones), denser random images whose
    instances have several basins, and the hand-made objects."""
    dense = [(f"dense blobs seed {s} {h} x {w}", R.blobs(s, h, w, n=8, ids=3)) for s, h, w in [(40, 40, 29), (43, 33, 38), (40, 24, 40), (46, 33, 38)]]
    return R.cases() + dense + list(SR.shapes().items())


@pytest.fixture(scope="module")
def reference(cases):
    """{(name, edge, h): split_ref.split}: computed once, shared, never changed."""
    return {(name, edge, h): SR.split(lab, h, edge) for name, lab in cases for edge in (False, True) for h in DEPTHS}


def test_the_cases_cover_what_they_should(cases, reference):
    shapes = [lab.shape for name, lab in cases if name.startswith("blobs")]
    assert len(shapes) >= 14 and (1, 1) in shapes and any(h == 1 and w > 1 for h, w in shapes) and any(w == 1 and h > 1 for h, w in shapes)
    rounds = [r[5] for r in reference.values()]
    assert max(rounds) >= 2 and min(rounds) == 0                                  # the merge loop runs more than once somewhere
    assert any(len(r[1]) > len(reference[(k[0], k[1], 32767)][1]) for k, r in reference.items() if k[2] == 0)      # h matters


@pytest.mark.parametrize("edge", [False, True])
def test_host_form_against_the_loops(cases, reference, edge):
    for name, lab in cases:
        for h in DEPTHS:
            _equal(S.split_labels(lab, h, edge=edge), reference[(name, edge, h)], (name, edge, h))


def _parts(lab, h, **kw):
    return int(S.split_labels(lab, h, **kw).parent.numel())


def test_hand_made_objects():
    sh = SR.shapes()
    assert [_parts(sh["two overlapping discs"], h) for h in (0, 1, 2)] == [2, 2, 2]
    for name in ("one disc", "a rectangle", "a tilted ellipse"):
        assert _parts(sh[name], 1) == 1, name
    assert _parts(sh["a tilted ellipse"], 0) == 3                                # the staircase of a tilted edge: separate rises at h = 0
    assert [_parts(sh["a dumbbell"], h) for h in (0, 1, 2)] == [2, 2, 2]
    assert [_parts(sh["one id in two pieces"], h) for h in DEPTHS] == [2, 2, 2, 2]
    lab = sh["a U-shaped plateau"]                                               # D2 = 4 along the whole centre line
    d2 = N(D.inner_distance(lab))
    up = np.array(SR.ascent(lab, d2))
    roots = [p for p in range(lab.size) if up[p] == p and lab.reshape(-1)[p] > 0]
    assert len(roots) > 1 and {int(d2.reshape(-1)[p]) for p in roots} == {4}
    got = S.split_labels(lab, 0)                                                 # P = S: t = 0 at h = 0
    assert got.parent.tolist() == [1] and got.peak_r2.tolist() == [4] and np.array_equal(N(got.labels), lab)


def test_nothing_crosses_a_border_between_labels():
    lab = SR.shapes()["two labels side by side"]
    for h in DEPTHS:
        got = S.split_labels(lab, h)
        assert got.parent.tolist() == [1, 2] and got.parts_of.tolist() == [1, 1] and np.array_equal(N(got.labels), lab), h


def test_frame_filling_label():
    lab = np.full((7, 10), 1, np.int32)
    for h in DEPTHS:
        got = S.split_labels(lab, h)                                             # all INF: one plateau, joined through P = S
        assert got.parent.tolist() == [1] and got.peak_r2.tolist() == [INF] and got.peak_xy.tolist() == [[0, 0]] and np.array_equal(N(got.labels), lab)
    assert S.split_labels(lab, 0, edge=True).peak_xy.tolist() == [[3, 3]]


def test_no_labelled_pixel_and_absent_ids():
    got = S.split_labels(np.zeros((6, 5), np.int32), 1)
    assert [tuple(t.shape) for t in got] == [(6, 5), (0,), (0,), (0, 2), (0,)] and int(got.labels.abs().sum()) == 0
    lab = dict(R.named_cases())["absent ids"]                                    # ids 2 and 5
    got = S.split_labels(lab, 1, num=7)
    assert got.parts_of.tolist() == [0, 1, 0, 0, 1, 0, 0] and got.parent.tolist() == [2, 5]
    assert np.array_equal(N(got.labels), np.where(lab == 2, 1, np.where(lab == 5, 2, 0)))


def test_shallow_at_equality():
    for p, s, h, fires in SR.THRESHOLDS:
        assert S.shallow(p, s, h) == SR.shallow(p, s, h) == fires, (p, s, h)
        assert fires == (np.sqrt(np.longdouble(p)) - np.sqrt(np.longdouble(s)) <= h + (1e-12 if fires else -1e-12)), (p, s, h)
    assert S.shallow(9, 4, 1) and not S.shallow(10, 4, 1)


@pytest.mark.parametrize("h", sorted({t[2] for t in SR.THRESHOLDS}))
def test_one_round_on_a_hand_made_edge_list(h):
    d2, edges, want = SR.round_case(h)
    for (p, s, hh, fires), y in zip([t for t in SR.THRESHOLDS if t[2] == h], range(0, 1000, 2)):
        assert (want.get(y + 1) == y) == fires, (p, s, h)
    ea, eb = (np.array([k[i] for k in edges], np.int64) for i in (0, 1))
    x, y = S._round_host(ea, eb, np.array(list(edges.values()), np.int64), np.array(d2, np.int64), np.arange(len(d2), dtype=np.int64), h)
    assert dict(zip(x.tolist(), y.tolist())) == want


def test_properties(cases):
    try:
        import scipy.ndimage as ndi                                               # connectivity is checked where scipy is installed
    except ImportError:
        ndi = None
    eight = np.ones((3, 3), int)
    for name, lab in cases:
        k = int(lab.max())
        components = sum(ndi.label(lab == i, structure=eight)[1] for i in range(1, k + 1)) if ndi else None
        d2 = N(D.inner_distance(lab))
        for h in DEPTHS:
            got = S.split_labels(lab, h)
            out, parent, r2, xy, parts_of = (N(t) for t in got)
            kk = len(parent)
            assert np.array_equal(out > 0, lab > 0) and sorted(set(out[out > 0].tolist())) == list(range(1, kk + 1)), (name, h)      # a partition
            assert np.array_equal(np.concatenate([[0], parent])[out], lab), (name, h)
            assert np.array_equal(parts_of, np.bincount(parent, minlength=k + 1)[1:k + 1]), (name, h)
            reps = xy[:, 1] * lab.shape[1] + xy[:, 0]
            order = list(zip(parent.tolist(), reps.tolist()))
            assert order == sorted(order) and len(set(order)) == kk, (name, h)
            for i in range(kk):
                m = out == i + 1
                assert ndi is None or ndi.label(m, structure=eight)[1] == 1, (name, h, i)                                           # every part is 8-connected
                first = np.flatnonzero((d2 == d2[m].max()) & m)[0]                                                     # the first row-major maximum
                assert r2[i] == d2[m].max() and reps[i] == first, (name, h, i)
            assert ndi is None or (kk >= components and (h < 32767 or kk == components)), (name, h)                                   # h = 32767: the components


def test_errors_and_routing():
    lab = R.blobs(5, 12, 12)
    for labels in (lab, torch.from_numpy(lab), torch.from_numpy(lab.astype(np.int64))):
        got = S.split_labels(labels, 1, device="cpu")
        assert not got.labels.is_cuda and np.array_equal(N(got.labels), N(S.split_labels(lab, 1).labels))
    bad = lab.copy()
    bad[0, 0] = -1
    for call in (lambda: S.split_labels(lab[0], 1), lambda: S.split_labels(np.zeros((0, 4), np.int32), 1), lambda: S.split_labels(lab, -1),
                 lambda: S.split_labels(lab, 32768), lambda: S.split_labels(lab, 1.0), lambda: S.split_labels(lab, True), lambda: S.split_labels(bad, 1),
                 lambda: S.split_labels(lab, 1, max_pairs=0), lambda: S.split_labels(lab, 1, max_pairs=2 ** 30 + 1), lambda: S.split_labels(lab, 1, max_rounds=0),
                 lambda: S.split_labels(lab, 1, route="fast"), lambda: S.split_labels(lab, 1, num=int(lab.max()) - 1), lambda: S.split_labels(lab, 1, num=-1)):
        with pytest.raises(ValueError):
            call()
    dense = R.blobs(40, 40, 29, n=8, ids=3)
    st = {}
    S.split_labels(dense, 2, stats=st)
    assert st["pairs"] >= 2 and st["rounds"] >= 1 and st["basins"] > st["parts"] >= 1
    with pytest.raises(_lib.UllsamError):
        S.split_labels(dense, 2, max_pairs=st["pairs"] - 1)
    S.split_labels(dense, 2, max_pairs=st["pairs"], max_rounds=st["rounds"] + 1)
    with pytest.raises(_lib.UllsamError):
        S.split_labels(dense, 2, max_rounds=st["rounds"])                          # the last round allowed must come to rest


def test_abi_and_symbols():
    from ullsam_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert _lib.ABI_VERSION == 14 == lib.ullsam_abi_version() == int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1))
    names = ["ullsam_split_ascent", "ullsam_split_flatten", "ullsam_split_passes", "ullsam_split_round", "ullsam_split_collect", "ullsam_split_relabel"]
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("ullsam_split_")) == sorted(names)
    for s in names:
        assert hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s


def test_split_kernels_have_no_spill_and_no_scratch():
    from ullsam_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels()
    for pat in KR.HOT_SPLIT:
        assert pat in KR.HOT_BF16
    hot = {n: r for n, r in ks.items() if any(re.search(h, n) for h in KR.HOT_SPLIT)}
    assert len(hot) == 9, sorted(hot)                                             # eight kernels, the ascent in both routes
    for n, r in hot.items():
        assert not (r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)), (n, r)
    lds = [r.get("group_segment_fixed_size", 0) for n, r in hot.items() if "split_ascent_kernelILb1E" in n]
    assert lds == [2 * 4 * 66 * 6]                                               # labels and D2 of 64 x 4 pixels and their halo
