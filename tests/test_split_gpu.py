"""Splitting touching objects on the GPU (csrc/split.hip): the device route of utils.split against the host form (itself checked against the plain
loops of tests/split_ref.py without a GPU), the kernels' raw outputs through ops against those loops, the status word, the driver's split_depth.
Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance_ref as R
from tests import split_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = 2 ** 31 - 1
DEPTHS = (0, 1, 2, 32767)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _same(got, want, what):
    for name, g, w in zip(got._fields, got, want):
        assert g.is_cuda and g.dtype == torch.int32 and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), (what, name)


@pytest.fixture(scope="module")
def small():
    return R.cases() + [(f"dense blobs seed {s} {h} x {w}", R.blobs(s, h, w, n=8, ids=3)) for s, h, w in [(40, 40, 29), (43, 33, 38)]] + list(SR.shapes().items())


@pytest.fixture(scope="module")
def shapes(small):
    """The shape list of tests/test_distance_gpu.py, and two large discs that share one long border (one table slot under contention)."""
    from tests import test_distance_gpu as TD
    from ullsam_amd.utils import synthetic as S
    frame = S.label_frame(7, 300, 517, 90, (6.0, 22.0))
    odd = R.blobs(21, 37, 63, n=9)
    assert odd.size % 4 != 0
    one = TD._disc(150, 170, 70, 90, 61)
    two = np.maximum(TD._disc(150, 260, 70, 80, 61), TD._disc(150, 260, 74, 175, 61))
    assert int((one == 1).sum()) > 10000 and int((two == 1).sum()) > 20000
    return list(small) + [(f"whole rows, width {w}", TD._whole_rows(w)) for w in (63, 64, 65, 130)] + [
        ("one label over several row tiles", TD._wide()), ("H * W no multiple of 4", odd), ("label_frame 300 x 517", frame),
        ("one instance of thousands of pixels", one), ("two large discs", two)]


@pytest.fixture(scope="module")
def host(shapes):
    """{(name, edge, h): the host form's SplitLabels}: computed once, shared, never changed."""
    from ullsam_amd.utils import split as S
    return {(name, edge, h): S.split_labels(lab, h, edge=edge) for name, lab in shapes for edge in (False, True) for h in DEPTHS}


@pytest.mark.parametrize("edge", [False, True])
def test_device_route_equals_the_host_form(shapes, host, edge):
    from ullsam_amd.utils import split as S
    for name, lab in shapes:
        d = T(lab)
        for h in DEPTHS:
            _same(S.split_labels(d, h, edge=edge), host[(name, edge, h)], (name, edge, h))
        _same(S.split_labels(d, 1, edge=edge, route="global"), host[(name, edge, 1)], (name, edge, "global"))
        _same(S.split_labels(d, 1, edge=edge, route="lds"), host[(name, edge, 1)], (name, edge, "lds"))
    # (the two discs are a few rows apart: the saddle between them has a rise of its own at h = 0, which h = 1 takes away)
    assert [len(host[("two large discs", False, h)].parent) for h in (0, 1)] == [3, 2] and len(host[("label_frame 300 x 517", edge, 0)].parent) > 40


def test_numpy_labels_with_device_and_two_runs(shapes, host):
    from ullsam_amd.utils import split as S
    for name, lab in shapes:
        _same(S.split_labels(lab, 2, device=DEV), host[(name, False, 2)], (name, "numpy labels, device="))
        d = T(lab)
        a, b = S.split_labels(d, 1, edge=True), S.split_labels(d, 1, edge=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, "two runs differ")
    st = {}
    S.split_labels(T(dict(shapes)["dense blobs seed 40 40 x 29"]), 2, stats=st)
    want = {}
    S.split_labels(dict(shapes)["dense blobs seed 40 40 x 29"], 2, stats=want)
    assert st == want and st["rounds"] >= 2


def test_unaligned_base_pointer(shapes, host):
    from ullsam_amd.utils import split as S
    for name in ("H * W no multiple of 4", "whole rows, width 65", "whole rows, width 64", "one label over several row tiles", "label_frame 300 x 517"):
        lab = dict(shapes)[name]
        h, w = lab.shape
        for off in (1, 3):
            flat = torch.zeros((h * w + 8,), dtype=torch.int32, device=DEV)
            flat[off:off + h * w] = T(lab).reshape(-1)
            d = flat[off:off + h * w].view(h, w)
            assert d.is_contiguous() and d.data_ptr() % 16 != 0
            _same(S.split_labels(d, 1), host[(name, False, 1)], (name, off))


def test_contention_on_one_root_and_one_slot(shapes, host):
    from ullsam_amd.utils import split as S
    for name, parts in (("one instance of thousands of pixels", 1), ("two large discs", 2)):
        d = T(dict(shapes)[name])
        for _ in range(3):
            got = S.split_labels(d, 1)
            _same(got, host[(name, False, 1)], name)
            assert got.parent.numel() == parts


def _table(keys, vals):
    k, v = N(keys), N(vals)
    return {(int(a), int(b), int(s)) for a, b, s in zip(k[k != 0] >> 32, k[k != 0] & 0xFFFFFFFF, v[k != 0])}


def test_raw_kernel_outputs_against_the_loops(small):
    """Every ops wrapper called directly: the ascent in both routes, flatten, the pass table, rounds until rest, collect, relabel."""
    from ullsam_amd import ops
    for name, lab in small:
        h, w = lab.shape
        n, k = h * w, int(lab.max())
        d = T(lab)
        for edge in (False, True):
            d2 = R.inner_distance(lab, edge)
            dd = T(d2.astype(np.int32))
            want_up = SR.ascent(lab, d2)
            up, flags = ops.split_ascent(d, dd, k, "lds")
            assert up.dtype == torch.int32 and tuple(up.shape) == (h, w) and N(up).reshape(-1).tolist() == want_up, (name, edge, "lds")
            up, _ = ops.split_ascent(d, dd, k, "global", flags=flags)
            assert N(up).reshape(-1).tolist() == want_up, (name, edge, "global")
            rep = SR.roots(want_up)
            ops.split_flatten(up, flags=flags)
            assert N(up).reshape(-1).tolist() == rep, (name, edge, "flatten")
            keys, vals, _ = ops.split_passes(d, dd, up, 64, k, flags=flags)
            want_edges = SR.passes(lab, d2, rep)
            assert _table(keys, vals) == {(a, b, s) for (a, b), s in want_edges.items()}, (name, edge, "passes")
            assert flags.cpu().tolist() == [0, 0, len(want_edges), 0, 0, 0, 0, 0], (name, edge)
            for depth in (0, 2):
                u = up.clone()
                best = torch.zeros((n,), dtype=torch.int64, device=DEV)
                d2f = [int(v) for v in d2.reshape(-1)]
                cur = list(rep)
                for _ in range(8):
                    changed = torch.zeros((1,), dtype=torch.int32, device=DEV)
                    ops.split_round(keys, vals, d, dd, u, depth, best, changed, k, flags=flags)
                    move = SR.merge_round(want_edges, d2f, cur, depth)
                    nxt = list(cur)
                    for x, y in move.items():
                        nxt[x] = y
                    assert N(u).reshape(-1).tolist() == nxt and int(changed.cpu()) == int(bool(move)) and int(best.abs().sum()) == 0, (name, edge, depth)
                    if not move:
                        break
                    ops.split_flatten(u, flags=flags)
                    cur = SR.roots(nxt)
                    assert N(u).reshape(-1).tolist() == cur, (name, edge, depth)
                want = SR.split(lab, depth, edge)
                parts = int(ops.split_collect(d, u, None, k)[4].cpu())
                assert parts == len(want[1]), (name, edge, depth)
                lst, _ = ops.split_collect(d, u, parts, k)
                assert sorted(N(lst).tolist()) == sorted((int(l) << 32) | (y * w + x) for l, (x, y) in zip(want[1], want[3])), (name, edge, depth)
                got = ops.split_relabel(torch.sort(lst).values, d, dd, u, k)
                for g, w_ in zip(got[:5], want[:5]):
                    assert g.dtype == torch.int32 and np.array_equal(N(g), w_), (name, edge, depth)
                assert got[5].cpu().tolist() == [0] * 8


@pytest.mark.parametrize("h", sorted({t[2] for t in SR.THRESHOLDS}))
def test_one_round_on_a_hand_made_edge_list(h):
    """The shallow test at equality and where its products leave 32 bits, the greatest (S, -rep Y), key(X) < key(Y): a synthetic D2 of one row."""
    from ullsam_amd import ops
    d2, edges, want = SR.round_case(h)
    n = len(d2)
    keys = T(np.array([(a << 32) | b for a, b in edges] + [0], np.int64))     # (an empty slot among them)
    vals = T(np.array(list(edges.values()) + [0], np.int32))
    up = T(np.arange(n, dtype=np.int32).reshape(1, n))
    best = torch.zeros((n,), dtype=torch.int64, device=DEV)
    changed = torch.zeros((1,), dtype=torch.int32, device=DEV)
    flags = ops.split_round(keys, vals, T(np.ones((1, n), np.int32)), T(np.array(d2, np.int32).reshape(1, n)), up, h, best, changed, 1)
    expect = list(range(n))
    for x, y in want.items():
        expect[x] = y
    assert N(up).reshape(-1).tolist() == expect and int(changed.cpu()) == int(bool(want)) and int(best.abs().sum()) == 0
    assert flags.cpu().tolist() == [0] * 8


def test_too_many_pairs_raises_and_the_next_call_works(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import split as S
    name = "dense blobs seed 40 40 x 29"
    lab = dict(shapes)[name]
    d = T(lab)
    st = {}
    S.split_labels(d, 2, stats=st)
    assert st["pairs"] >= 4
    with pytest.raises(ops._lib.UllsamError):
        S.split_labels(d, 2, max_pairs=st["pairs"] - 2)
    _same(S.split_labels(d, 2, max_pairs=st["pairs"]), host[(name, False, 2)], "the next call")
    with pytest.raises(ops._lib.UllsamError):
        S.split_labels(d, 2, max_rounds=st["rounds"])
    _same(S.split_labels(d, 2, max_rounds=st["rounds"] + 1), host[(name, False, 2)], "the next call")


def test_a_bad_label_raises_and_the_next_call_works(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import split as S
    name = "absent ids"                                   # ids 2 and 5
    lab = dict(shapes)[name]
    neg = lab.copy()
    neg[0, 0] = -3
    neg[7, 8] = -1                                        # inside id 5
    with pytest.raises(ops._lib.UllsamError):
        S.split_labels(T(neg), 1)
    with pytest.raises(ops._lib.UllsamError):
        S.split_labels(T(lab), 1, num=4)
    d2 = T(R.inner_distance(lab, False).astype(np.int32))
    up, flags = ops.split_ascent(T(lab), d2, 4)           # the id is skipped: the others are what they would be without it
    assert flags.cpu().tolist()[0] == 1 and N(up).reshape(-1).tolist() == SR.ascent(np.where(lab == 5, 0, lab), N(d2))
    _same(S.split_labels(T(lab), 1), host[(name, False, 1)], "the next call")
    for bad in (lambda: S.split_labels(T(lab), -1), lambda: S.split_labels(T(lab), 1.5), lambda: S.split_labels(T(lab), 1, max_pairs=0),
                lambda: S.split_labels(T(lab), 1, route="fast"), lambda: S.split_labels(T(lab)[0], 1)):
        with pytest.raises(ValueError):
            bad()


def test_generate_label_map_split_depth():
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import split as SP
    from ullsam_amd.utils import synthetic as S
    from ullsam_amd.utils import amg as A
    from tests import util as U
    from tests.test_amg_gpu import _small_sam
    sam, _ = _small_sam()
    S.blob_decoder_init(sam)                                # the structured decoder: a click draws a disc around itself
    kw = dict(points_per_side=6, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05, box_nms_thresh=0.7)
    gen = SamAutomaticMaskGenerator(sam, output_mode="uncompressed_rle", **kw)
    img = np.ascontiguousarray(U.rand_image((3, 150, 200), 22, 255.0).transpose(1, 2, 0).astype(np.uint8))
    plain, recs = gen.generate_label_map(img)
    again, recs_none = gen.generate_label_map(img, split_depth=None)
    assert torch.equal(plain, again) and recs_none == recs and all("parts" not in r for r in recs) and int(plain.max()) >= 3
    want = SP.split_labels(plain, 2, num=int(plain.max()))
    labels, recs2 = gen.generate_label_map(img, split_depth=2)
    assert labels.is_cuda and torch.equal(labels, want.labels)
    assert [{k: v for k, v in r.items() if k != "parts"} for r in recs2] == recs
    parent = want.parent.cpu().tolist()
    for r in recs2:
        assert r["parts"] == [i + 1 for i, p in enumerate(parent) if p == r["label"] and p > 0], r["label"]
    small, _ = gen.generate_label_map(img, split_depth=2, out_hw=(75, 120), window=(5, 10, 60, 100))
    assert torch.equal(small.cpu(), A.resize_labels_nearest(want.labels.cpu(), (75, 120), (5, 10, 60, 100)))
    _, _, table = gen.generate_label_map(img, split_depth=2, measure=True)
    assert int(table.area.numel()) == len(parent) and int(table.area.sum()) == int((labels > 0).sum())
    for bad in (-1, 1.0, True, 40000):
        with pytest.raises(ValueError):
            gen.generate_label_map(img, split_depth=bad)
