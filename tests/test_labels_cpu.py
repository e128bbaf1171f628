"""Instance label maps without a GPU: the host forms of utils.amg (the definition the device path is tested against) against the numpy
definitions of tests/labels_ref.py, instance_scores against brute-force matching on hand-made tables, the nearest rule against PIL, and
the C ABI's declarations.  Integer work: every comparison is equality."""
import os
import re

import numpy as np
import pytest
import torch

from tests import labels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ullsam_rle_paint_labels", "ullsam_label_stats", "ullsam_label_compact", "ullsam_label_remap", "ullsam_label_overlap",
           "ullsam_resize_nearest_i32")


def check_paint(got, want, name):
    for g, w_, what in zip(got, want, ("labels", "label_of_record", "areas", "boxes")):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.shape == w_.shape and np.array_equal(g, w_), f"{name}: {what}"


@pytest.mark.parametrize("hw", R.FRAMES)
def test_host_paint_label_map_is_the_sequential_overwrite(hw):
    from ullsam_amd.utils import amg as A
    h, w = hw
    for name, masks, order, keys, mva in R.paint_cases(h, w):
        rles = [R.mask_to_rle(m) for m in masks]
        got = A.paint_label_map(rles, order=order, keys=keys, min_visible_area=mva, device="cpu", size=(h, w))
        assert all(g.dtype == torch.int32 and not g.is_cuda for g in got)
        check_paint(got, R.paint(masks, (h, w), order, keys, mva), f"{hw} {name}")


def test_host_paint_orders_and_errors():
    from ullsam_amd import _lib
    from ullsam_amd.utils import amg as A
    h, w = 4, 6
    small = np.zeros((h, w), bool); small[1:3, 1:3] = True
    big = np.ones((h, w), bool)
    rles = [R.mask_to_rle(small), R.mask_to_rle(big)]
    lab, of_rec, areas, boxes = A.paint_label_map(rles, order="record")              # the app's order: the later, larger record hides the first
    assert of_rec.tolist() == [0, 1] and areas.tolist() == [24] and boxes.tolist() == [[0, 0, 5, 3]] and int(lab.min()) == 1
    lab, of_rec, areas, boxes = A.paint_label_map(rles, order="area")                # large first: the small one stays on top, as label 2
    assert of_rec.tolist() == [2, 1] and areas.tolist() == [20, 4] and boxes.tolist() == [[0, 0, 5, 3], [1, 1, 2, 2]]
    assert A.paint_ranks(rles, "score", [0.9, 0.1]).tolist() == [1, 0] and A.paint_ranks(rles, "score", [0.5, 0.5]).tolist() == [0, 1]
    lab, of_rec, areas, _ = A.paint_label_map(rles, order="area", min_visible_area=5)   # the dropped record's pixels become 0, not the big one's
    assert of_rec.tolist() == [0, 1] and areas.tolist() == [20] and int((lab == 0).sum()) == 4
    with pytest.raises(ValueError):
        A.paint_label_map(rles, order="score")
    with pytest.raises(ValueError):
        A.paint_label_map(rles, order="size")
    with pytest.raises(ValueError):
        A.paint_label_map([])
    for counts in ([5, -1, h * w - 4], [h * w + 5], [3, h * w + 2]):
        with pytest.raises(_lib.UllsamError):
            A.paint_label_map([rles[0], {"size": [h, w], "counts": counts}])
    with pytest.raises(_lib.UllsamError):
        A.paint_label_map([rles[0], {"size": [h, w + 1], "counts": [h * (w + 1)]}])


def _label_pair(h, w, na, nb, seed):
    """Two label images cut into seeded rectangles, ids up to na / nb with some declared ids absent."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (na, nb):
        x = np.zeros((h, w), np.int32)
        for _ in range(min(n, 40)):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            x[y0:y0 + rng.integers(1, h // 3 + 2), x0:x0 + rng.integers(1, w // 3 + 2)] = rng.integers(1, n + 1) if n else 0
        out.append(x)
    return out


@pytest.mark.parametrize("hw", [(33, 65), (96, 160)])
def test_host_label_overlap_matches_add_at(hw):
    from ullsam_amd import _lib
    from ullsam_amd.utils import amg as A
    h, w = hw
    for na in (0, 1, 300):
        for nb in (0, 1, 300):
            a, b = _label_pair(h, w, na, nb, 31 * na + nb)
            want, skipped = R.overlap(a, b, na, nb)
            assert skipped == 0 and want.sum() == h * w
            got = A.label_overlap(a, b, na, nb)
            assert got.dtype == np.int64 and got.shape == (na + 1, nb + 1) and np.array_equal(got, want)
            got_t = A.label_overlap(torch.from_numpy(a), torch.from_numpy(b), na, nb)
            assert isinstance(got_t, torch.Tensor) and np.array_equal(got_t.numpy(), want)
            auto = A.label_overlap(a, b)                                          # na / nb from the images: the table is a corner of the declared one
            assert np.array_equal(auto, want[:auto.shape[0], :auto.shape[1]]) and auto.sum() == h * w
    a, b = _label_pair(h, w, 5, 5, 1)
    a[0, 0] = 6
    with pytest.raises(_lib.UllsamError):
        A.label_overlap(a, b, 5, 5)
    with pytest.raises(_lib.UllsamError):
        A.label_overlap(a, b, 2 ** 13, 2 ** 13)                                   # more than 2^26 cells


THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))


def _check_scores(got, table, thresholds=THRESHOLDS):
    want = R.scores(table, thresholds)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), v), (k, got[k], v)


def test_instance_scores_against_brute_force():
    from ullsam_amd.utils import instances as I
    assert I.DEFAULT_THRESHOLDS == THRESHOLDS
    # a pair at IoU exactly 0.5 (2 / (3 + 3 - 2)): no match at t = 0.5; a perfect pair; a pair at 0.75; ids 3 (pred) and 4 (gt) declared, absent
    pred = np.array([[1, 1, 1, 0, 2, 2, 5, 5, 5, 5, 0, 0]], np.int32)
    gt = np.array([[0, 1, 1, 1, 2, 2, 3, 3, 3, 0, 0, 0]], np.int32)
    table = R.overlap(pred, gt, 5, 4)[0]
    assert table[1, 1] == 2 and table.sum(1)[1] == 3 and table.sum(0)[1] == 3
    s = I.instance_scores(pred, gt)
    _check_scores(s, table)
    assert s["n_pred"] == 3 and s["n_gt"] == 3                                     # present ids only
    assert s["tp"].tolist() == [2, 2, 2, 2, 2, 1, 1, 1, 1, 1] and s["fp"][0] == 1 and s["fn"][0] == 1
    assert s["ap"][0] == 2 / 4 and s["f1"][0] == 4 / 6 and s["mean_matched_iou"][0] == (1.0 + 0.75) / 2 and s["mean_matched_iou"][-1] == 1.0
    _check_scores(I.scores_from_table(table, (0.5, 0.75, 1.0)), table, (0.5, 0.75, 1.0))   # IoU == 0.75 is no match at t = 0.75 either
    # empty prediction, empty ground truth, both
    zero = np.zeros_like(gt)
    for p, g in ((zero, gt), (pred, zero), (zero, zero)):
        s = I.instance_scores(torch.from_numpy(p), torch.from_numpy(g))
        _check_scores(s, R.overlap(p, g, int(p.max()), int(g.max()))[0])
        assert s["tp"].sum() == 0 and s["f1"].sum() == 0 and s["precision"].sum() == 0 and s["recall"].sum() == 0
    # seeded label pairs, and an image against itself
    rng = np.random.default_rng(5)
    a, b = _label_pair(40, 50, 12, 9, 3)
    b2 = np.where(rng.random(a.shape) < 0.1, 0, a).astype(np.int32)                # a with a tenth of its pixels erased: most pairs match
    for p, g in ((a, b), (a, b2)):
        _check_scores(I.instance_scores(p, g), R.overlap(p, g, int(p.max()), int(g.max()))[0])
    s = I.instance_scores(a, a)
    assert (s["f1"] == 1).all() and (s["mean_matched_iou"] == 1).all() and (s["ap"] == 1).all()
    for bad in ((0.4,), (0.5, 0.49), (float("nan"),)):
        with pytest.raises(ValueError):
            I.instance_scores(a, b, thresholds=bad)


CASES_RESIZE = [((3, 5), (7, 4), None), ((64, 64), (100, 37), None), ((9, 11), (9, 11), None), ((64, 48), (100, 37), (13, 5, 50, 20)),
                ((5, 1), (7, 1), None), ((7, 3), (5, 2), (1, 1, 4, 1))]


def test_host_resize_labels_nearest_is_the_integer_rule():
    from ullsam_amd import _lib
    from ullsam_amd.utils import amg as A
    rng = np.random.default_rng(2)
    for ihw, ohw, win in CASES_RESIZE:
        x = rng.integers(0, 2 ** 31 - 1, ihw).astype(np.int32)                    # ids above 65535 survive
        got = A.resize_labels_nearest(x, ohw, win)
        assert got.dtype == np.int32 and np.array_equal(got, R.nearest(x, ohw, win))
        assert np.array_equal(A.resize_labels_nearest(torch.from_numpy(x), ohw, win).numpy(), got)
    assert np.array_equal(A.nearest_source_index(7, 5), [0, 1, 1, 2, 3, 3, 4]) and np.array_equal(A.nearest_source_index(5, 7), [0, 2, 3, 4, 6])
    with pytest.raises(_lib.UllsamError):
        A.resize_labels_nearest(np.zeros((4, 4), np.int32), (8, 8), (4, 0, 5, 8))


def test_resize_labels_nearest_equals_pil_nearest():
    from ullsam_amd.utils import amg as A
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("PIL is not installed: the rule is checked against its integer definition only")
    rng = np.random.default_rng(4)
    for ihw, ohw in (((5, 5), (7, 7)), ((7, 7), (5, 5)), ((5, 7), (7, 5)), ((64, 48), (100, 37))):
        x = rng.integers(0, 65536, ihw).astype(np.uint16)
        want = np.asarray(Image.fromarray(x).resize((ohw[1], ohw[0]), Image.NEAREST))
        got = A.resize_labels_nearest(x, ohw)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (ihw, ohw)


def test_header_declares_the_label_entry_points_and_the_abi_is_14():
    from ullsam_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert s in _lib.SIGNATURES
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", src).group(1)) == 14 == _lib.ABI_VERSION
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.ullsam_abi_version() == 14
    for fn in ("rle_paint_labels", "label_stats", "label_compact", "label_remap", "label_overlap", "resize_nearest_i32"):
        assert callable(getattr(ops, fn))
    with pytest.raises(_lib.UllsamError):                                          # the kernels' wrappers take GPU tensors only; the host forms live in utils.amg
        ops.label_overlap(torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32), 0, 0)
