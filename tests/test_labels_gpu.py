"""Instance label maps on the GPU (csrc/labels.hip): paint / stats / compact / remap against the host form of utils.amg.paint_label_map (itself
checked against tests/labels_ref.py without a GPU), the overlap table against np.add.at, the nearest resize against the integer rule, and
SamAutomaticMaskGenerator.generate_label_map.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import labels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(got, want, name):
    for g, w_, what in zip(got, want, ("labels", "label_of_record", "areas", "boxes")):
        assert g.dtype == torch.int32 and g.shape == w_.shape and torch.equal(g.cpu(), w_), f"{name}: {what}"


@pytest.mark.parametrize("hw", R.FRAMES)
def test_paint_label_map_matches_the_host_form(hw):
    """Every record set x order x min_visible_area of the frame (tests/labels_ref.paint_cases): the four kernels against the sequential overwrite,
    and a second run against the first, bit for bit."""
    from ullsam_amd.utils import amg as A
    h, w = hw
    for name, masks, order, keys, mva in R.paint_cases(h, w):
        rles = [R.mask_to_rle(m) for m in masks]
        want = A.paint_label_map(rles, order=order, keys=keys, min_visible_area=mva, device="cpu", size=(h, w))
        got = A.paint_label_map(rles, order=order, keys=keys, min_visible_area=mva, device=DEV, size=(h, w))
        assert all(g.is_cuda for g in got) and tuple(got[0].shape) == (h, w)
        _same(got, want, f"{hw} {name}")
        again = A.paint_label_map(rles, order=order, keys=keys, min_visible_area=mva, device=DEV, size=(h, w))
        assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{hw} {name}: two runs differ"


def test_paint_kernels_step_by_step():
    """The four entry points one after the other through their ops wrappers, each output against numpy: the transposed raw labels, the stats per
    raw label, the compaction tables, the remapped image."""
    from ullsam_amd import ops
    from ullsam_amd.utils import amg as A
    h, w = 65, 33
    masks = R.record_sets(h, w)["mixed"]
    n = len(masks)
    rles = [R.mask_to_rle(m) for m in masks]
    rank = A.paint_ranks(rles, "area")
    flat, offs, _, _ = A._rle_concat(rles, "test")
    raw, status = ops.rle_paint_labels(T(flat), T(offs), T(rank), h, w)
    assert raw.shape == (w, h) and not status.any()
    want_raw = np.zeros((h, w), np.int32)
    for r, i in enumerate(np.argsort(rank)):
        want_raw[masks[i]] = r + 1
    assert np.array_equal(raw.cpu().numpy().T, want_raw)
    areas_raw, boxes_raw = ops.label_stats(raw, n)
    a_np, b_np = areas_raw.cpu().numpy(), boxes_raw.cpu().numpy()
    for v in range(1, n + 1):
        ys, xs = np.nonzero(want_raw == v)
        assert a_np[v] == len(ys)
        assert b_np[v].tolist() == ([xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [2 ** 31 - 1, 2 ** 31 - 1, -1, -1])
    assert a_np[0] == 0
    mva = int(np.median(a_np[1:][a_np[1:] > 0])) + 1
    lmap, of_record, areas, boxes, k = ops.label_compact(areas_raw, boxes_raw, T(rank), mva)
    keep = (a_np != 0) & (a_np >= mva)
    want_map = np.cumsum(keep) * keep
    kk = int(k.item())
    assert kk == keep.sum() and 0 < kk < (a_np > 0).sum() and np.array_equal(lmap.cpu().numpy(), want_map)
    assert np.array_equal(of_record.cpu().numpy(), want_map[rank + 1]) and np.array_equal(areas.cpu().numpy()[:kk], a_np[keep])
    assert np.array_equal(boxes.cpu().numpy()[:kk], b_np[keep])
    labels = ops.label_remap(raw, lmap)
    assert labels.shape == (h, w) and np.array_equal(labels.cpu().numpy(), want_map[want_raw])


def test_paint_flags_malformed_counts_and_stays_inside_the_frame():
    """One record with a negative count and one whose counts sum to H * W + 5, among good ones: status flags exactly those, the wrapper raises, and
    the guard values around the output (a view inside a larger buffer) are intact -- the kernel clips every access to the frame by construction."""
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import amg as A
    h, w = 33, 65
    good = R.mask_to_rle(R.record_sets(h, w)["nested"][0])
    negative = {"size": [h, w], "counts": [10, -3, 20, h * w - 27]}
    long_ = {"size": [h, w], "counts": [h * w - 40, 45]}
    rles = [good, negative, good, long_, good]
    flat, offs, _, _ = A._rle_concat(rles, "test")
    guard, pad = -123456789, 4096
    buf = torch.full((pad + h * w + pad,), guard, dtype=torch.int32, device=DEV)
    out = buf[pad:pad + h * w].view(w, h)
    raw, status = ops.rle_paint_labels(T(flat), T(offs), T(np.arange(5, dtype=np.int32)), h, w, out=out)
    assert status.cpu().tolist() == [0, 1, 0, 1, 0]
    assert bool((buf[:pad] == guard).all()) and bool((buf[pad + h * w:] == guard).all())
    r = raw.cpu().numpy()
    assert r.min() >= 0 and r.max() <= 5 and r.reshape(-1)[-40:].tolist() == [4] * 40      # the in-range part of the long record is painted (the last good record lies elsewhere)
    _, status = ops.rle_paint_labels(T(flat), T(offs), T(np.array([0, 1, 7, 3, -1], np.int32)), h, w)   # a rank outside 0..N-1 is flagged and paints nothing
    assert status.cpu().tolist() == [0, 1, 1, 1, 1]
    with pytest.raises(_lib.UllsamError):
        A.paint_label_map(rles, device=DEV)
    with pytest.raises(_lib.UllsamError):
        A.paint_label_map([good, {"size": [h, w + 1], "counts": [h * (w + 1)]}], device=DEV)


def _label_pair(h, w, na, nb, seed):
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
def test_label_overlap_matches_add_at(hw):
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import amg as A
    h, w = hw
    for na in (0, 1, 300):
        for nb in (0, 1, 300):
            a, b = _label_pair(h, w, na, nb, 31 * na + nb)                        # ids up to na / nb declared, most of 1..300 absent
            want, _ = R.overlap(a, b, na, nb)
            table, status = ops.label_overlap(T(a), T(b), na, nb)
            assert table.dtype == torch.int64 and table.shape == (na + 1, nb + 1) and int(status.item()) == 0
            assert np.array_equal(table.cpu().numpy(), want) and int(table.sum()) == h * w
            assert torch.equal(A.label_overlap(T(a), T(b), na, nb), table)
            assert torch.equal(A.label_overlap(a, T(b), na, nb), table) and torch.equal(A.label_overlap(T(a), torch.from_numpy(b), na, nb), table)   # one image on the host: it follows the other
            again, _ = ops.label_overlap(T(a), T(b), na, nb)
            assert torch.equal(again, table)
    a, b = _label_pair(h, w, 300, 300, 9)
    a[h // 2, w // 2], b[0, 0], a[h - 1, w - 1] = 301, -1, 2 ** 31 - 1            # ids outside the declared ranges: flagged, skipped
    want, skipped = R.overlap(a, b, 300, 300)
    table, status = ops.label_overlap(T(a), T(b), 300, 300)
    assert int(status.item()) == 1 and skipped == 3 and np.array_equal(table.cpu().numpy(), want) and int(table.sum()) == h * w - 3
    with pytest.raises(_lib.UllsamError):
        A.label_overlap(T(a), T(b), 300, 300)
    with pytest.raises(_lib.UllsamError):
        ops.label_overlap(T(a), T(b), 2 ** 13, 2 ** 13)
    auto = A.label_overlap(T(np.abs(b)), T(np.abs(b)))                            # na / nb from the images; an image against itself is diagonal
    assert tuple(auto.shape) == (int(np.abs(b).max()) + 1,) * 2
    assert int(auto.sum()) == h * w and int(torch.diagonal(auto).sum()) == h * w


def test_resize_nearest_is_the_integer_rule():
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import amg as A
    rng = np.random.default_rng(3)
    for ihw, ohw, win in (((3, 5), (7, 4), None), ((64, 64), (100, 37), None), ((9, 11), (9, 11), None), ((64, 48), (100, 37), (13, 5, 50, 20)),
                          ((40, 300), (17, 700), (0, 150, 17, 550)), ((1, 1), (5, 3), (2, 1, 3, 2))):
        x = rng.integers(0, 2 ** 31 - 1, ihw).astype(np.int32)                    # int32 ids above 65535 survive
        want = R.nearest(x, ohw, win)
        got = ops.resize_nearest_i32(T(x), ohw, win)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (ihw, ohw, win)
        assert torch.equal(A.resize_labels_nearest(T(x), ohw, win), got)
        assert np.array_equal(A.resize_labels_nearest(x, ohw, win), want)
    with pytest.raises(_lib.UllsamError):
        ops.resize_nearest_i32(T(np.zeros((4, 4), np.int32)), (8, 8), (0, 4, 8, 5))


def test_generate_label_map_paints_the_generators_records():
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import amg as A
    from ullsam_amd.utils import instances as I
    from tests import util as U
    from tests.test_amg_gpu import _small_sam
    sam, _ = _small_sam()
    img = torch.from_numpy(U.rand_image((3, 150, 200), 22, 255.0))
    kw = dict(points_per_side=6, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05, box_nms_thresh=1.0)     # (no box suppression: the random decoder's masks overlap heavily, so many records end up hidden)
    gen = SamAutomaticMaskGenerator(sam, output_mode="uncompressed_rle", **kw)
    gen_bin = SamAutomaticMaskGenerator(sam, **kw)                                # the default output_mode: generate_label_map's records do not follow it
    before = gen.generate(img)
    before_bin = gen_bin.generate(img)
    assert len(before) >= 3
    for g, order in ((gen, "area"), (gen_bin, "score"), (gen, "record")):
        labels, records = g.generate_label_map(img, order=order, min_visible_area=3)
        assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (150, 200)
        assert [{k: v for k, v in r.items() if k != "label"} for r in records] == before and all("label" in r for r in records)
        rles = [r["segmentation"] for r in records]
        keys = [r["predicted_iou"] for r in records] if order == "score" else None
        want, of_record, areas, _ = A.paint_label_map(rles, order=order, keys=keys, min_visible_area=3, device="cpu")
        assert torch.equal(labels.cpu(), want) and [r["label"] for r in records] == of_record.tolist()
        assert int(labels.max()) == len(areas) > 0
        s = I.instance_scores(labels, labels)
        assert (s["f1"] == 1).all() and (s["mean_matched_iou"] == 1).all() and s["n_pred"] == len(areas)
    small, _ = gen.generate_label_map(img, out_hw=(75, 120), window=(5, 10, 60, 100))
    full, _ = gen.generate_label_map(img)
    assert torch.equal(small.cpu(), A.resize_labels_nearest(full.cpu(), (75, 120), (5, 10, 60, 100)))
    after, after_bin = gen.generate(img), gen_bin.generate(img)                  # generate() returns what it returned before
    assert after == before and len(after_bin) == len(before_bin)
    for x, y in zip(after_bin, before_bin):
        assert np.array_equal(x["segmentation"], y["segmentation"]) and {k: v for k, v in x.items() if k != "segmentation"} == {k: v for k, v in y.items() if k != "segmentation"}
