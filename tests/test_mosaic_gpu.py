"""The label-map mosaic on the GPU (csrc/mosaic.hip): the device route against the host form of utils.mosaic.stitch_label_maps (itself checked
against the loops of tests/mosaic_ref.py without a GPU), the kernels one by one through ops against numpy and a dictionary union-find, the
status flags, and SamAutomaticMaskGenerator.generate_tiled_label_map.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import mosaic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("labels", "label_of_global", "areas", "boxes")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    large = R.truth_case("many workgroups", *R.LARGE, 11, 150, (4.0, 40.0))
    return R.cases() + [large, dict(large, name="many workgroups, min_visible_area", mva=300)]


def _stitch(case, device, **kw):
    from ullsam_amd.utils import mosaic as M
    args = dict(iou=case["iou"], min_visible_area=case["mva"])
    args.update(kw)
    tiles = T(case["tiles"]) if device == DEV else case["tiles"]
    return M.stitch_label_maps(tiles, case["counts"], M.tile_grid(*case["grid"]), device=device, **args)


def test_device_route_equals_the_host_form(cases):
    for case in cases:
        want = _stitch(case, "cpu")
        got = _stitch(case, DEV)
        for g, w_, what in zip(got, want, NAMES):
            assert g.is_cuda and g.dtype == torch.int32 and g.shape == w_.shape and torch.equal(g.cpu(), w_), f"{case['name']}: {what}"
        again = _stitch(case, DEV)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{case['name']}: two runs differ"


def _device_inputs(case):
    from ullsam_amd.utils import mosaic as M
    grid = M.tile_grid(*case["grid"])
    base = np.concatenate([[0], np.cumsum(case["counts"])]).astype(np.int32)
    return grid, base, T(case["tiles"]), T(base), int(base[-1])


def test_seam_kernel_pairs_and_areas(cases):
    """The pair table, read back and sorted by key, and the [G + 1, 4] in-seam areas against the per-pixel loops."""
    from ullsam_amd import ops
    from ullsam_amd.utils import mosaic as M
    for case in (cases[0], cases[1], cases[9]):
        grid, base, tiles, base_d, g = _device_inputs(case)
        seams = M.seam_table(grid)
        keys, counts, areas, flags = ops.mosaic_seams(tiles, base_d, g, T(seams), int(seams[:, 6].max()), 4096)
        want_pairs, want_areas = R.seam_counts(case["tiles"], base, grid)
        k, c = keys.cpu().numpy().view(np.uint64), counts.cpu().numpy()
        assert keys.numel() == 8192 and (c[k == 0] == 0).all()
        got = sorted((int(x) >> 63, (int(x) >> 32) & 0x7fffffff, int(x) & 0xffffffff, int(n)) for x, n in zip(k[k != 0], c[k != 0]))
        assert got == sorted((d, a, b, n) for (d, a, b), n in want_pairs.items()) and len(got) > 0, case["name"]
        dense = np.zeros((g + 1, 4), np.int32)
        for (gid, side), n in want_areas.items():
            dense[gid, side] = n
        assert np.array_equal(areas.cpu().numpy(), dense), case["name"]
        assert flags.cpu().tolist()[:3] == [0, 0, len(got)]


def _pair_keys(pairs):
    return T(np.asarray([(a << 32) | b for a, b in pairs], np.int64).reshape(-1))


def test_union_find_kernel_on_hand_made_pairs():
    from ullsam_amd import ops
    rng = np.random.default_rng(5)
    n = 4096
    chain = [(i, i + 1) for i in range(1, n)]
    star = [(int(c), 77) for c in rng.permutation(np.arange(1, 300)) if c != 77]
    two = [(1, 2), (2, 3), (10, 11), (11, 12), (3, 1), (12, 10), (3, 2), (1, 3)]          # pairs already in one component, both ways round
    lists = {
        "chain reversed": (chain[::-1], n),
        "chain shuffled": ([chain[i] for i in rng.permutation(len(chain))], n),
        "chain, larger id first": ([(b, a) for a, b in chain], n),
        "star": (star, 300),
        "duplicated pairs": ([p for p in chain[:200] for _ in range(3)] + star[:50] * 2, 300),
        "already joined": (two, 12),
        "no pairs": ([], 5),
    }
    for name, (pairs, g) in lists.items():
        want = R.representatives(pairs, g)
        keys = _pair_keys(pairs) if pairs else torch.zeros((4,), dtype=torch.int64, device=DEV)     # (an empty slot is skipped)
        parent, flags = ops.mosaic_union(keys, g)
        assert parent.dtype == torch.int32 and np.array_equal(parent.cpu().numpy(), want), name
        assert not flags.cpu().numpy().any()
        again, _ = ops.mosaic_union(keys, g)
        assert torch.equal(parent, again), name
    assert np.array_equal(R.representatives(chain, n), np.concatenate([[0], np.ones(n, np.int64)]))
    _, flags = ops.mosaic_union(_pair_keys([(1, 2), (3, 9)]), 8)                            # an id above G: flagged, nothing is indexed with it
    assert flags.cpu().tolist()[0] == 1


@pytest.mark.parametrize("hwto", [(129, 131, 33, 7), (150, 170, 64, 16), (40, 50, 64, 16), (256, 512, 128, 32)])
def test_paste_equals_the_slicing_expression(hwto):
    """Odd core widths and unaligned left edges (tile 33, overlap 7) and 16-byte aligned rows (tile 128): with the identity table the paste is the
    cores copied as they are; with a random table it is the table applied to them; a guard band around the frame stays intact."""
    from ullsam_amd import ops
    from ullsam_amd.utils import mosaic as M
    grid = M.tile_grid(*hwto)
    rng = np.random.default_rng(9)
    counts = rng.integers(1, 50, grid.ntiles)
    tiles = np.stack([rng.integers(0, k + 1, (grid.th, grid.tw)) for k in counts]).astype(np.int32)
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    g = int(base[-1])
    cores = M.core_table(grid)
    glob = np.where(tiles > 0, tiles + base[:-1, None, None], 0)
    for table in (np.arange(g + 1, dtype=np.int32), rng.integers(0, 1000, g + 1).astype(np.int32)):
        table[0] = 0                                                               # (the background is not looked up: it stays 0)
        for shift in (0, 1):                                                       # shift 1: the frame starts 4 bytes off a 16-byte boundary
            guard, pad = -123456789, 1024
            buf = torch.full((pad + grid.H * grid.W + pad,), guard, dtype=torch.int32, device=DEV)
            out = buf[pad + shift:pad + shift + grid.H * grid.W].view(grid.H, grid.W)
            got = ops.mosaic_paste(T(tiles), T(base), g, T(cores), int(cores[:, 2].max()), T(table), grid.H, grid.W, out=out)
            assert np.array_equal(got.cpu().numpy(), R.paste(table[glob], grid))
            assert bool((buf[:pad + shift] == guard).all()) and bool((buf[pad + shift + grid.H * grid.W:] == guard).all())


def test_stats_and_compaction_kernels():
    from ullsam_amd import ops
    from ullsam_amd.utils import mosaic as M
    case = R.truth_case("stats", 150, 170, 64, 16, 21, 40, (3.0, 14.0), hand=True)
    grid, base, tiles, base_d, g = _device_inputs(case)
    pairs, _ = R.seam_counts(case["tiles"], base, grid)
    rep = R.representatives([(a, b) for (_, a, b) in pairs], g)                    # (cut from one truth: every pair of the seams is one instance)
    cores = M.core_table(grid)
    areas_raw, boxes_raw, flags = ops.mosaic_stats(tiles, base_d, g, T(cores), int(cores[:, 2].max()), T(rep.astype(np.int32)), grid.H, grid.W)
    glob = np.where(case["tiles"] > 0, case["tiles"] + base[:-1, None, None], 0)
    raw = R.paste(rep[glob].astype(np.int32), grid)
    a_np, b_np = areas_raw.cpu().numpy(), boxes_raw.cpu().numpy()
    for v in range(1, g + 1):
        ys, xs = np.nonzero(raw == v)
        assert a_np[v] == len(ys)
        assert b_np[v].tolist() == ([xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [2 ** 31 - 1, 2 ** 31 - 1, -1, -1])
    assert a_np[0] == 0 and not flags.cpu().numpy().any()
    mva = int(np.median(a_np[a_np > 0])) + 1
    log, areas, boxes, k = ops.mosaic_compact(areas_raw, boxes_raw, T(rep.astype(np.int32)), mva)
    keep = (a_np != 0) & (a_np >= mva)
    lmap = np.cumsum(keep) * keep
    kk = int(k.item())
    assert kk == keep.sum() and 0 < kk < (a_np > 0).sum() and np.array_equal(log.cpu().numpy(), lmap[rep])
    assert np.array_equal(areas.cpu().numpy()[:kk], a_np[keep]) and np.array_equal(boxes.cpu().numpy()[:kk], b_np[keep])


def test_status_flags_raise_and_leave_the_process_usable(cases):
    """An id outside 0..K_t (in a seam, and in a core only) and more distinct pairs than max_pairs are CHECKED inputs: they set a status word,
    index nothing out of bounds, and the next call works."""
    from ullsam_amd import _lib
    case = cases[0]
    for where, value in (((4, 5, 5), None), ((4, 30, 30), -7), ((0, 2, 60), 2 ** 31 - 1)):
        bad = dict(case, tiles=case["tiles"].copy())
        bad["tiles"][where] = case["counts"][where[0]] + 1 if value is None else value
        with pytest.raises(_lib.UllsamError):
            _stitch(bad, DEV)
    with pytest.raises(_lib.UllsamError):
        _stitch(case, DEV, max_pairs=4)                                             # far more pairs than the table is allowed to take
    two = {c["name"]: c for c in cases}["threshold(1, 2)"]
    with pytest.raises(_lib.UllsamError):
        _stitch(two, DEV, max_pairs=1)
    with pytest.raises(_lib.UllsamError):
        _stitch(two, DEV, max_pairs=2)                                              # three distinct pairs
    for g, w_ in zip(_stitch(two, DEV, max_pairs=3), _stitch(two, "cpu")):
        assert torch.equal(g.cpu(), w_)
    for g, w_ in zip(_stitch(case, DEV), _stitch(case, "cpu")):
        assert torch.equal(g.cpu(), w_)


def test_generate_tiled_label_map_stitches_the_tiles_label_maps():
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import mosaic as M
    from ullsam_amd.utils import synthetic as S
    from tests import util as U
    from tests.test_amg_gpu import _small_sam
    sam, _ = _small_sam()
    S.blob_decoder_init(sam)                                                       # the structured decoder: a click draws a disc around itself
    kw = dict(points_per_side=6, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05, box_nms_thresh=0.7)
    gen = SamAutomaticMaskGenerator(sam, output_mode="uncompressed_rle", **kw)
    img = np.ascontiguousarray(U.rand_image((3, 176, 176), 23, 255.0).transpose(1, 2, 0))
    tile, overlap = 96, 16
    grid = M.tile_grid(176, 176, tile, overlap)
    assert grid.ntiles == 4 and len(grid.seams()) == 4
    labels, records = gen.generate_tiled_label_map(img, tile=tile, overlap=overlap, min_visible_area=3)
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (176, 176)
    per_tile = [gen.generate_label_map(img[top:top + h, left:left + w]) for top, left, h, w in grid.boxes()]
    counts = [int(l.max()) for l, _ in per_tile]
    assert sum(counts) >= 4
    want, log, areas, _ = M.stitch_label_maps(torch.stack([l.cpu() for l, _ in per_tile]), counts, grid, min_visible_area=3, device="cpu")
    assert torch.equal(labels.cpu(), want) and int(labels.max()) == len(areas)
    base = np.concatenate([[0], np.cumsum(counts)])
    flat = [(t, r) for t, (_, recs) in enumerate(per_tile) for r in recs]
    assert len(records) == len(flat)
    for got, (t, r) in zip(records, flat):
        assert got["tile"] == t and tuple(got["offset"]) == grid.boxes()[t][:2]
        assert got["label"] == (int(log[base[t] + r["label"]]) if r["label"] else 0)
        assert {k: v for k, v in got.items() if k not in ("label", "tile", "offset")} == {k: v for k, v in r.items() if k != "label"}
    # a frame no larger than one tile: the tile's own label map, exactly
    small = img[:90, :80]
    one, recs = gen.generate_tiled_label_map(small, tile=tile, overlap=overlap)
    ref, ref_recs = gen.generate_label_map(small)
    assert torch.equal(one, ref) and [r["label"] for r in recs] == [r["label"] for r in ref_recs] and all(r["tile"] == 0 and tuple(r["offset"]) == (0, 0) for r in recs)
