"""The label-map mosaic without a GPU: utils.mosaic's grid and host form (the definition the device route is tested against) against the
plain-loop definitions of tests/mosaic_ref.py, the threshold's edges, chains, and the C ABI's declarations.  Integer work: every comparison
is equality."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mosaic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ullsam_mosaic_seams", "ullsam_mosaic_union", "ullsam_mosaic_stats", "ullsam_mosaic_compact", "ullsam_mosaic_paste")
NAMES = ("labels", "label_of_global", "areas", "boxes")


@pytest.fixture(scope="module")
def cases():
    return R.cases()


def host(case, **kw):
    from ullsam_amd.utils import mosaic as M
    args = dict(iou=case["iou"], min_visible_area=case["mva"])
    args.update(kw)
    return M.stitch_label_maps(case["tiles"], case["counts"], M.tile_grid(*case["grid"]), device="cpu", **args)


@pytest.mark.parametrize("hwto", R.GRIDS)
def test_grid_covers_partitions_and_ends_at_the_border(hwto):
    from ullsam_amd.utils import mosaic as M
    H, W, tile, overlap = hwto
    g = M.tile_grid(H, W, tile, overlap)
    assert (g.H, g.W, g.th, g.tw) == (H, W, min(tile, H), min(tile, W)) and g.ntiles == g.nrows * g.ncols == len(g.boxes()) == len(g.cores())
    covered = np.zeros((H, W), np.int32)
    owned = np.zeros((H, W), np.int32)
    for t, ((top, left, h, w), (ct, cl, ch, cw)) in enumerate(zip(g.boxes(), g.cores())):
        assert (top, left) == (g.row_starts[t // g.ncols], g.col_starts[t % g.ncols]) and (h, w) == (g.th, g.tw)      # row-major numbering
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W
        assert ch > 0 and cw > 0 and top <= ct and ct + ch <= top + h and left <= cl and cl + cw <= left + w         # the core lies inside its box
        covered[top:top + h, left:left + w] += 1
        owned[ct:ct + ch, cl:cl + cw] += 1
    assert (covered >= 1).all() and (owned == 1).all()                           # the boxes cover the frame, the cores partition it
    for extent, starts, t in ((H, g.row_starts, g.th), (W, g.col_starts, g.tw)):
        inside = np.zeros(extent, np.int32)
        for s in starts:
            inside[s:s + t] += 1
        assert inside.min() >= 1 and inside.max() <= 2                            # at most two intervals contain any coordinate
        assert starts[0] == 0 and starts[-1] + t == extent and list(starts) == sorted(set(starts))   # the last tile ends at the border
        if len(starts) > 1 and overlap > 0:
            assert all(b < a + t for a, b in zip(starts, starts[1:]))             # neighbours do overlap
    assert g.boxes()[-1][0] + g.th == H and g.boxes()[-1][1] + g.tw == W


def test_grid_numbers_and_cuts():
    from ullsam_amd.utils import mosaic as M
    g = M.tile_grid(7424, 7424, 2048, 256)                                        # the 4 x 4 mosaic of 2048^2 tiles
    assert g.row_starts == g.col_starts == (0, 1792, 3584, 5376) and g.row_cuts == (0, 1920, 3712, 5504, 7424) and (g.th, g.tw) == (2048, 2048)
    g = M.tile_grid(100, 300, 128, 32)
    assert g.row_starts == (0,) and g.th == 100 and g.col_starts == (0, 96, 172) and g.col_cuts == (0, 112, 198, 300)
    # where the regular step would put a third interval over a coordinate, the regular interval before the closing one is left out
    g = M.tile_grid(10, 170, 64, 16)
    assert g.col_starts == (0, 48, 106) and g.col_cuts == (0, 56, 109, 170)
    assert M.tile_grid(10, 80, 64, 32).col_starts == (0, 16)                       # (the start 0 always stays)
    assert len(g.seams()) == 2 and g.seams()[1] == (1, 2, 0, (0, 106, 10, 6))
    assert M.tile_grid(128, 192, 64, 0).seams() == []                             # overlap 0 on a frame of whole tiles: no seam
    assert len(M.tile_grid(200, 96, 64, 0).seams()) > 0                           # (a closing tile pushed back to the border still overlaps)


def test_host_form_is_the_loop_definition(cases):
    from ullsam_amd.utils import mosaic as M
    for case in cases:
        grid = M.tile_grid(*case["grid"])
        got = host(case)
        want = R.stitch(case["tiles"], case["counts"], grid, case["iou"], case["mva"])
        for g, w_, what in zip(got, want, NAMES):
            assert g.dtype == torch.int32 and tuple(g.shape) == w_.shape and np.array_equal(g.numpy(), w_), f"{case['name']}: {what}"
        assert tuple(got[0].shape) == (grid.H, grid.W) and got[1].numel() == sum(case["counts"]) + 1 and int(got[1][0]) == 0


def test_reconstruction_up_to_a_bijection(cases):
    from ullsam_amd.utils import mosaic as M
    seen = 0
    for case in cases:
        if case["truth"] is None or case["mva"]:
            continue
        grid = M.tile_grid(*case["grid"])
        assert all(min(h, w) >= 2 for _, _, _, (_, _, h, w) in grid.seams())          # (both pixels next to a cut lie in the seam)
        labels = host(case)[0].numpy()
        truth = case["truth"]
        if case["grid"][3] == 0 and grid.seams():                                  # (instances across the cuts that have no overlap stay split: no bijection)
            continue
        if case["grid"][3] == 0:                                                   # overlap 0: nothing merges, the mosaic is the paste, renumbered
            base = np.concatenate([[0], np.cumsum(case["counts"])])[:-1, None, None].astype(np.int32)
            assert R.same_up_to_a_bijection(labels, R.paste(case["tiles"] + (case["tiles"] > 0) * base, grid)), case["name"]
            if grid.ntiles > 1:
                assert grid.seams() == [] and int(labels.max()) > len(np.unique(truth)) - 1      # the instances a cut crosses stay split
            else:
                assert R.same_up_to_a_bijection(labels, truth)
        else:
            assert R.same_up_to_a_bijection(labels, truth), case["name"]
        seen += 1
    assert seen >= 9
    # the hand-placed instances of the 3 x 3 frame: one id each in the mosaic, although 2, 3 and 4 tiles hold parts of them
    case = cases[0]
    grid = M.tile_grid(*case["grid"])
    labels, log, _, _ = (x.numpy() for x in host(case))
    base = np.concatenate([[0], np.cumsum(case["counts"])])
    for inst, ntiles in ((1, 2), (2, 3), (3, 4), (4, 2), (5, 2)):
        holders = [t for t, (top, left, h, w) in enumerate(grid.boxes()) if (case["truth"][top:top + h, left:left + w] == inst).any()]
        assert len(holders) >= ntiles and len(np.unique(labels[case["truth"] == inst])) == 1, inst
        mosaic_id = int(labels[case["truth"] == inst][0])
        for t, (top, left, h, w) in enumerate(grid.boxes()):                       # every tile's own label of the instance maps to that id
            local = np.unique(case["tiles"][t][case["truth"][top:top + h, left:left + w] == inst])
            assert all(log[base[t] + l] == mosaic_id for l in local)


def test_threshold_edges(cases):
    by = {c["name"]: c for c in cases}
    log = host(by["threshold(1, 2)"])[1].tolist()                                  # global ids: tile 0 -> 1, 2; tile 1 -> 3, 4, 5, 6
    assert log[1] == log[3] == log[4] != 0 and log[2] == log[5] != log[1] and log[6] not in (0, log[1], log[2])     # IoU exactly 1/2 merges, with both halves
    log = host(by["threshold(501, 1000)"])[1].tolist()
    assert len({log[1], log[3], log[4]}) == 3 and log[2] == log[5]                  # just above 1/2: none of the three
    log = host(by["threshold(1, 1)"])[1].tolist()
    assert len({log[1], log[3], log[4]}) == 3 and log[2] == log[5]                  # only identical seam footprints
    labels = host(by["threshold(1, 1)"])[0].numpy()
    assert labels[0, 0] == 0 and labels[0, 5] == log[1] and labels[0, 12] == log[4] and labels[0, 11] == log[1]      # the cut is at column 12: the owner speaks


def test_chains_order_and_drops(cases):
    from ullsam_amd.utils import mosaic as M
    by = {c["name"]: c for c in cases}
    case = by["chain mva=0 empty=False"]
    grid = M.tile_grid(*case["grid"])
    truth, counts = case["truth"], case["counts"]
    base = np.concatenate([[0], np.cumsum(counts)])
    labels, log, areas, boxes = (x.numpy() for x in host(case))
    assert R.same_up_to_a_bijection(labels, truth) and len(areas) == 4
    bar = [int(base[t] + case["tiles"][t][0, 5]) for t in range(5)]                # the bar's label in each of the five tiles: one chain
    assert len(set(log[bar])) == 1 and log[bar[0]] in (1, 2) and min(bar) == bar[0] <= 2          # one component; its representative is tile 0's id
    # the instance across the last cut: members in tiles 3 and 4 only, so its representative (tile 3's id) is larger than every id of tiles 0..2
    m3, m4 = int(base[3] + case["tiles"][3][2, 34 - 24]), int(base[4] + case["tiles"][4][2, 34 - 32])
    assert log[m3] == log[m4] == labels[2, 35] and m3 < m4
    # final labels ascend with the representative = the smallest member
    reps = {}
    for gid in range(1, len(log)):
        if log[gid]:
            reps.setdefault(int(log[gid]), gid)
    assert [reps[k] for k in sorted(reps)] == sorted(reps.values()) and sorted(reps) == list(range(1, len(areas) + 1))
    # the instance inside the seam of tiles 1 and 2, right of the cut: tile 1's label is visible nowhere in tile 1's core, yet it has the mosaic id
    hidden = int(base[1] + case["tiles"][1][2, 21 - 8])
    assert log[hidden] == labels[2, 21] != 0 and not (R.paste(case["tiles"], grid)[:, 12:20][2:4] > 0).any()
    assert areas.tolist() == [int((labels == k).sum()) for k in range(1, 5)] and boxes[log[bar[0]] - 1].tolist() == [1, 0, 46, 0]
    # min_visible_area = 5 drops the one-pixel instance and the 4-pixel instance; BOTH tiles' labels of the latter map to 0
    drop = by["chain mva=5 empty=False"]
    labels5, log5, areas5, _ = (x.numpy() for x in host(drop))
    other = int(base[2] + drop["tiles"][2][2, 21 - 16])
    assert log5[hidden] == 0 and log5[other] == 0 and len(areas5) == 2 and (labels5[truth == 4] == 0).all() and (labels5[truth == 3] == 0).all()
    assert sorted(areas5.tolist()) == [8, 46] and int(labels5.max()) == 2
    # tiles without any instance
    empty = by["chain mva=0 empty=True"]
    assert empty["counts"][3] == 0 and empty["counts"][4] == 0
    assert R.same_up_to_a_bijection(host(empty)[0].numpy(), empty["truth"])
    none = M.stitch_label_maps(np.zeros((5, 6, 16), np.int32), [0] * 5, grid)
    assert int(none[0].abs().sum()) == 0 and none[1].tolist() == [0] and tuple(none[2].shape) == (0,) and tuple(none[3].shape) == (0, 4)


def test_single_tile_is_the_tile_with_hidden_ids_compacted():
    from ullsam_amd.utils import mosaic as M
    rng = np.random.default_rng(3)
    tile = np.zeros((40, 50), np.int32)
    for v in (2, 3, 5, 9):                                                         # ids 1, 4, 6, 7, 8 are declared and absent
        y, x = rng.integers(0, 30), rng.integers(0, 40)
        tile[y:y + 6, x:x + 7] = v
    grid = M.tile_grid(40, 50, 64, 16)
    assert grid.ntiles == 1 and grid.seams() == []
    labels, log, areas, boxes = M.stitch_label_maps(tile[None], [9], grid)
    present = np.unique(tile[tile > 0])
    lut = np.zeros(10, np.int32)
    lut[present] = np.arange(1, len(present) + 1)
    assert np.array_equal(labels.numpy(), lut[tile]) and np.array_equal(log.numpy(), lut) and areas.tolist() == [int((tile == v).sum()) for v in present]
    ys, xs = np.nonzero(tile == present[0])
    assert boxes[0].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
    same = M.stitch_label_maps(lut[tile][None], [len(present)], grid)[0]           # nothing hidden: the output equals the input tile
    assert np.array_equal(same.numpy(), lut[tile])


def test_errors(cases):
    from ullsam_amd import _lib
    from ullsam_amd.utils import mosaic as M
    for bad in ((100, 100, 64, 33), (100, 100, 64, -1), (100, 100, 1, 1), (0, 100, 64, 16)):
        with pytest.raises(ValueError):
            M.tile_grid(*bad)
    case = cases[0]
    grid = M.tile_grid(*case["grid"])
    tiles = case["tiles"].copy()
    tiles[4, 10, 10] = case["counts"][4] + 1                                       # an id above K_t
    with pytest.raises(_lib.UllsamError):
        M.stitch_label_maps(tiles, case["counts"], grid)
    tiles[4, 10, 10] = -1
    with pytest.raises(_lib.UllsamError):
        M.stitch_label_maps(tiles, case["counts"], grid)
    two = {c["name"]: c for c in cases}["threshold(1, 2)"]                         # three distinct pairs in its seam, two of them merging with label 1
    with pytest.raises(_lib.UllsamError):
        host(two, max_pairs=1)
    assert len(host(two, max_pairs=3)) == 4
    with pytest.raises(_lib.UllsamError):
        M.stitch_label_maps(np.zeros((1, 4, 4), np.int32), [2 ** 31 - 1], M.tile_grid(4, 4, 8, 0))      # G > 2^31 - 2
    for iou in ((0, 2), (3, 2), (1, 2 ** 31)):
        with pytest.raises(ValueError):
            host(two, iou=iou)
    with pytest.raises(ValueError):
        M.stitch_label_maps(case["tiles"][:3], case["counts"][:3], grid)


def _arg_count(decl):
    return len([a for a in decl.split(",") if a.strip()])


def test_header_declares_the_mosaic_entry_points_and_the_abi_stays_14():
    from ullsam_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code)
        assert m, s
        assert s in _lib.SIGNATURES and _arg_count(m.group(1)) == len(_lib.SIGNATURES[s]), s
        assert re.search(r"\b%s\b" % s.replace("ullsam_", ""), src.split("int ullsam_mosaic_seams")[0]), f"{s}: no comment states what it computes"
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", src).group(1)) == 14 == _lib.ABI_VERSION
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.ullsam_abi_version() == 14
    for fn in ("mosaic_seams", "mosaic_union", "mosaic_stats", "mosaic_compact", "mosaic_paste"):
        assert callable(getattr(ops, fn))
    assert ops.mosaic_table_slots(1) == 2 and ops.mosaic_table_slots(3) == 8 and ops.mosaic_table_slots(1 << 20) == 1 << 21
    with pytest.raises(_lib.UllsamError):                                          # the kernels' wrappers take GPU tensors only; the host form lives in utils.mosaic
        ops.mosaic_union(torch.zeros((2,), dtype=torch.int64), 3)


def test_label_frame_is_label_tile_on_a_square():
    from ullsam_amd.utils import synthetic as S
    for seed, size, n, rr in ((3, 256, 9, (20.0, 60.0)), (4, 97, 30, (2.0, 30.0))):
        assert np.array_equal(S.label_frame(seed, size, size, n, rr), S.label_tile(seed, size, n, rr))
    wide = S.label_frame(5, 60, 200, 12, (5.0, 25.0))
    assert wide.shape == (60, 200) and wide.dtype == np.int32 and 0 < len(np.unique(wide)) - 1 <= 12
