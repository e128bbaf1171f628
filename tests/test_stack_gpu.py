"""Linking label stacks on the GPU (csrc/stack.hip): the device route against the host form of utils.stack.link_label_stack (itself checked against
the loops of tests/stack_ref.py without a GPU), the kernels one by one through ops against per-pixel loops, Fractions and numpy, the status
flags, and SamAutomaticMaskGenerator.generate_stack_label_volume.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import stack_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("volume", "label_of_global", "voxels", "zrange", "boxes")
DTYPES = (torch.int32, torch.int32, torch.int64, torch.int32, torch.int32)
INT_MAX = 2 ** 31 - 1


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    large = R.sphere_case(*R.LARGE)
    return R.cases() + [dict(large, name="many workgroups"), dict(large, name="many workgroups, drops", min_planes=3, min_volume=2000)]


def _link(case, device, mode="mutual", **kw):
    from ullsam_amd.utils import stack as K
    args = dict(iou=case["iou"], mode=mode, min_planes=case["min_planes"], min_volume=case["min_volume"])
    args.update(kw)
    planes = T(case["planes"]) if device == DEV else case["planes"]
    return K.link_label_stack(planes, case["counts"], device=device, **args)


def test_device_route_equals_the_host_form(cases):
    for case in cases:
        for mode in ("mutual", "all"):
            want = _link(case, "cpu", mode)
            got = _link(case, DEV, mode)
            for g, w_, what, dt in zip(got, want, NAMES, DTYPES):
                assert g.is_cuda and g.dtype == dt and g.shape == w_.shape and torch.equal(g.cpu(), w_), f"{case['name']} {mode}: {what}"
            again = _link(case, DEV, mode)
            assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{case['name']} {mode}: two runs differ"


def _device_inputs(case):
    base = np.asarray(R.bases(case["counts"]), np.int32)
    return base, T(case["planes"]), T(base), int(base[-1])


def _table(keys, counts):
    k, c = keys.cpu().numpy().view(np.uint64), counts.cpu().numpy()
    assert (c[k == 0] == 0).all()
    return sorted((int(x) >> 32, int(x) & 0xffffffff, int(n)) for x, n in zip(k[k != 0], c[k != 0]))


def test_pair_kernel_table_and_areas(cases):
    """The pair table, read back and sorted by key, and the areas A [G + 1] against the per-pixel loops."""
    from ullsam_amd import ops
    by = {c["name"]: c for c in cases}
    names = ["no second choice", "exact ranking", "Z = 1, absent ids", "nothing at all", "runs crossing segment and row ends", "drops: none",
             "spheres seed 4 6 x 70 x 200", "many workgroups"] + [f"whole rows, width {w}" for w in (63, 64, 65, 130)]
    for name in names:
        case = by[name]
        base, planes, base_d, g = _device_inputs(case)
        keys, counts, areas, flags = ops.stack_pairs(planes, base_d, g, 4096)
        want_areas, want_pairs, _ = R.pixel_counts(case["planes"], case["counts"])
        assert keys.numel() == 8192 and keys.dtype == torch.int64 and counts.dtype == torch.int32
        got = _table(keys, counts)
        assert got == sorted((a, b, n) for (a, b), n in want_pairs.items()), name
        dense = np.zeros(g + 1, np.int32)
        for gid, n in want_areas.items():
            dense[gid] = n
        assert np.array_equal(areas.cpu().numpy(), dense), name
        assert flags.cpu().tolist()[:3] == [0, 0, len(got)], name
    assert len(R.pixel_counts(by["many workgroups"]["planes"], by["many workgroups"]["counts"])[1]) > 900


def _hand_table(pairs, areas):
    """pairs [(a, b, n)], areas {g: pixels} -> (keys, counts, areas [g + 1], g) on the device, with empty slots between the pairs."""
    g = max(areas)
    keys, counts = np.zeros(2 * len(pairs) + 3, np.int64), np.zeros(2 * len(pairs) + 3, np.int32)
    for i, (a, b, n) in enumerate(pairs):
        keys[2 * i + 1] = (a << 32) | b
        counts[2 * i + 1] = n
    dense = np.zeros(g + 1, np.int32)
    for gid, n in areas.items():
        dense[gid] = n
    return T(keys), T(counts), T(dense), g


def _best_by_fractions(pairs, areas, g, iou):
    from fractions import Fraction
    succ, pred, cands = [0] * (g + 1), [0] * (g + 1), {}
    for a, b, n in pairs:
        u = areas[a] + areas[b] - n
        if n > 0 and Fraction(n, u) >= Fraction(*iou):
            cands[a, b] = (Fraction(n, u))
    for (a, b), q in cands.items():
        if not succ[a] or (q, -b) > (cands[a, succ[a]], -succ[a]):
            succ[a] = b
        if not pred[b] or (q, -a) > (cands[pred[b], b], -pred[b]):
            pred[b] = a
    return succ, pred


def test_best_partner_and_link_kernels_on_hand_made_tables():
    from ullsam_amd import ops
    (n1, u1), (n2, u2) = R.EXACT_TABLE                     # (4096, 8191) against (4097, 8193): the first wins by a cross-product difference of 1
    assert n1 * u2 - n2 * u1 == 1 and np.float32(n1) / np.float32(u1) == np.float32(n2) / np.float32(u2)
    A = 5000                                                # the shared label's area; the partners' areas make the unions come out
    tables = {
        # name: (pairs (a, b, n), areas, iou, succ, pred, parent under mutual, parent under all)
        "tie on the successor side": ([(1, 2, 2), (1, 3, 2)], {1: 4, 2: 2, 3: 2}, (1, 2), [0, 2, 0, 0], [0, 0, 1, 1], [0, 1, 1, 3], [0, 1, 1, 1]),
        "tie on the predecessor side": ([(1, 3, 2), (2, 3, 2)], {1: 2, 2: 2, 3: 4}, (1, 2), [0, 3, 3, 0], [0, 0, 0, 1], [0, 1, 2, 1], [0, 1, 1, 1]),
        # the exact winner carries the LARGER id on the successor side and on the predecessor side: equal floats broken by the smaller id pick the loser
        "exact ranking, successor side": ([(1, 2, n2), (1, 3, n1)], {1: A, 2: u2 - A + n2, 3: u1 - A + n1}, (1, 4), [0, 3, 0, 0], [0, 0, 1, 1],
                                          [0, 1, 2, 1], [0, 1, 1, 1]),
        "exact ranking, predecessor side": ([(1, 3, n2), (2, 3, n1)], {1: u2 - A + n2, 2: u1 - A + n1, 3: A}, (1, 4), [0, 3, 3, 0], [0, 0, 0, 2],
                                            [0, 1, 2, 2], [0, 1, 1, 1]),
        "exact ranking, the winner has the smaller id": ([(1, 2, n1), (1, 3, n2)], {1: A, 2: u1 - A + n1, 3: u2 - A + n2}, (1, 4), [0, 2, 0, 0], [0, 0, 1, 1],
                                                         [0, 1, 1, 3], [0, 1, 1, 1]),
        # b = 3's best is a = 1, whose best is b' = 4; a2 = 2's only candidate is b: 12 / 20, 8 / 28, 8 / 48
        "no second choice": ([(1, 4, 12), (1, 3, 8), (2, 3, 8)], {1: 20, 2: 40, 3: 16, 4: 12}, (1, 8), [0, 4, 3, 0, 0], [0, 0, 0, 1, 1],
                             [0, 1, 2, 3, 1], [0, 1, 1, 1, 1]),
        # below the threshold and n = 0: no candidates; a chain of three planes
        "threshold and chain": ([(1, 3, 3), (2, 4, 2), (3, 5, 6), (1, 4, 0)], {1: 6, 2: 6, 3: 6, 4: 5, 5: 6}, (1, 3), [0, 3, 0, 5, 0, 0], [0, 0, 0, 1, 0, 3],
                                [0, 1, 2, 1, 4, 1], [0, 1, 2, 1, 4, 1]),
    }
    for name, (pairs, areas, iou, succ_w, pred_w, mutual_w, all_w) in tables.items():
        for order in (pairs, pairs[::-1]):                  # the slots' order does not matter
            keys, counts, areas_d, g = _hand_table(order, areas)
            assert (succ_w, pred_w) == _best_by_fractions(pairs, areas, g, iou), name
            succ, pred, flags = ops.stack_best(keys, counts, areas_d, g, iou)
            assert succ.dtype == torch.int32 and succ.cpu().tolist() == succ_w and pred.cpu().tolist() == pred_w, name
            parent, flags2 = ops.stack_link(g, succ=succ, pred=pred)
            assert parent.dtype == torch.int32 and parent.cpu().tolist() == mutual_w, name
            fused, flags3 = ops.stack_link(g, keys=keys, counts=counts, areas=areas_d, iou=iou)
            assert fused.cpu().tolist() == all_w, name
            assert not flags.cpu().numpy().any() and not flags2.cpu().numpy().any() and not flags3.cpu().numpy().any()
    # many labels contending for one word: 600 candidates of label 1 with distinct IoUs n / 1000; the largest n wins whatever arrives first
    rng = np.random.default_rng(7)
    ns = rng.permutation(np.arange(1, 601))
    pairs = [(1, 2 + i, int(n)) for i, n in enumerate(ns)]
    areas = {1: 1000, **{2 + i: int(n) for i, n in enumerate(ns)}}
    keys, counts, areas_d, g = _hand_table(pairs, areas)
    succ, pred, _ = ops.stack_best(keys, counts, areas_d, g, (1, 2 ** 20))
    assert int(succ[1]) == 2 + int(np.argmax(ns)) and pred.cpu().tolist()[2:] == [1] * 600 and succ.cpu().tolist()[2:] == [0] * 600
    parent, _ = ops.stack_link(g, succ=succ, pred=pred)
    want = np.arange(g + 1)
    want[2 + int(np.argmax(ns))] = 1
    assert np.array_equal(parent.cpu().numpy(), want)
    # a long chain 1 - 2 - ... - 3000 walks to its head; a table with ids no stack produces is flagged and indexes nothing
    n = 3000
    chain = [(i, i + 1, 1) for i in range(1, n)]
    keys, counts, areas_d, g = _hand_table(chain, {i: 1 for i in range(1, n + 1)})
    succ, pred, _ = ops.stack_best(keys, counts, areas_d, g, (1, 1))
    parent, _ = ops.stack_link(g, succ=succ, pred=pred)
    assert parent.cpu().tolist() == [0] + [1] * n and ops.stack_link(g, keys=keys, counts=counts, areas=areas_d, iou=(1, 1))[0].cpu().tolist() == [0] + [1] * n
    for bad in ([(1, 9, 1)], [(3, 2, 1)], [(2, 2, 1)], [(1, 2, 7)]):          # an id above G, descending ids, a self pair, an overlap above the areas
        keys, counts, areas_d, g = _hand_table(bad + [(1, 3, 2)], {1: 2, 2: 2, 3: 2})
        succ, pred, flags = ops.stack_best(keys, counts, areas_d, g, (1, 4))
        assert flags.cpu().tolist()[0] == 1 and succ.cpu().tolist() == [0, 3, 0, 0] and pred.cpu().tolist() == [0, 0, 0, 1]
        parent, flags = ops.stack_link(g, keys=keys, counts=counts, areas=areas_d, iou=(1, 4))
        assert flags.cpu().tolist()[0] == 1 and parent.cpu().tolist() == [0, 1, 2, 1]
    parent, flags = ops.stack_link(3, succ=T(np.asarray([0, 3, 0, 2], np.int32)), pred=T(np.asarray([0, 0, 3, 7], np.int32)))   # pred above G; a predecessor that is no smaller id
    assert flags.cpu().tolist()[0] == 1 and parent.cpu().tolist() == [0, 1, 2, 3]


def test_stats_compaction_and_relabel_kernels(cases):
    from ullsam_amd import ops
    case = {c["name"]: c for c in cases}["spheres seed 4 9 x 200 x 300"]
    base, planes, base_d, g = _device_inputs(case)
    ref = R.link(case["planes"], case["counts"], case["iou"], "all")
    rep = np.asarray([0] + [ref[5]["rep"][i] for i in range(1, g + 1)], np.int32)
    parent = T(rep)
    vox_raw, zr_raw, box_raw, flags = ops.stack_stats(planes, base_d, g, parent)
    assert vox_raw.dtype == torch.int64 and not flags.cpu().numpy().any()
    glob = np.where(case["planes"] > 0, case["planes"] + base[:-1, None, None], 0)
    raw = rep[glob]
    v_np, z_np, b_np = vox_raw.cpu().numpy(), zr_raw.cpu().numpy(), box_raw.cpu().numpy()
    zs, ys, xs = np.nonzero(raw)
    ids = raw[zs, ys, xs]
    want_v = np.bincount(ids, minlength=g + 1)
    assert np.array_equal(v_np, want_v) and v_np[0] == 0
    for v in range(1, g + 1):
        m = ids == v
        if m.any():
            assert z_np[v].tolist() == [zs[m].min(), zs[m].max()] and b_np[v].tolist() == [xs[m].min(), ys[m].min(), xs[m].max(), ys[m].max()]
        else:
            assert z_np[v].tolist() == [INT_MAX, -1] and b_np[v].tolist() == [INT_MAX, INT_MAX, -1, -1]
    present = v_np > 0
    for min_planes, min_volume in ((1, 0), (3, 0), (1, int(np.median(v_np[present])) + 1), (2, int(np.median(v_np[present])) + 1)):
        log, voxels, zrange, boxes, k = ops.stack_compact(vox_raw, zr_raw, box_raw, parent, min_planes, min_volume)
        keep = present & (v_np >= min_volume) & (z_np[:, 1].astype(np.int64) - z_np[:, 0] + 1 >= min_planes)
        lmap = (np.cumsum(keep) * keep).astype(np.int32)
        kk = int(k.item())
        assert kk == keep.sum() and 0 < kk and np.array_equal(log.cpu().numpy(), lmap[rep])
        assert kk < present.sum() or (min_planes, min_volume) == (1, 0)
        assert np.array_equal(voxels.cpu().numpy()[:kk], v_np[keep]) and np.array_equal(zrange.cpu().numpy()[:kk], z_np[keep])
        assert np.array_equal(boxes.cpu().numpy()[:kk], b_np[keep])
        assert np.array_equal(ops.stack_relabel(planes, base_d, g, log).cpu().numpy(), lmap[raw])
    # relabel: odd plane sizes (H * W no multiple of 4), 16 bytes per lane and not, buffers 4 bytes off a 16-byte boundary; a guard band stays intact
    rng = np.random.default_rng(9)
    for Z, H, W in ((3, 7, 37), (2, 33, 64), (2, 5, 1028), (1, 1, 1)):
        counts = rng.integers(1, 40, Z)
        pl = np.stack([rng.integers(0, k + 1, (H, W)) for k in counts]).astype(np.int32)
        b = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        gg = int(b[-1])
        table = rng.integers(0, 1000, gg + 1).astype(np.int32)
        want = np.where(pl > 0, table[pl + b[:-1, None, None]], 0)
        for shift in (0, 1):
            guard, pad = -123456789, 1024
            src = torch.zeros((pad + pl.size,), dtype=torch.int32, device=DEV)[shift:shift + pl.size].view(Z, H, W)
            src.copy_(T(pl))
            buf = torch.full((pad + pl.size + pad,), guard, dtype=torch.int32, device=DEV)
            out = buf[pad + shift:pad + shift + pl.size].view(Z, H, W)
            got = ops.stack_relabel(src, T(b), gg, T(table), out=out)
            assert np.array_equal(got.cpu().numpy(), want), (Z, H, W, shift)
            assert bool((buf[:pad + shift] == guard).all()) and bool((buf[pad + shift + pl.size:] == guard).all())


def test_status_flags_raise_and_leave_the_process_usable(cases):
    """An id outside 0..K_z and more distinct pairs than max_pairs are CHECKED inputs: they set a status word, index nothing out of bounds, and
    the next call works."""
    from ullsam_amd import _lib, ops
    by = {c["name"]: c for c in cases}
    case = by["spheres seed 4 6 x 70 x 200"]
    for where, value in (((2, 5, 5), None), ((5, 30, 30), -7), ((0, 2, 60), 2 ** 31 - 1), ((5, 69, 199), -(2 ** 31))):
        bad = dict(case, planes=case["planes"].copy())
        bad["planes"][where] = case["counts"][where[0]] + 1 if value is None else value
        for mode in ("mutual", "all"):
            with pytest.raises(_lib.UllsamError):
                _link(bad, DEV, mode)
        base, planes, base_d, g = _device_inputs(bad)       # the kernels skip the id: everything else is counted as if the pixel were background
        keys, counts, areas, flags = ops.stack_pairs(planes, base_d, g, 4096)
        clean = bad["planes"].copy()
        clean[where] = 0
        want_areas, want_pairs, _ = R.pixel_counts(clean, case["counts"])
        assert flags.cpu().tolist()[:2] == [1, 0] and _table(keys, counts) == sorted((a, b, n) for (a, b), n in want_pairs.items())
        assert int(areas.sum()) == sum(want_areas.values())
    with pytest.raises(_lib.UllsamError):
        _link(case, DEV, max_pairs=4)                       # far more pairs than the table is allowed to take
    small = by["no second choice"]                          # three distinct pairs
    for mode in ("mutual", "all"):
        with pytest.raises(_lib.UllsamError):
            _link(small, DEV, mode, max_pairs=1)
        with pytest.raises(_lib.UllsamError):
            _link(small, DEV, mode, max_pairs=2)
        for g_, w_ in zip(_link(small, DEV, mode, max_pairs=3), _link(small, "cpu", mode)):
            assert torch.equal(g_.cpu(), w_)
    for g_, w_ in zip(_link(case, DEV), _link(case, "cpu")):
        assert torch.equal(g_.cpu(), w_)


def test_generate_stack_label_volume_links_the_planes_label_maps():
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import stack as K
    from ullsam_amd.utils import synthetic as S
    from tests import util as U
    from tests.test_amg_gpu import _small_sam
    sam, _ = _small_sam()
    S.blob_decoder_init(sam)                                # the structured decoder: a click draws a disc around itself
    kw = dict(points_per_side=6, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05, box_nms_thresh=0.7)
    gen = SamAutomaticMaskGenerator(sam, output_mode="uncompressed_rle", **kw)
    img = np.ascontiguousarray(U.rand_image((3, 104, 104), 23, 255.0).transpose(1, 2, 0))
    images = [img[s:s + 96, s:s + 96] for s in (0, 3, 6)]    # three planes of 96^2, shifted by a few pixels
    volume, records, objects = gen.generate_stack_label_volume(images, min_visible_area=3, min_planes=1)
    assert volume.is_cuda and volume.dtype == torch.int32 and tuple(volume.shape) == (3, 96, 96)
    per_plane = [gen.generate_label_map(im, min_visible_area=3) for im in images]
    counts = [max((r["label"] for r in recs), default=0) for _, recs in per_plane]
    assert sum(counts) >= 3
    want = K.link_label_stack(torch.stack([l.cpu() for l, _ in per_plane]), counts, device="cpu")
    assert torch.equal(volume.cpu(), want[0]) and int(volume.max()) == len(want[2])
    assert sorted(objects) == ["boxes", "label_of_global", "voxels", "zrange"]
    for name, w_ in zip(("label_of_global", "voxels", "zrange", "boxes"), want[1:]):
        assert torch.equal(objects[name].cpu(), w_), name
    log = want[1]
    base = np.concatenate([[0], np.cumsum(counts)])
    flat = [(z, r) for z, (_, recs) in enumerate(per_plane) for r in recs]
    assert len(records) == len(flat)
    for got, (z, r) in zip(records, flat):
        assert got["plane"] == z and got["object"] == (int(log[base[z] + r["label"]]) if r["label"] else 0)
        assert {k: v for k, v in got.items() if k not in ("plane", "object")} == r
    # an array [Z, H, W, 3] and another mode / filter go the same way
    vol_all, _, obj_all = gen.generate_stack_label_volume(np.stack(images), min_visible_area=3, mode="all", iou=(1, 8), min_planes=2)
    want_all = K.link_label_stack(torch.stack([l.cpu() for l, _ in per_plane]), counts, iou=(1, 8), mode="all", min_planes=2, device="cpu")
    assert torch.equal(vol_all.cpu(), want_all[0]) and torch.equal(obj_all["zrange"].cpu(), want_all[3])
    # a stack of one plane: the plane's own label map, exactly
    one, recs, obj = gen.generate_stack_label_volume(images[:1])
    ref, ref_recs = gen.generate_label_map(images[0])
    assert torch.equal(one[0], ref) and [r["object"] for r in recs] == [r["label"] for r in ref_recs] and all(r["plane"] == 0 for r in recs)
    assert obj["zrange"].cpu().tolist() == [[0, 0]] * int(ref.max())
