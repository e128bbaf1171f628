"""Linking label stacks without a GPU: utils.stack's host form (the definition the device route is tested against) against the plain loops of
tests/stack_ref.py on every case and in both modes, the hand-made cases' outcomes spelled out, track_table, the argument errors, the synthetic
stacks and the C ABI's declarations.  Integer work: every comparison is equality."""
import os
import re

import numpy as np
import pytest
import torch

from tests import stack_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ullsam_stack_pairs", "ullsam_stack_best", "ullsam_stack_link", "ullsam_stack_stats", "ullsam_stack_compact", "ullsam_stack_relabel")
NAMES = ("volume", "label_of_global", "voxels", "zrange", "boxes")
DTYPES = (torch.int32, torch.int32, torch.int64, torch.int32, torch.int32)


@pytest.fixture(scope="module")
def cases():
    return R.cases()


@pytest.fixture(scope="module")
def refs(cases):
    """The loops' results, computed once: {(case name, mode): link(...)}."""
    out = {}
    for c in cases:
        stats = R.pixel_counts(c["planes"], c["counts"])
        for mode in ("mutual", "all"):
            out[c["name"], mode] = R.link(c["planes"], c["counts"], c["iou"], mode, c["min_planes"], c["min_volume"], stats=stats)
    return out


def host(case, mode="mutual", **kw):
    from ullsam_amd.utils import stack as K
    args = dict(iou=case["iou"], mode=mode, min_planes=case["min_planes"], min_volume=case["min_volume"], device="cpu")
    args.update(kw)
    return K.link_label_stack(case["planes"], case["counts"], **args)


def test_host_form_is_the_loop_definition(cases, refs):
    for case in cases:
        for mode in ("mutual", "all"):
            got, want = host(case, mode), refs[case["name"], mode]
            for g, w_, what, dt in zip(got, want, NAMES, DTYPES):
                assert g.dtype == dt and tuple(g.shape) == w_.shape and np.array_equal(g.numpy(), w_), f"{case['name']} {mode}: {what}"
            assert tuple(got[0].shape) == case["planes"].shape and got[1].numel() == sum(case["counts"]) + 1 and int(got[1][0]) == 0
            assert torch.equal(host(case, mode, device=None)[0], got[0])


def test_the_case_list_exercises_the_ranking(cases, refs):
    """On the loops' own results: the sphere stacks hold candidates that mutual leaves unlinked, and some case has fewer objects under all."""
    spheres = [c["name"] for c in cases if c["name"].startswith("spheres")]
    assert len(spheres) >= 3
    assert sum(refs[n, "mutual"][5]["candidates"] - refs[n, "mutual"][5]["links"] for n in spheres) >= 1
    assert any(refs[n, "all"][5]["K"] < refs[n, "mutual"][5]["K"] for n in spheres)
    info = refs["spheres seed 4 6 x 70 x 200", "mutual"][5]
    assert (info["G"], info["candidates"], info["links"], info["K"]) == (308, 223, 217, 74) and refs["spheres seed 4 6 x 70 x 200", "all"][5]["K"] == 69
    for n in spheres:                                     # ids are permuted per plane: linking by identity would not reproduce this
        c = next(c for c in cases if c["name"] == n)
        if c["min_planes"] > 1 or c["min_volume"] > 0:
            continue
        assert not np.array_equal(refs[n, "mutual"][0], c["planes"]) and np.array_equal(refs[n, "mutual"][0] > 0, c["planes"] > 0)


def test_hand_made_cases_by_their_outcome(cases):
    by = {c["name"]: c for c in cases}
    log = lambda name, mode="mutual": host(by[name], mode)[1].tolist()
    # ties at exactly 1 / 2 go to the smaller partner id; the other half stays alone -- and joins under "all"
    assert log("tie on the successor side") == [0, 1, 1, 2] and log("tie on the successor side", "all") == [0, 1, 1, 1]
    assert log("tie on the predecessor side") == [0, 1, 2, 1] and log("tie on the predecessor side", "all") == [0, 1, 1, 1]
    # n * den = num * u links, one shared pixel fewer does not
    assert log("threshold equality") == [0, 1, 1] and log("threshold one pixel below") == [0, 1, 2]
    # b (global 3)'s best is a (1), whose best is b' (4); a2 (2) is b's weaker candidate: b and a2 stay unlinked
    assert log("no second choice") == [0, 1, 2, 3, 1] and log("no second choice", "all") == [0, 1, 1, 1, 1]
    # 3000 / 8503 beats 3833 / 10864 by a cross-product difference of 1, and float32 cannot tell them apart
    (n1, u1), (n2, u2) = R.EXACT
    assert n2 * u1 - n1 * u2 == 1 and np.float32(n1) / np.float32(u1) == np.float32(n2) / np.float32(u2)
    assert log("exact ranking") == [0, 1, 2, 1] and log("exact ranking (predecessor side)") == [0, 1, 2, 2]
    out = host(by["exact ranking"])
    assert out[2].tolist() == [n1 + n2 + u2 - n1, u1 - n2] and out[3].tolist() == [[0, 1], [1, 1]]
    # an object that misses a plane comes back as a new one; the declared, absent id of the middle plane maps to 0
    v = host(by["vanish and reappear"])
    assert v[1].tolist() == [0, 1, 0, 2] and v[3].tolist() == [[0, 0], [2, 2]] and v[4].tolist() == [[2, 1, 5, 3]] * 2 and v[2].tolist() == [12, 12]
    # Z = 1: the plane with its absent ids compacted
    one = by["Z = 1, absent ids"]
    v = host(one)
    lut = np.asarray([0, 1, 0, 2, 0], np.int32)
    assert np.array_equal(v[0].numpy(), lut[one["planes"]]) and v[1].tolist() == lut.tolist() and v[4].tolist() == [[0, 4, 8, 5], [5, 1, 68, 2]]
    assert log("an empty plane with K = 0 in the middle") == [0, 0, 1, 2]
    none = host(by["nothing at all"])
    assert int(none[0].abs().sum()) == 0 and none[1].tolist() == [0] and [tuple(x.shape) for x in none[2:]] == [(0,), (0, 2), (0, 4)]
    for w in (63, 64, 65, 130):
        v = host(by[f"whole rows, width {w}"])
        assert v[1].tolist() == [0, 1, 0, 1, 1, 2] and v[2].tolist() == [3 * w + 3 * w + w, w // 2] and v[4][0].tolist() == [0, 0, w - 1, 3]
    # min_planes, min_volume and both: A = 3 planes x 3 pixels, B = 1 plane x 20, C = 2 planes x 3
    assert host(by["drops: none"])[2].tolist() == [9, 20, 6]
    assert host(by["drops: min_planes"])[2].tolist() == [9, 6] and host(by["drops: min_volume"])[2].tolist() == [9, 20]
    both = host(by["drops: both"])
    assert both[2].tolist() == [9] and both[3].tolist() == [[0, 2]] and int(both[0].max()) == 1 and int((both[0] > 0).sum()) == 9


def test_ranking_is_exact_where_float32_ties():
    """(4096, 8191) against (4097, 8193): the cross-products differ by 1, the float32 quotients coincide, the first must win -- on either side,
    whichever of the two carries the smaller id.  (No image holds this pair: both lie above 1 / 2.)"""
    from ullsam_amd.utils import stack as K
    (n1, u1), (n2, u2) = R.EXACT_TABLE
    assert n1 * u2 - n2 * u1 == 1 and np.float32(n1) / np.float32(u1) == np.float32(n2) / np.float32(u2)
    for first_partner, second_partner in ((5, 3), (3, 5)):
        group = np.asarray([1, 1], np.int64)
        partner = np.asarray([first_partner, second_partner], np.int64)
        best = K._best(group, partner, np.asarray([n1, n2], np.int64), np.asarray([u1, u2], np.int64), 2)
        assert best.tolist() == [-1, 0]
        assert R.rank_key(n1, u1, first_partner) > R.rank_key(n2, u2, second_partner)
    tie = K._best(np.asarray([1, 1, 1], np.int64), np.asarray([9, 4, 6], np.int64), np.asarray([2, 4, 1], np.int64), np.asarray([4, 8, 2], np.int64), 2)
    assert tie.tolist() == [-1, 1]                        # 2 / 4 = 4 / 8 = 1 / 2: the smaller partner
    big = K._best(np.asarray([0, 0], np.int64), np.asarray([1, 2], np.int64), np.asarray([2 ** 31 - 2, 2 ** 31 - 1], np.int64),
                  np.asarray([2 ** 32 - 3, 2 ** 32 - 2], np.int64), 1)
    assert big.tolist() == [1]                            # products just below 2^63: (2^31 - 1) (2^32 - 3) > (2^31 - 2) (2^32 - 2)


def test_track_table(cases, refs):
    from ullsam_amd import _lib
    from ullsam_amd.utils import stack as K
    for case in cases:
        log = refs[case["name"], "mutual"][1]
        got = K.track_table(torch.from_numpy(log), case["counts"])
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), R.table(log, case["counts"])), case["name"]
        assert tuple(got.shape) == (refs[case["name"], "mutual"][5]["K"], len(case["counts"]))
        vol = refs[case["name"], "mutual"][0]
        for k in range(min(got.shape[0], 5)):             # the index does what it is for: object k + 1's pixels in plane z are that local id's
            for z in range(got.shape[1]):
                l = int(got[k, z])
                assert np.array_equal(vol[z] == k + 1, case["planes"][z] == l) if l else not (vol[z] == k + 1).any()
    by = {c["name"]: c for c in cases}
    assert K.track_table([0, 1, 1, 2], [1, 2]).tolist() == [[1, 1], [0, 2]]
    with pytest.raises(_lib.UllsamError):                 # "all" fused the two halves of plane 1 into one object
        K.track_table(refs["tie on the successor side", "all"][1], by["tie on the successor side"]["counts"])
    with pytest.raises(ValueError):
        K.track_table([0, 1, 1], [1, 2])


def test_errors(cases):
    from ullsam_amd import _lib
    from ullsam_amd.utils import stack as K
    case = {c["name"]: c for c in cases}["no second choice"]
    planes, counts = case["planes"], case["counts"]
    for bad in (dict(iou=(0, 2)), dict(iou=(3, 2)), dict(iou=(1, 2 ** 31)), dict(iou=0.25), dict(mode="best"), dict(min_planes=0), dict(min_volume=-1),
                dict(max_pairs=0), dict(max_pairs=2 ** 30 + 1)):
        with pytest.raises(ValueError):
            host(case, **bad)
    with pytest.raises(ValueError):
        K.link_label_stack(planes[0], counts[:1])                                    # not [Z, H, W]
    with pytest.raises(ValueError):
        K.link_label_stack(planes, counts[:1])
    with pytest.raises(ValueError):
        K.link_label_stack(planes, [2, -1])
    with pytest.raises(ValueError):
        K.link_label_stack(np.zeros((1, 1, 46341), np.int32), [0])
    with pytest.raises(_lib.UllsamError):
        K.link_label_stack(np.zeros((2, 2, 2), np.int32), [2 ** 31 - 2, 1])          # G > 2^31 - 2
    for value in (3, -1):
        bad = planes.copy()
        bad[1, 0, 40] = value                                                        # an id outside 0..K_z
        with pytest.raises(_lib.UllsamError):
            K.link_label_stack(bad, counts)
    with pytest.raises(_lib.UllsamError):
        host(case, max_pairs=2)                                                      # three distinct pairs
    assert len(host(case, max_pairs=3)) == 5


def test_label_stack_follows_its_recipe():
    from ullsam_amd.utils import synthetic as S
    seed, Z, H, W, n, rr, dz = 4, 6, 70, 200, 60, (5.0, 16.0), 2.5
    planes, counts = S.label_stack(seed, Z, H, W, n, rr, dz)
    assert planes.dtype == np.int32 and planes.shape == (Z, H, W) and len(counts) == Z and sum(counts) == 308
    rng = np.random.default_rng([seed, 0x57AC])
    cx, cy, cz, r = rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(-1, Z, n), rng.uniform(*rr, n)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for z in range(Z):                                    # the recipe with every disc tested against the whole plane
        rr2 = r ** 2 - (dz * (z - cz)) ** 2
        present = np.nonzero(rr2 > 0)[0]
        perm = rng.permutation(len(present))
        want = np.zeros((H, W), np.int32)
        for j, i in enumerate(present):
            want[(xx - cx[i]) ** 2 + (yy - cy[i]) ** 2 <= rr2[i]] = perm[j] + 1
        assert counts[z] == len(present) and np.array_equal(planes[z], want), z
    again, _ = S.label_stack(seed, Z, H, W, n, rr, dz)
    assert np.array_equal(again, planes) and not np.array_equal(S.label_stack(seed + 1, Z, H, W, n, rr, dz)[0], planes)


def _arg_count(decl):
    return len([a for a in decl.split(",") if a.strip()])


def test_header_declares_the_stack_entry_points_and_the_abi_stays_14():
    from ullsam_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code)
        assert m, s
        assert s in _lib.SIGNATURES and _arg_count(m.group(1)) == len(_lib.SIGNATURES[s]), s
        assert re.search(r"\b%s:" % s.replace("ullsam_", ""), src.split("int ullsam_stack_pairs")[0]), f"{s}: no comment states what it computes"
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", src).group(1)) == 14 == _lib.ABI_VERSION
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in SYMBOLS) and lib.ullsam_abi_version() == 14
    for fn in ("stack_pairs", "stack_best", "stack_link", "stack_stats", "stack_compact", "stack_relabel"):
        assert callable(getattr(ops, fn))
    assert os.path.exists(os.path.join(ROOT, "ullsam_amd", "csrc", "stack.hip"))
    with pytest.raises(_lib.UllsamError):                 # the kernels' wrappers take GPU tensors only; the host form lives in utils.stack
        ops.stack_best(torch.zeros((2,), dtype=torch.int64), torch.zeros((2,), dtype=torch.int32), torch.zeros((4,), dtype=torch.int32), 3)
