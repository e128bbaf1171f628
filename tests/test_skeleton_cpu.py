"""utils.skeleton without a GPU: the tables and the numpy host form against the plain loops of tests/skeleton_ref.py, the small cases pixel for pixel,
the properties the rule promises (a fixed point, symmetry under relabelling, independence of neighbours, topology), the links and degrees, the ABI,
the kernels' resources, argument errors.  Integer work: every assertion is equality."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import distance_ref as R
from tests import skeleton_ref as K
from ullsam_amd import _lib
from ullsam_amd.utils import distance as D
from ullsam_amd.utils import skeleton as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


def N(t):
    return t.numpy().astype(np.int64)


def shape_list():
    """[(name, labels int32 [H, W])]: the smallest shapes at which the kernels can still go wrong (tests/test_skeleton_gpu.py runs the same list)."""
    from tests import test_distance_gpu as TD
    from ullsam_amd.utils import synthetic as SY
    odd = R.blobs(21, 37, 63, n=9)
    assert odd.size % 4 != 0
    disc = K.disc(70, 131, 32, 64, 24)                       # centred on a corner of the 64 x 32 tiles: the front crosses tile borders in both axes
    frame = SY.label_frame(7, 300, 517, 90, (6.0, 22.0))
    filaments = SY.filament_frame(3, 200, 260, 5)
    assert len(np.unique(frame)) > 40 and len(np.unique(filaments)) == 6
    return (K.hand_made() + R.cases() + [(f"whole rows, width {w}", TD._whole_rows(w)) for w in (63, 64, 65, 130)]
            + [("H * W no multiple of 4", odd), ("a disc of radius 24", disc), ("dense blobs, 3 ids, 40 x 29", R.blobs(40, 40, 29, n=8, ids=3)),
               ("label_frame 300 x 517", frame), ("branched filaments 200 x 260", filaments)])


@pytest.fixture(scope="module")
def shapes():
    return shape_list()


@pytest.fixture(scope="module")
def thinned(shapes):
    """{name: the host form's Skeleton}: computed once, shared, never changed."""
    return {name: S.skeletonize_labels(lab) for name, lab in shapes}


def test_tables_equal_the_formulas_bit_by_bit():
    for parity in (0, 1):
        assert S.TABLES[parity].tolist() == K.TABLES[parity] and sum(K.TABLES[parity]) == 37
        words = S.table_words(parity)
        assert len(words) == 8 and [bool((words[c >> 5] >> (c & 31)) & 1) for c in range(256)] == K.TABLES[parity]
    assert K.TABLES[0] != K.TABLES[1]


def test_host_form_against_the_loops(shapes, thinned):
    seen = 0
    for name, lab in shapes:
        want, n, trail = K.skeletonize(lab)
        got = thinned[name]
        assert isinstance(got, S.Skeleton) and got.labels.dtype == torch.int32 and tuple(got.labels.shape) == lab.shape, name
        assert np.array_equal(N(got.labels), want) and got.subiterations == n, name
        if lab.shape[0] <= 40 and lab.shape[1] <= 40:         # every sub-iteration, with its count
            img = lab
            for i, step in enumerate(trail):
                nxt, deleted = S._subiteration_host(img, i)
                assert np.array_equal(nxt, step) and deleted == int((img > 0).sum() - (step > 0).sum()), (name, i)
                img = nxt
            seen += len(trail)
    assert seen > 100
    assert thinned["a disc of radius 24"].subiterations > 2 * 8 and thinned["label_frame 300 x 517"].subiterations > 8


def test_small_cases_pixel_for_pixel():
    for name, lab, left, n in K.small_cases():
        got = S.skeletonize_labels(lab)
        assert sorted(map(tuple, np.argwhere(N(got.labels) > 0).tolist())) == sorted(left) and got.subiterations == n, name
    for n in range(2, 34):                                   # the fact MAX_SUBITERATIONS is derived from
        assert S.skeletonize_labels(np.ones((n, n), np.int32)).subiterations == n - 1, n
    assert S.MAX_SUBITERATIONS >= 2 * (32767 - 1)


def test_a_skeleton_is_a_fixed_point(shapes, thinned):
    for name, lab in shapes:
        again = S.skeletonize_labels(thinned[name].labels)
        assert again.subiterations == 0 and torch.equal(again.labels, thinned[name].labels), name


def test_relabelling_permutes_and_neighbours_do_not_matter(shapes, thinned):
    for name in ("dense blobs, 3 ids, 40 x 29", "two large instances that share a long straight border", "label_frame 300 x 517"):
        lab = dict(shapes)[name]
        k = int(lab.max())
        perm = np.concatenate([[0], np.random.default_rng(5).permutation(k) + 1]).astype(np.int32)
        got = S.skeletonize_labels(perm[lab])
        assert np.array_equal(N(got.labels), perm[N(thinned[name].labels)]) and got.subiterations == thinned[name].subiterations, name
    for name in ("dense blobs, 3 ids, 40 x 29", "two large instances that share a long straight border", "non-compact ids"):
        lab = dict(shapes)[name]
        whole, most = N(thinned[name].labels), 0
        for i in np.unique(lab[lab > 0]):
            alone = S.skeletonize_labels(np.where(lab == i, lab, 0))
            assert np.array_equal(N(alone.labels), np.where(lab == i, whole, 0)), (name, i)
            most = max(most, alone.subiterations)
        assert most == thinned[name].subiterations, name


def test_topology_is_kept(shapes, thinned):
    from ullsam_amd.utils.outline import label_outlines
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    for name, lab in shapes:
        sk = N(thinned[name].labels)
        ids = np.unique(np.concatenate([[0], lab.reshape(-1)]))
        assert np.array_equal(np.unique(np.concatenate([[0], sk.reshape(-1)])), ids), name            # every label present stays present
        assert np.array_equal(sk[sk > 0], lab[sk > 0]), name                                          # and nothing is added or renamed
        a, b = np.searchsorted(ids, lab).astype(np.int32), np.searchsorted(ids, sk).astype(np.int32)   # (compact ids for the outline tables)
        k = len(ids) - 1
        if k == 0:
            continue
        before, after = label_outlines(a, connectivity=8, num=k), label_outlines(b, connectivity=8, num=k)
        count = lambda o, sign: np.bincount(N(o.label)[sign * N(o.area2) > 0], minlength=k + 1).tolist()      # outer loops (+1), holes (-1) per label
        assert count(before, 1) == count(after, 1) and count(before, -1) == count(after, -1), name
        if ndi is not None and lab.size <= 60000:
            for i in range(1, k + 1):
                ca, cb = (ndi.label(img == i, structure=np.ones((3, 3), int))[1] for img in (a, b))
                ha, hb = (ndi.label(~np.pad(img == i, 1))[1] - 1 for img in (a, b))                  # 4-connected background, less the outside
                assert (ca, ha) == (cb, hb), (name, i)


def _table_equal(got, want, k, what):
    for f in K.FIELDS:
        t = getattr(got, f)
        assert t.dtype == torch.int64 and tuple(t.shape) == (k,) and t.tolist() == [int(v) for v in want[f]], (what, f)


def test_links_degrees_and_node_classes_against_the_loops(shapes, thinned):
    for name, lab in shapes:
        if lab.size > 60000 or int(lab.max()) > 1000:
            continue
        sk = N(thinned[name].labels)
        k = int(lab.max())
        for img, tag in ((sk, "skeleton"), (lab, "labels")):             # (any label image is taken as it is: thick pixels have high degrees)
            got = S.measure_skeletons(img.astype(np.int32), num_ids=k)
            _table_equal(got, K.measure(img, k), k, (name, tag))
            assert got.d2_sum is None and got.d2_min is None and got.d2_max is None
            nodes = S.node_image(img.astype(np.int32))
            assert nodes.dtype == torch.uint8 and np.array_equal(nodes.numpy(), K.node_image(img)), (name, tag)
            px, ep, jn, iso, lo, ld, ds = (N(getattr(got, f)) for f in K.FIELDS)
            assert np.array_equal(ds, 2 * (lo + ld)), (name, tag)
            two = np.bincount(img[nodes.numpy() == 2], minlength=k + 1)[1:k + 1]
            assert np.array_equal(px, ep + jn + iso + two), (name, tag)


def test_known_rows():
    row = np.zeros((3, 11), np.int32)
    row[1, 1:10] = 1
    t = S.measure_skeletons(row)
    assert (t.pixels.tolist(), t.end_points.tolist(), t.links_orth.tolist(), t.links_diag.tolist(), t.junctions.tolist()) == ([9], [2], [8], [0], [0])
    diag = np.eye(9, dtype=np.int32)[::-1].copy()
    t = S.measure_skeletons(diag)
    assert (t.links_diag.tolist(), t.links_orth.tolist(), t.end_points.tolist()) == ([8], [0], [2])
    plus = np.zeros((7, 7), np.int32)
    plus[3, :] = 2
    plus[:, 3] = 2
    t = S.measure_skeletons(plus)
    assert t.junctions.tolist() == [0, 1] and t.end_points.tolist() == [0, 4] and t.pixels.tolist() == [0, 13]
    assert S.node_image(plus)[3, 3] == 3 and S.node_image(plus)[0, 3] == 1 and S.node_image(plus)[1, 3] == 2 and S.node_image(plus)[0, 0] == 0
    one = np.zeros((3, 3), np.int32)
    one[1, 1] = 1
    t = S.measure_skeletons(one)
    assert t.isolated.tolist() == [1] and t.degree_sum.tolist() == [0] and S.node_image(one)[1, 1] == 4
    corner = np.array([[1, 1], [0, 1]], np.int32)                           # an L-corner is no triangle: the diagonal is no link
    t = S.measure_skeletons(corner)
    assert t.links_orth.tolist() == [2] and t.links_diag.tolist() == [0] and t.end_points.tolist() == [2]
    props = S.derive_skeletons(S.measure_skeletons(diag, num_ids=2), pixel_size=0.5)
    assert props["length"][0] == 8 * np.sqrt(2.0) * 0.5 and np.isnan(props["length"][1]) and "mean_width" not in props


def test_widths_against_a_gather_of_inner_distance(shapes, thinned):
    for name in ("a ring with a hole", "dense blobs, 3 ids, 40 x 29", "two large instances that share a long straight border", "branched filaments 200 x 260"):
        lab = dict(shapes)[name]
        k = int(lab.max()) + 1                                               # (one absent id at the end)
        d2 = D.inner_distance(lab)
        sk = thinned[name].labels
        got = S.measure_skeletons(sk, num_ids=k, d2=d2)
        assert got.d2_sum.dtype == torch.int64 and got.d2_min.dtype == torch.int32 and got.d2_max.dtype == torch.int32
        for i in range(1, k + 1):
            v = N(d2)[N(sk) == i]
            want = (int(v.sum()), int(v.min()), int(v.max())) if v.size else (0, INT_MAX, -1)
            assert (int(got.d2_sum[i - 1]), int(got.d2_min[i - 1]), int(got.d2_max[i - 1])) == want, (name, i)
        loops = K.measure(N(sk), k, N(d2)) if lab.size < 3000 else None
        if loops:
            assert got.d2_sum.tolist() == loops["d2_sum"] and got.d2_min.tolist() == loops["d2_min"] and got.d2_max.tolist() == loops["d2_max"], name
        props = S.derive_skeletons(got, 2.0)
        assert props["max_width"][0] == 2.0 * np.sqrt(float(got.d2_max[0])) * 2.0 and np.isnan(props["mean_width"][k - 1])
        assert props["min_width"][0] <= props["mean_width"][0] <= props["max_width"][0]


def test_errors_and_routing():
    lab = R.blobs(5, 12, 12)
    want = S.skeletonize_labels(lab)
    for labels in (torch.from_numpy(lab), torch.from_numpy(lab.astype(np.int64))):
        got = S.skeletonize_labels(labels, device="cpu")
        assert not got.labels.is_cuda and torch.equal(got.labels, want.labels) and got.subiterations == want.subiterations
    bad = lab.copy()
    bad[0, 0] = -1
    d2 = D.inner_distance(lab)
    calls = {"[H, W]": lambda: S.skeletonize_labels(lab[0]), "0 x 4": lambda: S.skeletonize_labels(np.zeros((0, 4), np.int32)),
             "32768": lambda: S.skeletonize_labels(np.zeros((1, 32768), np.int32)), "-1": lambda: S.skeletonize_labels(lab, max_subiterations=-1),
             str(2 ** 30 + 1): lambda: S.skeletonize_labels(lab, max_subiterations=2 ** 30 + 1), "1.0": lambda: S.skeletonize_labels(lab, max_subiterations=1.0),
             "True": lambda: S.skeletonize_labels(lab, max_subiterations=True), "'fast'": lambda: S.skeletonize_labels(lab, route="fast"),
             "negative": lambda: S.skeletonize_labels(bad), "= 0": lambda: S.skeletonize_labels(lab, block=0),
             f"0..{int(lab.max()) - 1}": lambda: S.measure_skeletons(lab, num_ids=int(lab.max()) - 1), "= -2": lambda: S.measure_skeletons(lab, num_ids=-2),
             "a negative": lambda: S.measure_skeletons(bad), "[12, 12]": lambda: S.measure_skeletons(lab, d2=d2[:5]),
             "int32": lambda: S.measure_skeletons(lab, d2=d2.to(torch.int64)), "(12,)": lambda: S.node_image(lab[0])}
    for number, call in calls.items():
        with pytest.raises(ValueError) as e:
            call()
        assert number in str(e.value), (number, str(e.value))
    n = want.subiterations
    assert n >= 2
    assert torch.equal(S.skeletonize_labels(lab, max_subiterations=n).labels, want.labels)
    with pytest.raises(_lib.UllsamError) as e:
        S.skeletonize_labels(lab, max_subiterations=n - 1)
    assert f"max_subiterations = {n - 1}" in str(e.value)
    assert S.skeletonize_labels(np.zeros((4, 5), np.int32), max_subiterations=0).subiterations == 0


def test_filament_generator():
    from ullsam_amd.utils import synthetic as SY
    a, b = SY.filament_frame(3, 200, 260, 5), SY.filament_frame(3, 200, 260, 5)
    assert a.dtype == np.int32 and a.shape == (200, 260) and np.array_equal(a, b) and not np.array_equal(a, SY.filament_frame(4, 200, 260, 5))
    sk = S.skeletonize_labels(a)
    t = S.measure_skeletons(sk.labels)
    assert int(t.junctions.sum()) >= 2 and int(t.end_points.sum()) >= 6 and 0.02 < (a > 0).mean() < 0.5      # branched, thin, sparse


def test_abi_and_symbols():
    from ullsam_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert _lib.ABI_VERSION == 14 == lib.ullsam_abi_version() == int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1))
    names = ["ullsam_skel_step", "ullsam_skel_tile", "ullsam_skel_measure"]
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("ullsam_skel_")) == sorted(names)
    for s in names:
        assert hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    from ullsam_amd import ops
    assert ops.SKEL_BLOCK % ops.SKEL_TILE_STEPS == 0 and ops.SKEL_TILE_STEPS % 2 == 0 and tuple(ops.SKEL_FIELDS) == tuple(K.FIELDS) == tuple(S.COUNT_FIELDS)


def test_skeleton_kernels_have_no_spill_and_no_scratch():
    from ullsam_amd import build, ops
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels()
    others = [v for n, v in vars(KR).items() if n.startswith("HOT") and n != "HOT_SKELETON"]
    for pat in KR.HOT_SKELETON:                                                   # a list of its own, in no aggregate
        assert all(pat not in other for other in others), pat
        assert sum(1 for n in ks if re.search(pat, n)) == 1, pat
    for n in ks:                                                                  # and no older pattern takes one of its kernels
        if "skel_" in n:
            assert not any(re.search(h, n) for other in others for h in other), n
    hot = {n: r for n, r in ks.items() if any(re.search(h, n) for h in KR.HOT_SKELETON)}
    assert len(hot) == 3, sorted(hot)
    for n, r in hot.items():
        assert not (r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)), (n, r)
    s, (ch, cw) = ops.SKEL_TILE_STEPS, ops.SKEL_TILE
    lds = [r.get("group_segment_fixed_size", 0) for n, r in hot.items() if "skel_lds_kernel" in n]
    assert lds == [2 * 4 * (cw + 2 * s) * (ch + 2 * s) + 4 * s + 4]               # two images of the core and its halo, a counter per sub-iteration, one word
