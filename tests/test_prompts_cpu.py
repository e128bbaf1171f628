"""Prompts from an instance label image, host side (ullsam_amd/utils/prompts.py): the brute-force definitions (tests/prompts_ref.py) against the
reference's literal scipy statements (train_joint_v2.py:342-343, 423-435), the numpy host route against the brute-force definitions, the draw rule,
the PromptSet's shapes and dtypes, the empty image and the instance that fills the frame."""
import functools

import numpy as np
import pytest

from tests import prompts_ref as R
from ullsam_amd.utils import prompts as P

FIELDS = ("ids", "coords", "point_labels", "boxes", "masks", "counts")


def _scene_scipy():
    """96 x 80: a disc, a thin bar (no interior), two touching blobs, a blob cut by the frame"""
    lab = np.zeros((96, 80), np.int32)
    R._disc(lab, 30, 25, 17, 1)
    lab[60:66, 10:60] = 2
    R._disc(lab, 30, 58, 14, 3)
    lab[20:45, 40:50][lab[20:45, 40:50] == 0] = 4          # fills the gap between discs 1 and 3: touches both
    R._disc(lab, 92, 70, 16, 5)
    return lab


@functools.lru_cache(maxsize=None)
def _scene(name):
    lab = getattr(R, name)()
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _d1(name):
    return R.d1(_scene(name))


@functools.lru_cache(maxsize=None)
def _ref(name, kw=()):
    """the brute-force PromptSet of a scene, computed once per (scene, arguments) and shared; kw as sorted items"""
    return R.prompts(_scene(name), **{k: (list(v) if k == "ids" else v) for k, v in kw})


def _key(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))


def _same(ps, ref):
    for f in FIELDS:
        got, want = np.asarray(getattr(ps, f)), ref[f]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), f


def test_brute_force_sets_equal_the_reference_scipy_statements():
    ndimage = pytest.importorskip("scipy").ndimage
    lab = _scene_scipy()
    d1_all, d1_fast = R.d1(lab, restrict=False), R.d1(lab, restrict=True)
    assert np.array_equal(d1_all, d1_fast)
    for i in (1, 2, 3, 4, 5):
        m = (lab == i).astype(np.float32)
        eroded = ndimage.binary_erosion(m, iterations=10)
        dilated = ndimage.binary_dilation(m, iterations=10)
        dist = ndimage.distance_transform_edt(np.logical_not(np.logical_xor(m, ndimage.binary_erosion(m))))
        ring = np.logical_and(np.logical_and(dist >= 9, dist <= 11), np.logical_not(m))
        assert np.array_equal(R.inner_set(lab, i, 10, d1_all), eroded), i
        assert np.array_equal(R.d2(lab, i, restrict=False), R.d2(lab, i, restrict=True)), i
        assert np.array_equal(R.ring_set(lab, i, (9, 11)), ring), i
        assert np.array_equal(R.l1_to_instance(lab, i) > 10, np.logical_not(dilated)), i
    assert not R.inner_set(lab, 2, 10, d1_all).any() and R.inner_set(lab, 1, 10, d1_all).any()
    inner, ring = P.candidate_sets(lab, [1, 2, 3, 4, 5])
    for n, i in enumerate((1, 2, 3, 4, 5)):
        assert np.array_equal(inner[n], R.inner_set(lab, i, 10, d1_all)) and np.array_equal(ring[n], R.ring_set(lab, i, (9, 11)))


@pytest.mark.parametrize("scene,kw", [
    ("scene_a", dict(max_instances=16)),
    ("scene_a", dict(max_instances=16, inner_radius=1, ring=(1, 2))),
    ("scene_a", dict(max_instances=3, seed=5)),
    ("scene_a", dict(ids=[8, 2, 5], seed=9)),
    ("scene_b", dict(num_pos=4, num_neg=2, max_instances=8)),
    ("scene_b", dict(max_instances=8, inner_radius=1, ring=(1, 2), seed=3)),
    ("scene_c", dict()),
    ("scene_d", dict()),
    ("scene_d", dict(inner_radius=2, ring=(20, 20))),
])
def test_host_route_equals_the_brute_force_definitions(scene, kw):
    lab = _scene(scene)
    ref = _ref(scene, _key(kw))
    _same(P.prompts_from_labels(lab, **kw), ref)
    inner, ring = P.candidate_sets(lab, ref["ids"], kw.get("inner_radius", 10), kw.get("ring", (9, 11)))
    assert np.array_equal(inner, ref["inner"]) and np.array_equal(ring, ref["ring"])
    assert np.array_equal(np.minimum(_d1(scene), kw.get("inner_radius", 10) + 1), P.d1_truncated(lab, kw.get("inner_radius", 10)))


def test_scenes_take_every_branch():
    lab_a = _scene("scene_a")
    a = _ref("scene_a", _key(dict(max_instances=16)))
    assert a["ids"].tolist() == [1, 2, 3, 5, 7, 8]
    assert a["counts"][0, 0] > 0 and a["counts"][1, 0] == 0 and a["counts"][2, 0] == 0          # disc: interior; pixel and bar: centroid
    assert a["ring"][4][lab_a == 8].any() and a["ring"][5][lab_a == 7].any()                    # rings over the neighbour
    b = _ref("scene_b", _key(dict(num_pos=4, num_neg=2, max_instances=8)))
    assert b["ids"].tolist() == [2, 4, 11, 65535] and b["counts"][0, 0] == 3                     # cyclic: 0 < |inner| < num_pos
    assert b["coords"][0, 3].tolist() == b["coords"][0, 0].tolist()
    c = _ref("scene_c")
    assert c["counts"].shape == (1, 2) and c["counts"][0, 0] > 0 and c["counts"][0, 1] == 0      # no ring at all: the cyclic fallback
    assert _ref("scene_d")["counts"][0, 1] == 1                                                  # one ring pixel < num_neg: second fallback
    assert _ref("scene_d", _key(dict(inner_radius=2, ring=(20, 20))))["counts"][0, 1] == 0       # first fallback (36 far pixels)
    picked = R.choose(lab_a, 3, 5)
    assert len(picked) == 3 and picked != [1, 2, 3]


def test_draw_rule():
    for seed, inst, kind, k, m in [(0, 1, 0, 1, 1), (0, 7, 1, 16, 16), (2 ** 63 + 5, 65535, 3, 16, 1000), (123, 4, 2, 3, 5), (1, 2, 0, 16, 10 ** 9)]:
        picks = P.draw_points(seed, inst, kind, k, m)
        assert picks == R.draw_points(seed, inst, kind, k, m)
        assert len(set(picks)) == k and all(0 <= r < m for r in picks)
        assert picks == P.draw_points(seed, inst, kind, k, m)                                    # a function of (seed, id, kind, set size) only
        assert P.draw_points(seed, inst, kind, max(k - 1, 0), m) == picks[:max(k - 1, 0)]       # and the first picks do not depend on how many follow
    assert P.draw_points(0, 3, 1, 16, 10 ** 6) != P.draw_points(1, 3, 1, 16, 10 ** 6)            # two seeds differ
    assert P.draw_points(0, 3, 1, 16, 10 ** 6) != P.draw_points(0, 4, 1, 16, 10 ** 6)
    assert P.draw_points(0, 3, 1, 16, 10 ** 6) != P.draw_points(0, 3, 0, 16, 10 ** 6)
    # every rank can come out, and k = m yields a permutation
    assert sorted(P.draw_points(11, 2, 0, 7, 7)) == list(range(7))
    assert {P.draw_points(s, 1, 0, 1, 3)[0] for s in range(64)} == {0, 1, 2}
    # the first word against Random123's known answer for the all-zero block
    assert R.philox_word0(0, (0, 0, 0, 0)) == 0x6627E8D5


def test_dropping_another_instance_leaves_the_points_unchanged():
    lab = R.scene_a()
    full = P.prompts_from_labels(lab, max_instances=16, seed=4, num_pos=2)
    without = lab.copy()
    without[without == 2] = 0                                # the one-pixel instance is far from the disc (1) and its ring
    part = P.prompts_from_labels(without, max_instances=16, seed=4, num_pos=2)
    assert part.ids.tolist() == [1, 3, 5, 7, 8]
    assert np.array_equal(part.coords[0], full.coords[0]) and np.array_equal(part.counts[0], full.counts[0])
    only = P.prompts_from_labels(lab, ids=[1], seed=4, num_pos=2)
    assert np.array_equal(only.coords[0], full.coords[0])
    assert not np.array_equal(P.prompts_from_labels(lab, ids=[1], seed=5, num_pos=2).coords, only.coords)


def test_prompt_set_shapes_and_dtypes():
    lab = R.scene_a()
    ps = P.prompts_from_labels(lab, num_pos=2, num_neg=5)
    n = 4
    assert isinstance(ps, P.PromptSet) and ps._fields == FIELDS
    assert ps.ids.shape == (n,) and ps.ids.dtype == np.int32
    assert ps.coords.shape == (n, 7, 2) and ps.coords.dtype == np.float32
    assert ps.point_labels.shape == (n, 7) and ps.point_labels.dtype == np.int32 and ps.point_labels[0].tolist() == [1, 1, 0, 0, 0, 0, 0]
    assert ps.boxes.shape == (n, 4) and ps.boxes.dtype == np.float32
    assert ps.masks.shape == (n, 67, 131) and ps.masks.dtype == np.float32
    assert ps.counts.shape == (n, 2) and ps.counts.dtype == np.int32
    for k, i in enumerate(ps.ids):
        assert np.array_equal(ps.masks[k], (lab == i).astype(np.float32))
        for (x, y), pl in zip(ps.coords[k], ps.point_labels[k]):
            assert (lab[int(y), int(x)] == i) == bool(pl)                                        # positives inside, negatives outside
    assert P.prompts_from_labels(lab, return_masks=False).masks is None
    with pytest.raises(ValueError):
        P.prompts_from_labels(lab, num_pos=17)
    with pytest.raises(ValueError):
        P.prompts_from_labels(lab, ids=[4])                  # an absent id
    with pytest.raises(ValueError):
        P.prompts_from_labels(lab.astype(np.float32))


def test_empty_image_gives_the_default_instance():
    ps = P.prompts_from_labels(np.zeros((64, 48), np.int32), num_pos=2, num_neg=5)
    assert ps.ids.tolist() == [0] and not ps.masks.any() and ps.masks.shape == (1, 64, 48)
    assert ps.coords[0].tolist() == [[24, 32], [24, 32], [10, 10], [38, 10], [10, 54], [38, 54], [10, 10]]
    assert ps.point_labels[0].tolist() == [1, 1, 0, 0, 0, 0, 0] and ps.counts.tolist() == [[0, 0]] and ps.boxes.tolist() == [[0, 0, 0, 0]]
    _same(ps, R.prompts(np.zeros((64, 48), np.int32), num_pos=2, num_neg=5))


def test_arguments_are_checked_before_anything_runs():
    """Every argument error is a ValueError raised up front; none of these touches a device."""
    torch = pytest.importorskip("torch")
    lab = _scene("scene_a")
    for kw in (dict(inner_radius=65), dict(ring=(9, 65))):                   # the kernels' halo limit, not the host route's
        with pytest.raises(ValueError, match="<= 64"):
            P.prompts_from_labels(lab, device="cuda", **kw)
        with pytest.raises(ValueError, match="<= 64"):
            P.candidate_sets(lab, [1], kw.get("inner_radius", 10), kw.get("ring", (9, 11)), device="cuda")
    assert P.prompts_from_labels(_scene("scene_d"), inner_radius=2, ring=(20, 70)).counts.shape == (1, 2)
    with pytest.raises(ValueError, match="CPU tensor"):
        P.prompts_from_labels(torch.from_numpy(np.array(lab)))
    with pytest.raises(ValueError, match="not a GPU"):
        P.prompts_from_labels(lab, device="cpu")
    with pytest.raises(ValueError, match="integer image"):
        P.prompts_from_labels(lab.astype(np.float32), device="cuda")
    with pytest.raises(ValueError, match="integer image"):
        P.prompts_from_labels(torch.zeros((4, 4)), device="cuda")
    with pytest.raises(ValueError, match="0..65535"):
        P.prompts_from_labels(lab.astype(np.int64) + 2 ** 32)               # the host route checks the range in the labels' own width
    with pytest.raises(ValueError, match="GiB of device scratch"):
        P._check_scratch(65535, 1024, 1024)
    P._check_scratch(64, 1024, 1024)
    P._check_scratch(3971, 1024, 1024)
    with pytest.raises(ValueError, match="at most 3971"):
        P._check_scratch(3972, 1024, 1024)


def test_label_tile_is_the_microscopy_tile_of_the_same_seed():
    """utils.synthetic.label_tile labels the discs microscopy_tile draws: without noise the bright pixels are the labelled ones."""
    from ullsam_amd.utils import synthetic as S
    for seed, size, n, rr in ((7, 128, 6, (8.0, 20.0)), (3, 96, 14, (5.0, 30.0))):
        img, centres = S.microscopy_tile(seed, size, n, rr, noise=0.0)
        lab = S.label_tile(seed, size, n, rr)
        assert lab.dtype == np.int32 and lab.shape == (size, size) and lab.max() <= n
        assert np.array_equal(lab > 0, img[0] > 0.5)
        for i in np.unique(lab[lab > 0]):                                    # cell i + 1 lies around centre i (unless hidden)
            ys, xs = np.where(lab == i)
            assert np.hypot(xs - centres[i - 1, 0], ys - centres[i - 1, 1]).max() < rr[1]


def test_instance_filling_the_frame_raises():
    with pytest.raises(ValueError, match="fills the frame"):
        P.prompts_from_labels(np.full((40, 50), 2, np.int32))
    ps = P.prompts_from_labels(np.full((40, 50), 2, np.int32), num_neg=0)    # no negative asked for: nothing to fail
    assert ps.coords.shape == (1, 1, 2) and ps.counts[0, 0] == 20 * 30
