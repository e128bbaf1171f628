"""Connected regions on the GPU (csrc/regions.hip): 8-connected labelling, small-region removal, inverse RLE and the generator's
min_mask_region_area step.  Every result depends only on region membership and integer sizes, so every assertion is exact equality:
labels against scipy.ndimage.label (each scipy label mapped to the minimum linear index of its region), removal against the host
utils.amg.remove_small_regions mask by mask, inverse RLE against utils.amg.rle_to_mask, and the generator step with
device_small_regions=True against the same step with False (the host loop)."""
import copy

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu
DEV = "cuda"
EIGHT = np.ones((3, 3), dtype=np.uint8)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- patterns ----------------------------------------------------------------------------------------------------------------
def _serpentine(h, w):
    """One-pixel-wide path: every other row filled, joined alternately at the right and the left end: ONE region that crosses every
    vertical tile border once per row (long parent chains); its complement is one region per odd row."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for y in range(1, h, 2):
        m[y, w - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def _rings(h, w):
    yy, xx = np.mgrid[:h, :w]
    return (np.maximum(np.abs(yy - h // 2), np.abs(xx - w // 2)) % 6) < 3


def _corners(h, w):
    m = np.zeros((h, w), bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    return m


def _noise(fill, seed):
    return lambda h, w: np.random.default_rng(seed).random((h, w)) < fill


PATTERNS = {
    "empty": lambda h, w: np.zeros((h, w), bool),
    "full": lambda h, w: np.ones((h, w), bool),
    "corners": _corners,
    "eye": lambda h, w: np.eye(h, w, dtype=bool),
    "checker": lambda h, w: (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0,
    "serpentine": _serpentine,
    "rings": _rings,
    "noise05": _noise(0.05, 1),
    "noise50": _noise(0.5, 2),
    "noise95": _noise(0.95, 3),
}
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (517, 643), (1024, 1024)]


def _speckled_disc(h, w, cy, cx, r, seed, p=0.001):
    yy, xx = np.mgrid[:h, :w]
    disc = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return disc ^ (np.random.default_rng(seed).random((h, w)) < p), disc


def _ref_labels(mask, background):
    """scipy's regions, each renamed to the minimum linear index of its pixels (= its first pixel in raster order)."""
    work = ~mask if background else mask
    lab, n = ndimage.label(work, structure=EIGHT)
    flat = lab.reshape(-1)
    vals, first = np.unique(flat, return_index=True)
    table = np.full(n + 1, -1, np.int64)
    table[vals] = first
    table[0] = -1
    return table[flat].reshape(mask.shape).astype(np.int32)


def _check_labels(masks):
    from ullsam_amd.utils import amg as A
    stack = np.stack(masks)
    for background in (False, True):
        got = A.label_regions(T(stack.astype(np.uint8)), background=background)
        assert got.dtype == torch.int32 and got.shape == stack.shape
        got = got.cpu().numpy()
        for i, m in enumerate(masks):
            assert np.array_equal(got[i], _ref_labels(m, background)), (i, background, m.shape)


# ---- 1. labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_regions_matches_scipy(shape):
    """utils.amg.label_regions (ullsam_label_regions) against the 8-connected reference labelling of this file, every pattern, as one batch and mask by mask."""
    masks = [f(*shape) for f in PATTERNS.values()]
    _check_labels(masks)                       # all patterns as one batch: a mask must not leak labels into its neighbour
    for m in masks[:4]:
        _check_labels([m])                     # N = 1


@pytest.mark.parametrize("n", [1, 3, 17])
def test_label_regions_batches_mix_patterns(n):
    names = list(PATTERNS)
    for shape in ((64, 64), (517, 643)):
        _check_labels([PATTERNS[names[(3 * i + n) % len(names)]](*shape) for i in range(n)])


def test_label_regions_2048():
    _check_labels([_noise(0.5, 7)(2048, 2048)])


def test_label_regions_bool_input_and_2d():
    from ullsam_amd.utils import amg as A
    m = _rings(70, 90)
    got = A.label_regions(T(m))
    assert got.shape == (70, 90) and np.array_equal(got.cpu().numpy(), _ref_labels(m, False))


# ---- 2. removal -----------------------------------------------------------------------------------------------------------------
THRESHOLDS = [1, 2, 50, 200, 10 ** 9, 7.5]


def _check_removal(masks, thresholds=THRESHOLDS, modes=("holes", "islands")):
    from ullsam_amd.utils import amg as A
    stack = T(np.stack(masks).astype(np.uint8))
    n_changed = 0
    for mode in modes:
        for thr in thresholds:
            got, changed = A.remove_small_regions_batched(stack, thr, mode)
            assert got.dtype == torch.uint8 and changed.dtype == torch.bool and changed.shape == (len(masks),)
            got, changed = got.cpu().numpy(), changed.cpu().numpy()
            for i, m in enumerate(masks):
                want, want_changed = A.remove_small_regions(m, thr, mode)
                assert bool(changed[i]) == want_changed, (i, mode, thr)
                assert np.array_equal(got[i].astype(bool), want), (i, mode, thr)
                n_changed += want_changed
    return n_changed


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (64, 64), (517, 643)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_remove_small_regions_matches_host(shape):
    """utils.amg.remove_small_regions_batched (ullsam_remove_small_regions) against the host form of amg.py:267-291, holes and islands."""
    masks = [f(*shape) for f in PATTERNS.values()]
    masks.append(_speckled_disc(*shape, shape[0] / 2, shape[1] / 2, min(shape) / 3, 5, p=0.01)[0])
    n_changed = _check_removal(masks)
    assert shape == (1, 1) or n_changed > 0


def test_remove_small_regions_1024_and_2048():
    _check_removal([_speckled_disc(1024, 1024, 400, 600, 300, 11)[0], _noise(0.5, 12)(1024, 1024), _serpentine(1024, 1024)], thresholds=[50, 10 ** 9])
    _check_removal([_speckled_disc(2048, 2048, 900, 1100, 500, 13)[0]], thresholds=[200])


def _blocks(h, w, blocks):
    m = np.zeros((h, w), bool)
    for y, x, bh, bw in blocks:
        m[y:y + bh, x:x + bw] = True
    return m


def test_remove_small_regions_edge_rules():
    from ullsam_amd.utils import amg as A
    # a region whose size EQUALS the threshold stays (strict <); one pixel more of threshold removes it
    eq = _blocks(100, 150, [(5, 5, 5, 10), (40, 40, 30, 30)])
    for m in (eq, ~eq):
        mode = "islands" if m is eq else "holes"
        _check_removal([m], thresholds=[50, 51, 49.5, 50.5], modes=(mode,))
    got, changed = A.remove_small_regions_batched(T(eq[None]), 50, "islands")
    assert not bool(changed[0]) and got.dtype == torch.bool and np.array_equal(got[0].cpu().numpy(), eq)
    got, changed = A.remove_small_regions_batched(T(eq[None]), 51, "islands")
    assert bool(changed[0]) and np.array_equal(got[0].cpu().numpy(), _blocks(100, 150, [(40, 40, 30, 30)]))
    # every island small, two of equal largest size: the one whose first pixel comes first in raster order stays, although the other
    # one lies further left and a smaller island comes before both
    tie = _blocks(100, 150, [(2, 2, 2, 2), (10, 40, 3, 3), (12, 5, 3, 3), (50, 90, 2, 4)])
    got, changed = A.remove_small_regions_batched(T(tie[None]), 50, "islands")
    assert bool(changed[0]) and np.array_equal(got[0].cpu().numpy(), _blocks(100, 150, [(10, 40, 3, 3)]))
    # one island above the threshold: it alone is kept
    one = _blocks(100, 150, [(2, 2, 3, 3), (20, 20, 10, 10), (60, 100, 2, 2)])
    got, changed = A.remove_small_regions_batched(T(one[None]), 50, "islands")
    assert bool(changed[0]) and np.array_equal(got[0].cpu().numpy(), _blocks(100, 150, [(20, 20, 10, 10)]))
    _check_removal([tie, one, eq, ~tie])
    # an empty mask is unchanged in both modes at any threshold; a full one too
    _check_removal([np.zeros((33, 65), bool), np.ones((33, 65), bool)])


def test_holes_then_islands_as_the_generator():
    from ullsam_amd.utils import amg as A
    masks = [_speckled_disc(517, 643, 250, 300, 120, 21)[0], _speckled_disc(517, 643, 100, 500, 60, 22, p=0.01)[0], _rings(517, 643),
             _noise(0.5, 23)(517, 643)]
    for thr in (50, 200, 7.5):
        a, ch1 = A.remove_small_regions_batched(T(np.stack(masks)), thr, "holes")
        b, ch2 = A.remove_small_regions_batched(a, thr, "islands")
        b, ch = b.cpu().numpy(), (ch1 | ch2).cpu().numpy()
        for i, m in enumerate(masks):
            w1, c1 = A.remove_small_regions(m, thr, "holes")
            w2, c2 = A.remove_small_regions(w1, thr, "islands")
            assert np.array_equal(b[i], w2) and bool(ch[i]) == (c1 or c2)


# ---- 3. inverse RLE -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (64, 64), (517, 643)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rle_to_mask_device_matches_host(shape):
    from ullsam_amd.utils import amg as A
    masks = [f(*shape) for f in PATTERNS.values()]                       # "full", "corners", "eye", ... start with a 1-run
    masks.append(_speckled_disc(*shape, shape[0] / 2, shape[1] / 2, min(shape) / 3, 5)[0])
    rles = A.mask_to_rle_pytorch(T(np.stack(masks)))
    assert any(r["counts"][0] == 0 for r in rles)
    got = A.rle_to_mask_device(rles, DEV)
    assert got.dtype == torch.uint8 and got.shape == (len(masks),) + shape
    got = got.cpu().numpy()
    for i, r in enumerate(rles):
        assert np.array_equal(got[i].astype(bool), A.rle_to_mask(r)) and np.array_equal(got[i].astype(bool), masks[i])
    arr = [{"size": r["size"], "counts": np.asarray(r["counts"], np.int64)} for r in rles]      # the generator's array form
    assert torch.equal(A.rle_to_mask_device(arr, DEV), T(got))


def test_rle_to_mask_device_long_records():
    """More runs than one scan chunk (2048) and runs longer than a column."""
    from ullsam_amd.utils import amg as A
    masks = [_noise(0.5, 31)(300, 200), _blocks(300, 200, [(0, 10, 300, 50), (7, 100, 200, 3)]), _serpentine(300, 200)]
    rles = A.mask_to_rle_pytorch(T(np.stack(masks)))
    assert max(len(r["counts"]) for r in rles) > 3 * 2048 and max(max(r["counts"]) for r in rles) > 5 * 300
    got = A.rle_to_mask_device(rles, DEV).cpu().numpy().astype(bool)
    for i, m in enumerate(masks):
        assert np.array_equal(got[i], m)


def test_rle_to_mask_device_rejects_malformed_counts():
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import amg as A
    h, w = 40, 30
    good = A.mask_to_rle_pytorch(T(_rings(h, w)[None]))[0]
    for counts in ([h * w - 1], [h * w + 1], [10, -3, h * w - 7], good["counts"] + [5], good["counts"][:-1], [], [0, 2 ** 40]):
        with pytest.raises(_lib.UllsamError):
            A.rle_to_mask_device([good, {"size": [h, w], "counts": counts}, good], DEV)
    with pytest.raises(_lib.UllsamError):
        A.rle_to_mask_device([good, {"size": [h, w + 1], "counts": [h * (w + 1)]}], DEV)
    # an over-long record between two good ones: flagged, and its neighbours' masks are untouched
    bad = [5, 10 * h * w, 7, 10 * h * w]
    cs = [np.asarray(c, np.int32) for c in (good["counts"], bad, good["counts"])]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    masks, status = ops.rle_to_mask(T(np.concatenate(cs)), T(offs), h, w)
    assert status.cpu().tolist() == [0, 1, 0]
    for i in (0, 2):
        assert np.array_equal(masks[i].cpu().numpy().astype(bool), _rings(h, w))


# ---- 4. the generator step ------------------------------------------------------------------------------------------------------
def _speckled_set(h, w, seed):
    """Discs with 0.1 % salt-and-pepper noise, three of them also as a clean copy: the cleaned speckled disc has the clean copy's box,
    so the NMS (which prefers unchanged masks) has records to drop."""
    rng = np.random.default_rng(seed)
    masks = []
    for i in range(10):
        r = int(rng.integers(min(h, w) // 12, min(h, w) // 5))
        cy, cx = int(rng.integers(r, h - r)), int(rng.integers(r, w - r))
        noisy, disc = _speckled_disc(h, w, cy, cx, r, seed * 100 + i)
        masks.append(noisy)
        if i < 3:
            masks.append(disc)
    return masks


def _mask_data(masks):
    from ullsam_amd.utils import amg as A
    n = len(masks)
    h, w = masks[0].shape
    dev_masks = T(np.stack(masks).astype(np.uint8))
    rng = np.random.default_rng(n)
    return A.MaskData(rles=A.mask_to_rle_pytorch(dev_masks), boxes=A.batched_mask_to_box(dev_masks),
                      iou_preds=T(rng.random(n).astype(np.float32)), points=T(rng.random((n, 2)).astype(np.float32) * w),
                      stability_score=T(rng.random(n).astype(np.float32)), crop_boxes=T(np.tile(np.asarray([[0, 0, w, h]]), (n, 1))))


@pytest.mark.parametrize("shape,seed", [((512, 640), 1), ((1024, 1024), 2)], ids=["512x640", "1024x1024"])
def test_postprocess_small_regions_device_equals_host(shape, seed):
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import amg as A
    masks = _speckled_set(*shape, seed)
    min_area, nms_thresh = 100, 0.7
    host_changed = 0
    for m in masks:                                            # the conditions against a vacuous pass, from the host definition
        a, c1 = A.remove_small_regions(m, min_area, "holes")
        _, c2 = A.remove_small_regions(a, min_area, "islands")
        host_changed += bool(c1 or c2)
    assert 2 * host_changed >= len(masks)
    data = _mask_data(masks)
    out = {}
    for device in (False, True):
        gen = SamAutomaticMaskGenerator(None, points_per_side=2, device_small_regions=device)
        out[device] = gen.postprocess_small_regions(copy.deepcopy(data), min_area, nms_thresh)
    host, dev = out[False], out[True]
    assert len(host["rles"]) < len(masks)                      # the NMS dropped a record
    assert len(dev["rles"]) == len(host["rles"])
    for a, b in zip(dev["rles"], host["rles"]):
        assert a["size"] == b["size"] and [int(v) for v in a["counts"]] == [int(v) for v in b["counts"]]
    for key in ("boxes", "iou_preds", "points", "stability_score", "crop_boxes"):
        assert dev[key].dtype == host[key].dtype and torch.equal(dev[key], host[key]), key
    assert any(list(map(int, a["counts"])) != list(map(int, r["counts"])) for a, r in zip(host["rles"], data["rles"]))   # something was re-encoded


def test_generate_with_min_mask_region_area_device_equals_host():
    from tests.test_amg_gpu import _small_sam
    from tests import util as U
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    sam, _ = _small_sam()
    img = torch.from_numpy(U.rand_image((3, 512, 640), 23, 255.0))
    kw = dict(points_per_side=4, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.3, stability_score_offset=0.05,
              min_mask_region_area=200)
    host = SamAutomaticMaskGenerator(sam, device_small_regions=False, **kw).generate(img)
    dev = SamAutomaticMaskGenerator(sam, **kw).generate(img)
    assert len(dev) == len(host) > 0
    for a, b in zip(dev, host):
        assert a.keys() == b.keys()
        assert np.array_equal(a["segmentation"], b["segmentation"])
        for key in a:
            if key != "segmentation":
                assert a[key] == b[key], key


# ---- 5. reproducibility -----------------------------------------------------------------------------------------------------------
def test_remove_small_regions_is_bit_reproducible_2048():
    from ullsam_amd.utils import amg as A
    stack = T(np.stack([_noise(0.5, 41)(2048, 2048), _speckled_disc(2048, 2048, 1000, 900, 600, 42)[0], _rings(2048, 2048)]).astype(np.uint8))
    for mode in ("holes", "islands"):
        runs = [A.remove_small_regions_batched(stack, 200, mode, return_labels=True) for _ in range(2)]
        for x, y in zip(*runs):
            assert torch.equal(x, y)
        assert runs[0][2].dtype == torch.int32 and bool(runs[0][1].any())
