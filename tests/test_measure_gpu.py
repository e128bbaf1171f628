"""Per-instance measurements and contacts on the GPU (csrc/measure.hip): the device route against the numpy route of utils.measure (itself
checked against per-pixel loops in tests/test_measure_cpu.py), with the LDS table and without it, the status words, unaligned views inside
guarded buffers, and the measure= keyword of the two label-map drivers.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import measure_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGES = ((None, 0), (np.uint8, 1), (np.uint8, 3), (np.uint16, 4), (np.uint16, 0))   # (dtype, C); C = 0: [H, W]
SLOTS = 128                                                                          # ops.MEASURE_LDS_SLOTS: the LDS table on, the default (0: the direct route)
LARGE = (600, 520)                                                                   # the mosaic tests' frame: many workgroups


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _frames():
    from ullsam_amd.utils import synthetic as S
    f = R.frames()
    rng = np.random.default_rng(2)
    out = {
        "1x1": f["1x1"],
        "5x3": f["5x3"],
        "1x200": (np.repeat(rng.integers(0, 6, 40), 5).astype(np.int32).reshape(1, 200), 6),
        "64x64": (S.label_frame(5, 64, 64, 12, (3.0, 12.0)), 12),
        "128x64": (S.label_frame(6, 128, 64, 20, (3.0, 14.0)), 20),
        "discs 150x170": f["discs 150x170"],
        "discs 600x520": (S.label_frame(11, LARGE[0], LARGE[1], 150, (4.0, 40.0)), 150),
    }
    return out


@pytest.fixture(scope="module")
def frames():
    return _frames()


def _fields(t):
    return {n: getattr(t, n) for n in t._fields if getattr(t, n) is not None}


def _same(got, want, what):
    g, w_ = _fields(got), _fields(want)
    assert set(g) == set(w_), what
    for n in g:
        assert g[n].is_cuda and g[n].dtype == w_[n].dtype and g[n].shape == w_[n].shape and torch.equal(g[n].cpu(), w_[n]), (what, n)


@pytest.mark.parametrize("name", ["1x1", "5x3", "1x200", "64x64", "128x64", "discs 150x170", "discs 600x520"])
def test_device_route_equals_the_numpy_route(frames, name):
    from ullsam_amd.utils import measure as M
    lab, k = frames[name]
    lab_d = T(lab)
    for dtype, c in IMAGES:
        img = None if dtype is None else R.intensity(lab.shape[0], lab.shape[1], c, dtype)
        want = M.measure_instances(lab, img, num=k)
        img_d = None if img is None else T(img)
        for slots in (SLOTS, 0):
            got = M.measure_instances(lab_d, img_d, num=k, device=DEV, lds_slots=slots)
            _same(got, want, (name, dtype, c, slots))
            again = M.measure_instances(lab_d, img_d, num=k, device=DEV, lds_slots=slots)
            assert all(torch.equal(a, b) for a, b in zip(_fields(got).values(), _fields(again).values())), (name, dtype, c, slots, "two runs differ")
    # host inputs and num left to labels.max()
    _same(M.measure_instances(lab, None, device=DEV), M.measure_instances(lab), (name, "host input"))


@pytest.mark.parametrize("name", ["1x1", "5x3", "1x200", "64x64", "128x64", "discs 150x170", "discs 600x520"])
def test_contacts_equal_the_loops_and_tie_to_contact_edges(frames, name):
    from ullsam_amd.utils import measure as M
    lab, k = frames[name]
    want = R.contacts(lab)
    got = M.label_contacts(T(lab), num=k, device=DEV)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (len(want), 3)
    assert got.cpu().tolist() == [list(r) for r in want]
    assert torch.equal(got.cpu(), M.label_contacts(lab, num=k)) and torch.equal(got, M.label_contacts(T(lab), num=k, device=DEV))
    per = M.measure_instances(T(lab), num=k, device=DEV).perimeter                   # the invariant on the DEVICE outputs
    ce = torch.zeros(k + 1, dtype=torch.int64, device=DEV)
    ce.index_add_(0, got[:, 0], got[:, 2])
    ce.index_add_(0, got[:, 1], got[:, 2])
    assert torch.equal(per[:, 2], ce[1:]) and bool((per[:, 1] >= per[:, 2]).all())
    if name == "discs 600x520":
        assert len(want) > 20


def test_every_pixel_its_own_id():
    """K = 4096 on 64 x 64: 2048 labels per workgroup against 128 LDS slots -- the table and the direct route act within one launch --, the
    largest number of contact pairs per pixel, and max_pairs one below the true count."""
    from ullsam_amd import _lib
    from ullsam_amd.utils import measure as M
    lab = (np.arange(4096, dtype=np.int32) + 1).reshape(64, 64)
    img = R.intensity(64, 64, 3, np.uint8)
    want = M.measure_instances(lab, img, num=4096)
    for slots in (SLOTS, 16, 0):
        got = M.measure_instances(T(lab), T(img), num=4096, device=DEV, lds_slots=slots)
        _same(got, want, slots)
    npairs = 2 * 64 * 63
    pairs = M.label_contacts(T(lab), num=4096, max_pairs=npairs, device=DEV)
    assert tuple(pairs.shape) == (npairs, 3) and torch.equal(pairs.cpu(), M.label_contacts(lab, num=4096)) and bool((pairs[:, 2] == 1).all())
    with pytest.raises(_lib.UllsamError):
        M.label_contacts(T(lab), num=4096, max_pairs=npairs - 1, device=DEV)
    assert torch.equal(M.label_contacts(T(lab), num=4096, device=DEV), pairs)       # the next call succeeds


def test_one_label_over_1024x1024_with_saturated_uint16():
    """The whole-segment carry, and sums beyond 2^32 and beyond float32's integer range, against closed forms."""
    from ullsam_amd.utils import measure as M
    n = 1024
    lab = torch.ones((n, n), dtype=torch.int32, device=DEV)
    img = T(np.full((n, n), 65535, np.uint16))
    s1, s2 = n * (n - 1) // 2, (n - 1) * n * (2 * n - 1) // 6
    for slots in (SLOTS, 0):
        t = M.measure_instances(lab, img, num=1, device=DEV, lds_slots=slots)
        assert t.area.tolist() == [n * n] and t.box.tolist() == [[0, 0, n - 1, n - 1]]
        assert t.moments.tolist() == [[n * s1, n * s1, n * s2, n * s2, s1 * s1]]
        assert t.perimeter.tolist() == [[4 * n - 4, 4 * n, 0]]
        assert t.isum.tolist() == [[n * n * 65535]] and t.isum2.tolist() == [[n * n * 65535 ** 2]] and t.imin.tolist() == [[65535]] and t.imax.tolist() == [[65535]]
    assert n * n * 65535 ** 2 > 2 ** 51 and n * s2 > 2 ** 32 and n * n * 65535 > 2 ** 32      # (far past int32 and past float32's 2^24)
    assert tuple(M.label_contacts(lab, num=1, device=DEV).shape) == (0, 3)


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.uint16, 2), (np.uint8, 0)])
def test_unaligned_views_inside_guarded_buffers(frames, dtype, c):
    """Labels 4 bytes and the image one sample off a 16-byte boundary, every output a view inside a guarded buffer: the guards stay intact."""
    from ullsam_amd import ops
    from ullsam_amd.utils import measure as M
    lab, k = frames["discs 150x170"]
    h, w = lab.shape
    img = R.intensity(h, w, c, dtype)
    want = _fields(M.measure_instances(lab, img, num=k))
    pad = 64
    lbuf = np.ones((pad + h * w + pad,), np.int32)                                   # (1: a label that would be counted if the frame's surroundings were read)
    lbuf[pad + 1:pad + 1 + h * w] = lab.reshape(-1)
    lab_d = T(lbuf)[pad + 1:pad + 1 + h * w].view(h, w)
    ibuf = np.full((pad + img.size + pad,), 200, dtype)
    ibuf[pad + 1:pad + 1 + img.size] = img.reshape(-1)
    img_d = T(ibuf)[pad + 1:pad + 1 + img.size].view(img.shape)
    assert lab_d.data_ptr() % 16 == 4 and img_d.data_ptr() % 16 == img_d.element_size()
    for slots in (ops.MEASURE_LDS_SLOTS, 0):
        guard, bufs, out = -123456789, {}, {}
        for n, v in want.items():
            bufs[n] = torch.full((pad + v.numel() + pad,), guard, dtype=v.dtype, device=DEV)
            out[n] = bufs[n][pad + 1:pad + 1 + v.numel()].view(v.shape)
        fbuf = torch.full((pad + ops.MEASURE_FLAGS + pad,), guard, dtype=torch.int32, device=DEV)
        got, flags = ops.measure_instances(lab_d, k, img_d, slots, out=out, flags=fbuf[pad:pad + ops.MEASURE_FLAGS])
        assert flags.cpu().tolist()[0] == 0
        for n, v in want.items():
            assert got[n].data_ptr() == out[n].data_ptr() and torch.equal(out[n].cpu(), v), (n, slots)
            assert bool((bufs[n][:pad + 1] == guard).all()) and bool((bufs[n][pad + 1 + v.numel():] == guard).all()), (n, slots)
        assert bool((fbuf[:pad] == guard).all()) and bool((fbuf[pad + ops.MEASURE_FLAGS:] == guard).all())
    rows, flags = ops.label_contacts(lab_d, k, 64)
    fl = flags.cpu().tolist()
    ref = M.label_contacts(lab, num=k)
    assert fl[:2] == [0, 0] and fl[2] == fl[3] == len(ref)
    r = rows[:fl[2]].cpu()
    r = r[torch.argsort(r[:, 0])]
    assert torch.equal(torch.stack([r[:, 0] >> 32, r[:, 0] & 0xffffffff, r[:, 1]], 1), ref)


def test_ids_outside_the_range_raise_and_leave_the_process_usable(frames):
    from ullsam_amd import _lib
    from ullsam_amd.utils import measure as M
    lab, k = frames["discs 150x170"]
    img = R.intensity(lab.shape[0], lab.shape[1], 3, np.uint8)
    want, want_pairs = M.measure_instances(lab, img, num=k), M.label_contacts(lab, num=k)
    for value in (k + 1, -7, 2 ** 31 - 1):
        for where in ((70, 80), (0, 169), (149, 0), (33, 0)):                        # the interior, two corners, the left edge
            bad = lab.copy()
            bad[where] = value
            for slots in (SLOTS, 0):
                with pytest.raises(_lib.UllsamError):
                    M.measure_instances(T(bad), T(img), num=k, device=DEV, lds_slots=slots)
            with pytest.raises(_lib.UllsamError):
                M.label_contacts(T(bad), num=k, device=DEV)
        _same(M.measure_instances(T(lab), T(img), num=k, device=DEV), want, value)    # the next call is correct
        assert torch.equal(M.label_contacts(T(lab), num=k, device=DEV).cpu(), want_pairs)


def test_argument_checks_of_the_wrappers(frames):
    from ullsam_amd import _lib, ops
    lab = T(frames["5x3"][0])
    with pytest.raises(_lib.UllsamError):
        ops.measure_instances(lab, 5, torch.zeros((5, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(_lib.UllsamError):
        ops.measure_instances(lab, 5, torch.zeros((5, 3, 5), dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.UllsamError):
        ops.measure_instances(lab, 5, lds_slots=48)
    with pytest.raises(_lib.UllsamError):
        ops.measure_instances(torch.zeros((46341, 1), dtype=torch.int32, device=DEV), 0)
    with pytest.raises(_lib.UllsamError):
        ops.label_contacts(torch.zeros((1, 46341), dtype=torch.int32, device=DEV), 0)
    with pytest.raises(_lib.UllsamError):
        ops.label_contacts(lab, 5, max_pairs=0)
    t, flags = ops.measure_instances(lab, 0)                                        # K = 0: empty tables, every id is out of range
    assert t["area"].numel() == 0 and flags.cpu().tolist()[0] == 1


def test_drivers_return_the_table_of_their_labels():
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import amg as A
    from ullsam_amd.utils import measure as M
    from ullsam_amd.utils import mosaic as MZ
    from ullsam_amd.utils import synthetic as S
    from tests import util as U
    from tests.test_amg_gpu import _small_sam
    sam, _ = _small_sam()
    S.blob_decoder_init(sam)
    kw = dict(points_per_side=6, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05, box_nms_thresh=0.7)
    gen = SamAutomaticMaskGenerator(sam, output_mode="uncompressed_rle", **kw)
    img = np.ascontiguousarray((U.rand_image((3, 176, 176), 23, 255.0).transpose(1, 2, 0)).astype(np.uint8))
    tile, overlap = 96, 16
    # tiled
    labels0, records0 = gen.generate_tiled_label_map(img, tile=tile, overlap=overlap, min_visible_area=3)
    labels, records, table = gen.generate_tiled_label_map(img, tile=tile, overlap=overlap, min_visible_area=3, measure=True)
    assert torch.equal(labels, labels0) and records == records0 and int(labels.max()) >= 2
    _same(table, M.measure_instances(labels.cpu(), img), "tiled")
    grid = MZ.tile_grid(176, 176, tile, overlap)
    per_tile = [gen.generate_label_map(img[top:top + h, left:left + w]) for top, left, h, w in grid.boxes()]
    counts = [int(l.max()) for l, _ in per_tile]
    want, _, areas, boxes = MZ.stitch_label_maps(torch.stack([l for l, _ in per_tile]), counts, grid, min_visible_area=3, device=DEV)
    assert torch.equal(want, labels) and torch.equal(table.area, areas.to(torch.int64)) and torch.equal(table.box, boxes)
    # one tile
    small = np.ascontiguousarray(img[:90, :80])
    labels0, records0 = gen.generate_label_map(small)
    labels, records, table = gen.generate_label_map(small, measure=True)
    assert torch.equal(labels, labels0) and records == records0 and int(labels.max()) >= 1
    _same(table, M.measure_instances(labels.cpu(), small), "one tile")
    _, _, areas, boxes = A.paint_label_map([r["segmentation"] for r in records], order="area", device=DEV, size=small.shape[:2])
    assert torch.equal(table.area, areas.to(torch.int64)) and torch.equal(table.box, boxes)
    with pytest.raises(ValueError):
        gen.generate_label_map(small, out_hw=(45, 40), measure=True)
