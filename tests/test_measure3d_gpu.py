"""Per-object measurements and contacts of label volumes on the GPU (csrc/measure3d.hip; ops.measure_objects3d = ullsam_measure_objects3d,
ops.object_contacts3d = ullsam_object_contacts3d): the device route against the numpy route of utils.measure3d (itself checked against per-voxel
loops in tests/test_measure3d_cpu.py), with the LDS table at two sizes and without it, closed forms past 2^32, the status words, unaligned views
inside guarded buffers, and the measure= keyword of generate_stack_label_volume.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance3d_ref as R3
from tests import measure3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOTS = (128, 16, 0)                                                                 # the LDS table at its largest, a small one, the direct route
INT_MAX = 2 ** 31 - 1


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _whole_rows():
    """3 x 5 x 300: one run per row, of the widths 63 / 64 / 65 / 130 (and a whole row), placed across the 256-column tile edge and at the row's
    start -- whole 64-voxel segments that are carried, runs that end one voxel before, at and after a segment's end, and the tile seam at x = 256."""
    vol = np.zeros((3, 5, 300), np.int32)
    runs = [(193, 63), (192, 64), (192, 65), (128, 130), (224, 64), (126, 130), (0, 63), (0, 64), (0, 65), (0, 130), (0, 300), (64, 192), (191, 66),
            (255, 2), (170, 130)]
    for i, (x0, n) in enumerate(runs):
        vol[i // 5, i % 5, x0:x0 + n] = 1 + i % 4                                    # four ids: rows of one id touch along y and z, others are contacts
    return vol


def _volumes():
    from ullsam_amd import ops
    rng = np.random.default_rng(2)
    r, p = ops.MEASURE3D_TILE_R, ops.MEASURE3D_TILE_P
    out = {
        "1x1x1": (np.array([[[1]]], np.int32), 1),
        "2x3x5": (R3.blobs(7, 2, 3, 5), 9),
        "1x1x200 runs of 5": (np.repeat(rng.integers(0, 6, 40), 5).astype(np.int32).reshape(1, 1, 200), 6),
        "3x5x300 whole-row runs": (_whole_rows(), 5),
        "tiles along y and z": (R3.blobs(11, 2 * p + 1, 2 * r + 3, 300, n=40, ids=40), 42),          # three tiles along z, three along y, two along x
    }
    out.update({name: (vol, k) for name, vol, k in R.cases()})
    return out


VOLUMES = None


def _get(name):
    global VOLUMES
    if VOLUMES is None:
        VOLUMES = _volumes()
    return VOLUMES[name]


NAMES = ["1x1x1", "2x3x5", "1x1x200 runs of 5", "3x5x300 whole-row runs", "tiles along y and z"] + [name for name, _ in R3.cases()]


def _fields(t):
    return {n: getattr(t, n) for n in t._fields if getattr(t, n) is not None}


def _same(got, want, what):
    g, w_ = _fields(got), _fields(want)
    assert set(g) == set(w_), what
    for n in g:
        assert g[n].is_cuda and g[n].dtype == w_[n].dtype and g[n].shape == w_[n].shape and torch.equal(g[n].cpu(), w_[n]), (what, n)


@pytest.mark.parametrize("name", NAMES)
def test_device_route_equals_the_numpy_route(name):
    from ullsam_amd.utils import measure3d as M
    vol, k = _get(name)
    vol_d = T(vol)
    for dtype, c in R.IMAGES:
        img = R.image(vol, dtype, c)
        want = M.measure_objects(vol, img, num=k)
        img_d = None if img is None else T(img)
        for slots in SLOTS:
            got = M.measure_objects(vol_d, img_d, num=k, lds_slots=slots)
            _same(got, want, (name, dtype, c, slots))
            again = M.measure_objects(vol_d, img_d, num=k, lds_slots=slots)
            assert all(torch.equal(a, b) for a, b in zip(_fields(got).values(), _fields(again).values())), (name, dtype, c, slots, "two runs differ")
    # host inputs sent to the device, num left to volume.max(), the default lds_slots
    _same(M.measure_objects(vol, None, device=DEV), M.measure_objects(vol), (name, "host input"))


@pytest.mark.parametrize("name", NAMES)
def test_contacts_equal_the_numpy_route_and_tie_to_the_contact_faces(name):
    from ullsam_amd.utils import measure3d as M
    vol, k = _get(name)
    want = M.object_contacts(vol, num=k)
    got = M.object_contacts(T(vol), num=k)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want)
    assert torch.equal(got, M.object_contacts(T(vol), num=k)) and torch.equal(M.object_contacts(vol, device=DEV).cpu(), M.object_contacts(vol))
    surf = M.measure_objects(T(vol), num=k).surface                                  # the invariant on the DEVICE outputs
    c = torch.zeros((k + 1, 3), dtype=torch.int64, device=DEV)
    c.index_add_(0, got[:, 0], got[:, 2:])
    c.index_add_(0, got[:, 1], got[:, 2:])
    assert torch.equal(surf[:, 4:7], c[1:]) and bool((surf[:, 1:4] >= surf[:, 4:7]).all())
    if name == "tiles along y and z":
        assert len(want) > 20


def test_every_voxel_its_own_id():
    """K = 4096 on 16 x 16 x 16: far more labels per workgroup than LDS slots -- the table and the direct route act within one launch --, the largest
    number of contact pairs per voxel, and max_pairs one below the true count."""
    from ullsam_amd import _lib
    from ullsam_amd.utils import measure3d as M
    vol = (np.arange(4096, dtype=np.int32) + 1).reshape(16, 16, 16)
    img = R.intensity(16, 16, 16, 3, np.uint8)
    want = M.measure_objects(vol, img, num=4096)
    for slots in SLOTS:
        _same(M.measure_objects(T(vol), T(img), num=4096, lds_slots=slots), want, slots)
    npairs = 3 * 16 * 16 * 15
    assert npairs == 11520
    pairs = M.object_contacts(T(vol), num=4096, max_pairs=npairs)
    assert tuple(pairs.shape) == (npairs, 5) and torch.equal(pairs.cpu(), M.object_contacts(vol, num=4096))
    assert bool((pairs[:, 2:].sum(1) == 1).all()) and bool((pairs[:, 2:].max(1).values == 1).all())       # exactly one axis count, equal to 1
    assert pairs[:, 2:].sum(0).tolist() == [16 * 16 * 15] * 3
    with pytest.raises(_lib.UllsamError):
        M.object_contacts(T(vol), num=4096, max_pairs=npairs - 1)
    assert torch.equal(M.object_contacts(T(vol), num=4096), pairs)                   # the next call succeeds


def test_one_label_over_32x512x512_with_saturated_uint16():
    """The whole-segment carry over every row of every tile, and sums beyond 2^32 and beyond float32's integer range, against closed forms."""
    from ullsam_amd.utils import measure3d as M
    Z, H, W = 32, 512, 512
    vol = torch.ones((Z, H, W), dtype=torch.int32, device=DEV)
    img = torch.full((Z, H, W), 65535, dtype=torch.uint16, device=DEV)
    s1 = lambda n: n * (n - 1) // 2
    s2 = lambda n: (n - 1) * n * (2 * n - 1) // 6
    n = Z * H * W
    moments = [Z * H * s1(W), Z * W * s1(H), H * W * s1(Z), Z * H * s2(W), Z * W * s2(H), H * W * s2(Z), Z * s1(W) * s1(H), H * s1(W) * s1(Z), W * s1(H) * s1(Z)]
    for slots in (128, 0):
        t = M.measure_objects(vol, img, num=1, lds_slots=slots)
        assert t.voxels.tolist() == [n] and t.box.tolist() == [[0, 0, 0, W - 1, H - 1, Z - 1]]
        assert t.moments.tolist() == [moments]
        assert t.surface.tolist() == [[n - (Z - 2) * (H - 2) * (W - 2), 2 * H * W, 2 * Z * W, 2 * Z * H, 0, 0, 0]]
        assert t.isum.tolist() == [[n * 65535]] and t.isum2.tolist() == [[n * 65535 ** 2]] and t.imin.tolist() == [[65535]] and t.imax.tolist() == [[65535]]
    assert n * 65535 ** 2 > 2 ** 54 and moments[3] > 2 ** 32 and n * 65535 > 2 ** 32   # (far past int32 and past float32's 2^24)
    assert tuple(M.object_contacts(vol, num=1).shape) == (0, 5)


def test_ids_outside_the_range_raise_and_leave_the_tables_of_the_rest():
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import measure3d as M
    vol, k = _get("tiles along y and z")
    img = R.intensity(vol.shape[0], vol.shape[1], vol.shape[2], 3, np.uint8)
    where = (4, 9, 150)                                                              # the interior
    clean = vol.copy()
    clean[where] = 0                                                                 # a bad id reads as background
    want, want_pairs = M.measure_objects(clean, img, num=k), M.object_contacts(clean, num=k)
    for value in (k + 1, -1):
        bad = vol.copy()
        bad[where] = value
        for slots in SLOTS:
            with pytest.raises(_lib.UllsamError):
                M.measure_objects(T(bad), T(img), num=k, lds_slots=slots)
            t, flags = ops.measure_objects3d(T(bad), k, T(img), slots)
            assert flags.cpu().tolist()[0] == 1
            for n, v in _fields(want).items():
                assert torch.equal(t[n].cpu(), v), (value, slots, n)
        with pytest.raises(_lib.UllsamError):
            M.object_contacts(T(bad), num=k)
        rows, flags = ops.object_contacts3d(T(bad), k, 4096)
        fl = flags.cpu().tolist()
        assert fl[:2] == [1, 0] and fl[2] == fl[3] == len(want_pairs)
        _same(M.measure_objects(T(clean), T(img), num=k), want, value)                # the next call is correct
        assert torch.equal(M.object_contacts(T(clean), num=k).cpu(), want_pairs)


def test_unaligned_views_inside_guarded_buffers():
    """The volume 4 bytes and the uint8 x 3 image one sample off a 16-byte boundary, every output a view inside a guarded buffer: the guards stay
    intact, and the surroundings of the volume are never read as neighbours."""
    from ullsam_amd import ops
    from ullsam_amd.utils import measure3d as M
    vol, k = _get("tiles along y and z")
    img = R.intensity(vol.shape[0], vol.shape[1], vol.shape[2], 3, np.uint8)
    want = _fields(M.measure_objects(vol, img, num=k))
    pad = 64
    vbuf = np.ones((pad + vol.size + pad,), np.int32)                                # (1: an id that would be counted if the volume's surroundings were read)
    vbuf[pad + 1:pad + 1 + vol.size] = vol.reshape(-1)
    vol_d = T(vbuf)[pad + 1:pad + 1 + vol.size].view(vol.shape)
    ibuf = np.full((pad + img.size + pad,), 200, np.uint8)
    ibuf[pad + 1:pad + 1 + img.size] = img.reshape(-1)
    img_d = T(ibuf)[pad + 1:pad + 1 + img.size].view(img.shape)
    assert vol_d.data_ptr() % 16 == 4 and img_d.data_ptr() % 16 == 1
    for slots in (128, 0):
        guard, bufs, out = -123456789, {}, {}
        for n, v in want.items():
            bufs[n] = torch.full((pad + v.numel() + pad,), guard, dtype=v.dtype, device=DEV)
            out[n] = bufs[n][pad + 1:pad + 1 + v.numel()].view(v.shape)
        fbuf = torch.full((pad + ops.MEASURE_FLAGS + pad,), guard, dtype=torch.int32, device=DEV)
        got, flags = ops.measure_objects3d(vol_d, k, img_d, slots, out=out, flags=fbuf[pad:pad + ops.MEASURE_FLAGS])
        assert flags.cpu().tolist()[0] == 0
        for n, v in want.items():
            assert got[n].data_ptr() == out[n].data_ptr() and torch.equal(out[n].cpu(), v), (n, slots)
            assert bool((bufs[n][:pad + 1] == guard).all()) and bool((bufs[n][pad + 1 + v.numel():] == guard).all()), (n, slots)
        assert bool((fbuf[:pad] == guard).all()) and bool((fbuf[pad + ops.MEASURE_FLAGS:] == guard).all())
    assert torch.equal(M.object_contacts(vol_d, num=k).cpu(), M.object_contacts(vol, num=k))


def test_raw_wrappers_flags_row_count_and_unsorted_rows():
    from ullsam_amd import _lib, ops
    from ullsam_amd.utils import measure3d as M
    vol, k = _get("tiles along y and z")
    ref = M.object_contacts(vol, num=k)
    rows, flags = ops.object_contacts3d(T(vol), k, 256)
    fl = flags.cpu().tolist()
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (256, 4) and fl[:2] == [0, 0] and fl[2] == fl[3] == len(ref)
    r = rows[:fl[2]].cpu()
    r = r[torch.argsort(r[:, 0])]
    assert torch.equal(torch.cat([torch.stack([r[:, 0] >> 32, r[:, 0] & 0xffffffff], 1), r[:, 1:]], 1), ref)
    rows, flags = ops.object_contacts3d(T(vol), k, 4)                                # too small a table: refused and counted, nothing written past it
    fl = flags.cpu().tolist()
    assert fl[0] == 0 and (fl[1] == 1 or fl[2] > 4)
    t, flags = ops.measure_objects3d(T(vol), k)
    assert sorted(t) == ["box", "moments", "surface", "voxels"] and flags.dtype == torch.int32 and flags.cpu().tolist()[0] == 0
    t, flags = ops.measure_objects3d(T(vol), 0)                                      # K = 0: empty tables, every id is out of range
    assert t["voxels"].numel() == 0 and flags.cpu().tolist()[0] == 1
    small = T(vol[:2, :3, :5])
    with pytest.raises(_lib.UllsamError):
        ops.measure_objects3d(small, 5, torch.zeros((2, 3, 5), dtype=torch.float32, device=DEV))
    with pytest.raises(_lib.UllsamError):
        ops.measure_objects3d(small, 5, torch.zeros((2, 3, 5, 5), dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.UllsamError):
        ops.measure_objects3d(small, 5, lds_slots=48)
    with pytest.raises(_lib.UllsamError):
        ops.measure_objects3d(torch.zeros((32768, 1, 1), dtype=torch.int32, device=DEV), 0)
    with pytest.raises(_lib.UllsamError):
        ops.object_contacts3d(torch.zeros((1, 1, 32768), dtype=torch.int32, device=DEV), 0)
    with pytest.raises(_lib.UllsamError):
        ops.object_contacts3d(small, 5, max_pairs=0)


def test_generate_stack_label_volume_returns_the_table_of_its_volume():
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import measure3d as M
    from ullsam_amd.utils import synthetic as S
    from tests import util as U
    from tests.test_amg_gpu import _small_sam
    sam, _ = _small_sam()
    S.blob_decoder_init(sam)                                # the structured decoder: a click draws a disc around itself
    kw = dict(points_per_side=6, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05, box_nms_thresh=0.7)
    gen = SamAutomaticMaskGenerator(sam, output_mode="uncompressed_rle", **kw)
    img = np.ascontiguousarray(U.rand_image((3, 104, 104), 23, 255.0).transpose(1, 2, 0).astype(np.uint8))
    images = [np.ascontiguousarray(img[s:s + 96, s:s + 96]) for s in (0, 3, 6)]      # three planes of 96^2, shifted by a few pixels
    volume0, records0, objects0 = gen.generate_stack_label_volume(images, min_visible_area=3)
    out = gen.generate_stack_label_volume(images, min_visible_area=3, measure=True)
    assert len(out) == 4
    volume, records, objects, table = out
    assert torch.equal(volume, volume0) and records == records0 and int(volume.max()) >= 2
    assert sorted(objects) == sorted(objects0) and all(torch.equal(objects[n], objects0[n]) for n in objects)
    _same(table, M.measure_objects(volume.cpu(), np.stack(images)), "stack")
    assert torch.equal(table.voxels, objects["voxels"]) and torch.equal(table.box[:, [0, 1, 3, 4]], objects["boxes"]) and torch.equal(table.box[:, [2, 5]], objects["zrange"])
    with pytest.raises(ValueError):
        gen.generate_stack_label_volume([im.astype(np.float32) for im in images], measure=True)
