"""utils.measure without a GPU: the numpy route against the per-pixel loops and the exact rational definitions of tests/measure_ref.py, the
boundary against scipy's binary erosion, the invariants that tie the tables to the contact list, and the argument checks."""
import numpy as np
import pytest
import torch

from tests import measure_ref as R

IMAGES = ((None, 0), (np.uint8, 1), (np.uint8, 3), (np.uint16, 4), (np.uint16, 0))   # (dtype, C); C = 0: [H, W]


@pytest.fixture(scope="module")
def frames():
    return R.frames()


def _image(lab, dtype, c):
    return None if dtype is None else R.intensity(lab.shape[0], lab.shape[1], c, dtype)


def test_numpy_route_equals_the_loops(frames):
    from ullsam_amd.utils import measure as M
    for name, (lab, k) in frames.items():
        for dtype, c in (IMAGES if lab.size <= 1000 else IMAGES[:1] + IMAGES[3:4]):
            img = _image(lab, dtype, c)
            got = M.measure_instances(lab, img, num=k)
            assert got.area.dtype == torch.int64 and got.box.dtype == torch.int32 and got.moments.dtype == torch.int64 and got.perimeter.dtype == torch.int64
            assert tuple(got.box.shape) == (k, 4) and tuple(got.moments.shape) == (k, 5) and tuple(got.perimeter.shape) == (k, 3)
            if img is None:
                assert got.isum is None and got.isum2 is None and got.imin is None and got.imax is None
            else:
                cc = max(c, 1)
                assert got.isum.dtype == torch.int64 and got.imin.dtype == torch.int32 and tuple(got.isum2.shape) == (k, cc) and tuple(got.imax.shape) == (k, cc)
            assert R.as_lists(got) == R.tables(lab, k, img), (name, dtype, c)
        assert M.label_contacts(lab, num=k).tolist() == [list(r) for r in R.contacts(lab)], name
        # the same through a CPU tensor and with num left to labels.max()
        kmax = max(int(lab.max()), 0)
        assert R.as_lists(M.measure_instances(torch.from_numpy(lab))) == R.tables(lab, kmax), name
    lab, k = frames["discs 150x170"]
    present = int((np.bincount(lab.reshape(-1), minlength=k + 1)[1:] > 0).sum())
    pairs = M.label_contacts(lab, num=k)
    assert present == 36 and len(pairs) == 12 and len(set(pairs[:, :2].reshape(-1).tolist())) == 18      # absent labels and contacts are covered


def test_large_sums_stay_exact_in_the_numpy_route():
    """A weight sum past 2^53 (where np.bincount's float64 accumulation would round): the route splits the weights, the result is the closed form."""
    from ullsam_amd.utils import measure as M
    idx = np.zeros(3, np.int64)
    big = np.array([2 ** 32 - 1, 2 ** 32 - 3, 5], np.int64)
    wide = np.broadcast_to(big, (1 << 20, 3)).reshape(-1)
    got = M._wsum(np.zeros(wide.size, np.int64), wide, 1)
    assert int(got[0]) == (1 << 20) * int(big.sum()) and int(M._wsum(idx, big, 1)[0]) == int(big.sum())
    assert (2 ** 32 - 1) * wide.size >= 2 ** 53                                                         # (the split path was the one taken)
    lab = np.ones((300, 300), np.int32)
    img = np.full((300, 300), 65535, np.uint16)
    t = M.measure_instances(lab, img, num=1)
    assert int(t.isum2[0, 0]) == 90000 * 65535 ** 2 and int(t.isum[0, 0]) == 90000 * 65535
    assert t.moments[0].tolist() == [300 * 44850, 300 * 44850, 300 * 8955050, 300 * 8955050, 44850 * 44850]


def test_boundary_pixels_equal_mask_xor_binary_erosion(frames):
    ndi = pytest.importorskip("scipy.ndimage")
    from ullsam_amd.utils import measure as M
    for name in ("discs 150x170", "5x3", "checkerboard of distinct ids", "one label fills the frame"):
        lab, k = frames[name]
        per = M.measure_instances(lab, num=k).perimeter.numpy()
        for l in range(1, k + 1):
            m = lab == l
            assert per[l - 1, 0] == int((m ^ ndi.binary_erosion(m)).sum()), (name, l)


def test_invariants_between_the_tables_and_the_contact_list(frames):
    from ullsam_amd.utils import measure as M
    for name, (lab, k) in frames.items():
        t = M.measure_instances(lab, num=k)
        pairs = M.label_contacts(lab, num=k).numpy()
        per = t.perimeter.numpy()
        want = np.zeros(k, np.int64)
        np.add.at(want, pairs[:, 0] - 1, pairs[:, 2])
        np.add.at(want, pairs[:, 1] - 1, pairs[:, 2])
        assert np.array_equal(per[:, 2], want), name
        assert (per[:, 1] >= per[:, 2]).all() and (per[:, 1] >= per[:, 0]).all() and (4 * per[:, 0] >= per[:, 1]).all(), name
        assert int(t.area.sum()) == int((lab > 0).sum()), name
        assert (pairs[:, 0] < pairs[:, 1]).all() and (pairs[:, 0] > 0).all() and (pairs[:, 2] > 0).all()
        keys = pairs[:, 0] * (k + 1) + pairs[:, 1]
        assert (np.diff(keys) > 0).all()


def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def test_derive_against_the_rational_definition():
    from ullsam_amd.utils import measure as M
    lab, k = R.ellipse_scene()
    img = R.intensity(lab.shape[0], lab.shape[1], 3, np.uint16, seed=4)
    t = M.measure_instances(lab, img, num=k)
    for ps in (1.0, 0.325):
        d = M.derive(t, pixel_size=ps)
        ref, iref = R.shape_fraction(lab, k), R.intensity_fraction(lab, k, img)
        present = [i for i in range(k) if ref[i] is not None]
        checked = 0
        for i in range(k):
            if ref[i] is None:
                for name, v in d.items():
                    assert np.isnan(v[i]).all(), (i, name)
                continue
            r = ref[i]
            assert _close(d["area"][i], r["area"] * ps * ps, 1e-9)
            for j in range(2):
                assert _close(d["centroid"][i, j], r["centroid"][j] * ps, 1e-9)
            for name in ("equivalent_diameter", "major_axis_length", "minor_axis_length"):
                assert _close(d[name][i], r[name] * ps, 1e-9), (i, name, d[name][i], r[name] * ps)
            assert d["perimeter"][i] == int(t.perimeter[i, 1]) * ps and d["contact_length"][i] == int(t.perimeter[i, 2]) * ps
            for j in range(3):
                assert _close(d["mean"][i, j], iref[i][j][0], 1e-9) and _close(d["std"][i, j], iref[i][j][1], 1e-9)
                assert d["min"][i, j] == int(t.imin[i, j]) and d["max"][i, j] == int(t.imax[i, j])
            if r["l1"] - r["l2"] > 1e-3 * r["l1"]:                                  # sqrt(1 - l2 / l1) and atan2 near (0, 0) are ill-conditioned for near-circles
                checked += 1
                assert abs(d["eccentricity"][i] - r["eccentricity"]) <= 1e-6 and abs(d["orientation"][i] - r["orientation"]) <= 1e-6, i
        assert len(present) == k - 1 and 2 * checked >= len(present) and checked == len(present)
    # a single pixel: l1 == 0, eccentricity 0; an empty table
    one = M.derive(M.measure_instances(np.array([[0, 1]], np.int32), num=1))
    assert one["eccentricity"][0] == 0.0 and one["major_axis_length"][0] == 0.0 and one["centroid"][0].tolist() == [1.0, 0.0] and one["area"][0] == 1.0
    assert all(len(v) == 0 for v in M.derive(M.measure_instances(np.zeros((2, 2), np.int32), num=0)).values())


def test_orientation_sign_convention():
    """A thin bar from the top left to the bottom right (y down): the major axis makes a POSITIVE angle with +x in image coordinates."""
    from ullsam_amd.utils import measure as M
    lab = np.zeros((40, 40), np.int32)
    for i in range(5, 35):
        lab[i, i - 1:i + 2] = 1
    d = M.derive(M.measure_instances(lab, num=1))
    assert abs(d["orientation"][0] - np.pi / 4) < 0.02 and d["eccentricity"][0] > 0.95
    d = M.derive(M.measure_instances(lab[::-1].copy(), num=1))
    assert abs(d["orientation"][0] + np.pi / 4) < 0.02


def test_argument_checks():
    from ullsam_amd import _lib
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils import measure as M
    lab = np.zeros((6, 8), np.int32)
    lab[2:4, 2:5] = 1
    with pytest.raises(_lib.UllsamError):
        M.measure_instances(lab, np.zeros((6, 8), np.float32), num=1)                # float intensity
    with pytest.raises(_lib.UllsamError):
        M.measure_instances(lab, np.zeros((6, 8, 5), np.uint8), num=1)               # C = 5
    with pytest.raises(_lib.UllsamError):
        M.measure_instances(np.zeros((46341, 1), np.int32), num=0)                   # H > 46340
    with pytest.raises(_lib.UllsamError):
        M.label_contacts(np.zeros((1, 46341), np.int32), num=0)
    with pytest.raises(ValueError):
        M.measure_instances(lab, np.zeros((6, 9), np.uint8), num=1)                  # shape mismatch
    with pytest.raises(ValueError):
        M.measure_instances(lab, np.zeros((8, 6, 3), np.uint8), num=1)
    for bad in (2, -7, 2 ** 31 - 1):                                                 # an id outside 0..K, then a good call
        b = lab.copy()
        b[0, 0] = bad
        with pytest.raises(_lib.UllsamError):
            M.measure_instances(b, num=1)
        with pytest.raises(_lib.UllsamError):
            M.label_contacts(b, num=1)
    assert M.measure_instances(lab, num=1).area.tolist() == [6]
    two = np.array([[1, 2, 3]], np.int32)
    with pytest.raises(_lib.UllsamError):
        M.label_contacts(two, num=3, max_pairs=1)                                    # two distinct pairs: refused, not truncated
    assert M.label_contacts(two, num=3, max_pairs=2).tolist() == [[1, 2, 1], [2, 3, 1]]
    gen = object.__new__(SamAutomaticMaskGenerator)                                  # (the check comes before the model is touched)
    img = np.zeros((6, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        gen.generate_label_map(img, out_hw=(12, 16), measure=True)
    with pytest.raises(ValueError):
        gen.generate_label_map(img, window=(0, 0, 3, 3), measure=True)
    with pytest.raises(ValueError):
        gen.generate_label_map(img.astype(np.float32), measure=True)                 # measured against the uint8 image the caller passed
    with pytest.raises(ValueError):
        gen.generate_tiled_label_map(img.astype(np.float32), measure=True)
