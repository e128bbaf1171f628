"""The references of tests/amg_ref.py against each other, on the CPU: post32 (the bits the fused mask post-processing declares) against post64 (float64
F.interpolate twice, the meaning), the change words against the oracle's RLE, and the float32 NMS matrix against the integer one on the boxes the GPU test
uses.  What holds here is what lets tests/test_amg_kernels_gpu.py compare exactly."""
import numpy as np
import pytest

from oracle import amg_oracle as AO
from tests import amg_ref as R


@pytest.mark.parametrize("name", sorted(R.GEOMS))
def test_post32_stays_within_a_tenth_of_the_band_of_post64(name):
    """On the smooth planes the float32 composition is within band / 10 of the float64 one, band = 1e-4 * max(1, max|low|) being the kernel's own footprint
    margin; fewer than 1 % of the pixels lie within the band of a threshold, and outside it the two masks agree at all three thresholds of every pair."""
    geom = R.GEOMS[name]
    low = R.planes(name, 0.0, 1.0)[:R.N_SMOOTH]
    v32 = R.post32(low, geom[1], geom[2], R.crop_hw(geom))
    v64 = R.post64(low, geom[1], geom[2], R.crop_hw(geom))
    band = R.band_of(low)
    gap = float(np.abs(v32.astype(np.float64) - v64).max())
    print(f"{name}: gap {gap:.3e}, band {band:.3e}")
    assert gap <= band / 10
    for thr, off in R.PAIRS + (R.FIX_PAIR,):
        share, outside = R.band_share(v64, band, thr, off)
        for t in R.thresholds(thr, off):
            assert np.array_equal((v32 > t)[outside], (v64 > float(t))[outside])
        if v64.size >= 1000:                                       # (a frame of a few pixels has no share to speak of: one pixel is all of it)
            print(f"{name} {(thr, off)}: band share {share:.5f}")
            assert share < 0.01


def test_post32_of_the_identity_geometry_is_the_input():
    geom = R.GEOMS["identity"]
    low = R.planes("identity", 0.25, 0.5)[:R.N_SMOOTH]
    assert np.array_equal(R.post32(low, geom[1], geom[2], R.crop_hw(geom)).view(np.uint32), low.view(np.uint32))


def test_post32_lets_nan_and_inf_flow_as_ieee_does():
    """A NaN cell poisons exactly the pixels whose taps touch it; an inf cell gives inf where its weight is positive and NaN where it meets weight 0 or -inf."""
    geom = R.GEOMS["full_nc1"]
    low = R.planes("full_nc1", 0.0, 1.0)[-1:]
    v = R.post32(low, geom[1], geom[2], R.crop_hw(geom))
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and np.isfinite(v).mean() > 0.8
    clean = R.post32(np.where(np.isfinite(low), low, 0).astype(np.float32), geom[1], geom[2], R.crop_hw(geom))
    far = np.isfinite(v)                                           # a tap that touches such a cell, even with weight 0, is not finite: the finite pixels never saw it
    assert np.array_equal(v[far], clean[far])


@pytest.mark.parametrize("shape", [(1, 1), (64, 3), (65, 3), (130, 1), (1, 130)])
@pytest.mark.parametrize("last", [False, True])
def test_change_words_round_trip(shape, last):
    """words -> positions -> runs equals the oracle's RLE, with the last element of the flattening set and clear (it has no successor)."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1] + last)
    m = rng.random((4,) + shape) < 0.5
    m[:, -1, -1] = last
    m[1, 0, 0] = True
    m[2, 0, 0] = False
    words = R.change_words(m)
    assert words.shape == (4, (shape[0] + 63) // 64, shape[1]) and words.dtype == np.uint64
    ref = AO.mask_to_rle(m)
    pos = [R.words_to_positions(words[i], shape[0]) for i in range(4)]
    for i in range(4):
        assert pos[i].size == 0 or pos[i].max() < shape[0] * shape[1] - 1
        runs = R.positions_to_runs(pos[i], m[i, 0, 0], *shape)
        assert runs == ref[i]["counts"]
        assert np.array_equal(R.runs_to_mask(runs, *shape), m[i])
    try:
        from ullsam_amd.utils.amg import _rle_records
    except Exception as e:                                         # the module imports the library's binding: without it, only this part is left out
        pytest.skip(f"ullsam_amd.utils.amg cannot be imported here: {e}")
    offs = np.concatenate([[0], np.cumsum([len(p) for p in pos])])
    recs = _rle_records(np.concatenate(pos).astype(np.int64), offs, m[:, 0, 0].astype(np.uint8), shape[0], shape[1])
    assert recs == ref


def test_expected_is_consistent_with_itself():
    """expected(): the RLE, the change words, the counts and the first bits describe one frame mask; the box is the crop's."""
    for name in ("inside", "flush", "row"):
        geom = R.GEOMS[name]
        e = R.expected(R.planes(name, 0.25, 0.5), geom, 0.25, 0.5)
        x0, y0, x1, y1 = geom[3]
        FH, FW = geom[4]
        for i in range(R.M_PLANES):
            pos = R.words_to_positions(e["words"][i], FH)
            assert len(pos) == e["rle_counts"][i]
            assert R.positions_to_runs(pos, e["first"][i], FH, FW) == e["rles"][i]["counts"]
            assert e["mask"][i].sum() == e["mask"][i, y0:y1, x0:x1].sum()
        assert e["stab"][6].tolist() == [0, 0] and e["stab"][7].tolist() == [(y1 - y0) * (x1 - x0)] * 2
        assert e["boxes"][7].tolist() == [0, 0, x1 - x0 - 1, y1 - y0 - 1] and e["boxes"][6].tolist() == [0, 0, 0, 0]


def test_fix_pair_thresholds_differ_between_float_and_double_sums():
    """(-1.0, 0.6): float32(thr + off) of the doubles is -0.40000001, the sum of the two float32 values is -0.39999998; the pairs of PAIRS agree."""
    thr, off = R.FIX_PAIR
    _, hi, lo = R.thresholds(thr, off)
    hi2, lo2 = R.thresholds_two_floats(thr, off)
    assert hi != hi2 and hi2 == np.nextafter(hi, np.float32(0))
    for p in R.PAIRS:
        assert R.thresholds(*p)[1:] == R.thresholds_two_floats(*p)
    low = R.fix_pair_planes("identity")
    e = R.expected(low, R.GEOMS["identity"], thr, off)
    assert e["stab"][R.M_PLANES + 1, 0] == 32 * 32                 # the plane at the two-float hi lies ABOVE the reference's hi ...
    assert e["stab"][R.M_PLANES + 0, 0] == 0                       # ... the plane at the reference's hi does not


@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_nms_float32_matrix_equals_the_integer_one_on_the_integer_boxes(n):
    """Coordinates <= 1024 give areas and unions below 2^22, exact in float32, and a quotient cannot round across a threshold with denominator 2 or 4
    (the nearest other quotient of integers below 2^22 is further than an ulp away): so the GPU test needs no band."""
    b = R.nms_int_boxes(n)
    assert b.min() >= 0 and b.max() <= 1024
    for num, den in R.NMS_THRESHOLDS:
        exact = R.nms_bits_exact(b, num, den)
        assert np.array_equal(R.nms_bits32(b, num / den), exact)
        assert exact.shape == (n, (n + 63) // 64)
    if n >= 64:                                                    # the planted pairs are there and sit where they should relative to each threshold
        half, quarter = R.nms_bits_exact(b, 1, 2), R.nms_bits_exact(b, 1, 4)
        ones = lambda bits: int(np.unpackbits(bits.view(np.uint8)).sum())
        assert ones(quarter) > ones(half) > ones(R.nms_bits_exact(b, 3, 4)) > 0


def test_footprint_rule_is_never_wrong_on_the_single_cell_spikes():
    """The CPU restatement of the kernel's footprint rule, on single-cell spike planes of the GPU test (+-5 and +-1e6): wherever it decides a block
    without evaluating a pixel, post32 agrees on every pixel of the block and on the row after it -- so a failure of the GPU test is the kernel's."""
    for name, ncols, tall in (("inside", 256, 5), ("full_nc4", 256, 5), ("row_after", 64, 5), ("row_after", 64, 1e6), ("inside", 256, 1e6)):
        geom = R.GEOMS[name]
        (lh, lw), S1, inp, (x0, y0, x1, y1), (FH, FW) = geom
        for sign in (1, -1):
            low = R.spike_planes(lh, lw, 5 * sign, -tall * sign, cells=range(0, lh * lw, 7))
            v = R.post32(low, S1, inp, (y1 - y0, x1 - x0))
            decided = 0
            for thr, off in ((0.0, 1.0), (0.25, 0.5)):
                th = R.thresholds(thr, off)
                for p in range(low.shape[0]):
                    for ys in range(0, FH, 64):
                        for bx0 in range(0, FW, ncols):
                            d = R.footprint_decision(low[p], geom, thr, off, ys, bx0, ncols)
                            if not d:
                                continue
                            decided += 1
                            blk = v[p, max(ys - y0, 0):max(min(ys + 65, FH) - y0, 0), max(bx0 - x0, 0):max(bx0 + ncols - x0, 0)]
                            assert all(((blk > t) if d == 1 else ~(blk > t)).all() for t in th)
            assert decided > 0
