"""The mask-generation kernels of csrc/amg.hip against the exact definitions of tests/amg_ref.py, at their edges: the fused post-processing launch
(ullsam_amg_postprocess) per geometry and threshold pair, its `index` argument, its footprint shortcut and its entry checks; the stability counts, the
box and RLE helpers per byte position and across emission trips, and the whole NMS suppression matrix.  Every comparison is exact: post32 restates the
kernel's float32 arithmetic operation by operation, the rest is integer work.  tests/test_amg_ref_cpu.py holds the references against each other."""
import numpy as np
import pytest
import torch

from oracle import amg_oracle as AO
from tests import amg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                                        # elements of 0xA5 bytes after every output buffer


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _filled(n, dtype):
    """n elements of dtype plus GUARD more, every byte 0xA5."""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full(((n + GUARD) * size,), 0xA5, dtype=torch.uint8, device=DEV).view(dtype)


def _untouched(t, start=0):
    return bool((t[start:].contiguous().view(torch.uint8) == 0xA5).all().item())


def _post_direct(low, index, M, geom, thr, off, boxes_shift=0, alloc_frame=None):
    """ullsam_amg_postprocess by direct call into pre-filled, guarded buffers -> dict of host arrays + `guards_ok`.  alloc_frame: size the words for
    that frame instead of the geometry's (calls that must be rejected on their sizes alone).  A raising call leaves `_post_direct.untouched_after_error`."""
    from ullsam_amd import _lib
    from ullsam_amd.ops import _stream
    (LH, LW), S1, (nh, nw), (x0, y0, x1, y1), (FH, FW) = geom
    aFH, aFW = (FH, FW) if alloc_frame is None else alloc_frame
    nyb = (aFH + 63) // 64
    nwords = M * nyb * aFW
    words, counts, first = _filled(nwords, torch.int64), _filled(M, torch.int32), _filled(M, torch.uint8)
    boxes, stab = _filled(4 * M + 4, torch.int32), _filled(2 * M, torch.int32)
    idx = None if index is None else T(np.asarray(index, np.int32))
    bufs = dict(words=(words, nwords), rle_counts=(counts, M), first=(first, M), boxes=(boxes[boxes_shift:], 4 * M), stab=(stab, 2 * M))
    try:
        _lib.call("ullsam_amg_postprocess", low.data_ptr(), None if idx is None else idx.data_ptr(), M, LH, LW, S1, nh, nw, y1 - y0, x1 - x0, FH, FW,
                  x0, y0, float(thr), float(off), words.data_ptr(), counts.data_ptr(), first.data_ptr(), boxes[boxes_shift:].data_ptr(), stab.data_ptr(),
                  _stream())
    except _lib.UllsamError:
        torch.cuda.synchronize()
        _post_direct.untouched_after_error = all(_untouched(t) for t in (words, counts, first, boxes, stab))
        raise
    torch.cuda.synchronize()
    out = {k: t[:n].cpu().numpy() for k, (t, n) in bufs.items()}
    out["guards_ok"] = all(_untouched(t, n) for t, n in bufs.values())
    out["all_untouched"] = all(_untouched(t) for t, _ in bufs.values())
    out["words"] = out["words"].view(np.uint64).reshape(M, nyb, aFW)
    out["boxes"] = out["boxes"].reshape(M, 4).astype(np.int64)
    out["stab"] = out["stab"].reshape(M, 2).astype(np.int64)
    out["rle_counts"] = out["rle_counts"].astype(np.int64)
    return out


def _same(got, e, sel=None, what=""):
    """Every output of the fused launch equals `expected` (of the planes `sel`), exactly."""
    sel = np.arange(len(e["first"])) if sel is None else np.asarray(sel)
    assert got["guards_ok"], f"{what}: a store past the end of an output"
    for k in ("stab", "boxes", "first", "rle_counts"):
        bad = np.nonzero((got[k] != e[k][sel]).reshape(len(sel), -1).any(-1))[0]
        assert bad.size == 0, f"{what}: {k} differs on planes {bad.tolist()}: got {got[k][bad[:4]].tolist()}, expected {e[k][sel][bad[:4]].tolist()}"
    diff = got["words"] != e["words"][sel]
    assert not diff.any(), f"{what}: {int(diff.sum())} change words differ, first at (plane, row block, x) = {np.argwhere(diff)[0].tolist()}"


CASES = [(g, p) for g in R.GEOMS for p in R.PAIRS + (R.FIX_PAIR,)]


@pytest.mark.parametrize("name,pair", CASES, ids=[f"{g}-{p[0]}-{p[1]}" for g, p in CASES])
def test_fused_postprocess_is_exact_per_geometry_and_threshold_pair(name, pair):
    """amg_postprocess_kernel<1> / <4> against post32 + the integer oracle: boxes, both stability counts, the score, first, the change counts, the RLEs
    (all, and a permuted selection with a repeat) and the change words themselves, written into a 0xA5-filled, guarded buffer.  The geometries reach
    ragged column blocks and short last row blocks, idle waves of a second workgroup, crops that start mid-block / on a block boundary / flush with the
    frame's end, the column-end branch (post_eval of the next column's top) with r = 64 and on every element, memo rows skipped (stage 2 down by > 3) and
    reused (stage 1 down), CH = CW = 1, FW = 1 and three emission trips; the planes reach NaN / inf cells (`bad` in the footprint test), constants on
    the thresholds, and the pairs reach hi == lo and hi < lo (max / min of the three in the footprint test).  (-1.0, 0.6) is the pair whose float and
    double sums differ: with hi built from two floats the planes planted at either candidate value count differently."""
    from ullsam_amd.utils import amg as A
    geom = R.GEOMS[name]
    thr, off = pair
    low_h = R.fix_pair_planes(name) if pair == R.FIX_PAIR else R.planes(name, thr, off)
    M = low_h.shape[0]
    e = R.expected(low_h, geom, thr, off)
    low = T(low_h)
    _, S1, inp, crop, orig = geom
    # ---- the public entry
    words, sc, frame = A.postprocess_low_res(low, S1, inp, list(crop), orig, thr, off, defer=True)
    h = sc.cpu().numpy()
    stab = h[6:8].reshape(-1)[:2 * M].reshape(M, 2).astype(np.int64)
    print(f"{name} {pair}: stability counts differ on {int((stab != e['stab']).any(-1).sum())} planes of {M}, by {np.abs(stab - e['stab']).sum(0).tolist()} pixels")
    assert np.array_equal(stab, e["stab"]), (stab.tolist(), e["stab"].tolist())
    pp = A.PostprocessedMasks(words, sc, frame)
    assert np.array_equal(pp.boxes, e["boxes"])
    assert np.array_equal(pp.stability_score, e["score"], equal_nan=True)
    assert np.array_equal(pp.first, e["first"]) and np.array_equal(pp.rle_counts, e["rle_counts"])
    rles = pp.rles(np.arange(M))
    assert rles == e["rles"]
    sel = [M - 1, 3, 3, 0, 7]
    assert pp.rles(sel) == [e["rles"][i] for i in sel]
    assert np.array_equal(words.cpu().numpy().view(np.uint64), e["words"])
    # ---- the same launch into guarded buffers: every word of the frame written, nothing after it
    _same(_post_direct(low, None, M, geom, thr, off), e, what=f"{name} {pair}")
    # ---- the meaning: outside the kernel's own margin the decoded masks are float64 F.interpolate twice, thresholded
    (x0, y0, x1, y1), (FH, FW) = crop, orig
    v64 = R.post64(low_h[:R.N_SMOOTH], S1, inp, (y1 - y0, x1 - x0))
    share, outside = R.band_share(v64, R.band_of(low_h[:R.N_SMOOTH]), thr, off)
    assert share < 0.01 or v64.size < 1000
    for i in range(R.N_SMOOTH):
        m = R.runs_to_mask(rles[i]["counts"], FH, FW)
        assert np.array_equal(m[y0:y1, x0:x1][outside[i]], (v64[i] > float(np.float32(thr)))[outside[i]])
        assert m.sum() == m[y0:y1, x0:x1].sum()


@pytest.mark.parametrize("name", ["inside", "full_nc1"])
def test_fused_postprocess_index_selects_the_planes(name):
    """`index != NULL` (lowp = low + index[n] * LH * LW; no Python caller passes it): output i is `expected` of plane index[i], with a repeat and out of order."""
    geom = R.GEOMS[name]
    low_h = R.planes(name, 0.0, 1.0)
    e = R.expected(low_h, geom, 0.0, 1.0)
    index = [11, 0, 0, 5, 3]
    _same(_post_direct(T(low_h), index, len(index), geom, 0.0, 1.0), e, sel=index, what=name)


@pytest.mark.parametrize("kind", ["spikes_down", "spikes_up", "tall_spikes_down", "tall_spikes_up", "hi_spikes", "lo_spikes", "straddle"])
@pytest.mark.parametrize("pair", [(0.0, 1.0), (0.25, 0.5)], ids=str)
@pytest.mark.parametrize("name", ["inside", "full_nc4", "row_after"])
def test_fused_postprocess_footprint_shortcut(name, pair, kind):
    """The footprint test of amg_postprocess_kernel (`decided`: a 64-row block whose low-res footprint clears every threshold by the margin is written
    without evaluating a pixel).  spikes: one plane per low-res cell, constant +-5 with that cell at -+5 -- a footprint one cell too small decides a
    block the spike reaches; tall spikes: the same with the cell at -+1e6, because a +-5 spike enters a block's first or last row (and the row after the
    block, which the change word's top bit needs) with a weight too small to cross a threshold, so a footprint short by that one row would pass: a
    spike of 1e6 crosses at a weight of 1e-5, and inside the footprint it raises the margin so that the block is evaluated (`row_after` is the geometry
    where the row after a block reaches a low-res row that no row of the block does: on the other two a footprint without that row is the same footprint);
    hi / lo spikes: planes just above one threshold with one cell just below it, so only that count may change (max / min over
    hi, lo, thr); straddle: constants half a margin and two margins outside the thresholds, on both sides of the decision."""
    geom = R.GEOMS[name]
    (lh, lw), (x0, y0, x1, y1) = geom[0], geom[3]
    thr, off = pair
    t, hi, lo = (float(x) for x in R.thresholds(thr, off))
    npix = (y1 - y0) * (x1 - x0)
    if kind == "spikes_down":
        low_h = R.spike_planes(lh, lw, 5, -5)
    elif kind == "spikes_up":
        low_h = R.spike_planes(lh, lw, -5, 5)
    elif kind == "tall_spikes_down":
        low_h = R.spike_planes(lh, lw, 5, -1e6)
    elif kind == "tall_spikes_up":
        low_h = R.spike_planes(lh, lw, -5, 1e6)
    elif kind == "hi_spikes":
        low_h = R.spike_planes(lh, lw, hi + 0.01, hi - 0.01, cells=range(0, lh * lw, 5))
    elif kind == "lo_spikes":
        low_h = R.spike_planes(lh, lw, lo + 0.01, lo - 0.01, cells=range(0, lh * lw, 5))
    else:
        low_h = R.straddle_planes(lh, lw, thr, off)
    e = R.expected(low_h, geom, thr, off)
    if kind == "hi_spikes":                                        # what the inputs are for, from the reference alone
        assert (e["stab"][:, 1] == npix).all() and (e["mask"].sum((-1, -2)) == npix).all() and (e["stab"][:, 0] < npix).sum() > len(low_h) // 2
    if kind == "lo_spikes":
        assert (e["stab"][:, 0] == 0).all() and not e["mask"].any() and ((e["stab"][:, 1] < npix).sum() > len(low_h) // 2)
    if "spikes_" in kind and kind[0] in "st":
        assert ((e["stab"][:, 0] > 0) & (e["stab"][:, 1] < npix)).sum() > len(low_h) // 2
    if kind == "straddle":
        assert e["stab"].tolist() == [[npix, npix], [npix, npix], [0, 0], [0, 0]]
    _same(_post_direct(T(low_h), None, low_h.shape[0], geom, thr, off), e, what=f"{name} {pair} {kind}")


def test_fused_postprocess_entry_rejections():
    """The checks of ullsam_amg_postprocess: nh > S1, a crop past the frame, boxes off 16 bytes and FH * FW >= 2^31 raise before anything is launched or
    cleared (pre-filled outputs untouched); M = 0 returns 0 and writes nothing."""
    from ullsam_amd import _lib
    low = T(R.planes("one_pixel_crop", 0.0, 1.0))
    g = R.GEOMS["one_pixel_crop"]
    bad = {
        "nh > S1": (g[0], 64, (65, 64), g[3], g[4]),
        "nw > S1": (g[0], 64, (64, 65), g[3], g[4]),
        "crop past the right edge": (g[0], 64, g[2], (5, 3, 10, 4), (7, 9)),
        "crop past the bottom": (g[0], 64, g[2], (5, 3, 6, 8), (7, 9)),
        "frame of 2^31 elements": (g[0], 64, g[2], (0, 0, 1, 1), (65536, 32768)),
    }
    for what, geom in bad.items():
        _post_direct.untouched_after_error = False
        with pytest.raises(_lib.UllsamError):
            _post_direct(low, None, 2, geom, 0.0, 1.0, alloc_frame=(1, 1))
        assert _post_direct.untouched_after_error, what
    _post_direct.untouched_after_error = False
    with pytest.raises(_lib.UllsamError):
        _post_direct(low, None, 2, g, 0.0, 1.0, boxes_shift=1)
    assert _post_direct.untouched_after_error
    assert _post_direct(low, None, 0, g, 0.0, 1.0)["all_untouched"]
    ok = _post_direct(low, None, 2, g, 0.0, 1.0)                   # and the same call with nothing wrong goes through
    assert ok["guards_ok"] and not ok["all_untouched"]


# ---- the helpers --------------------------------------------------------------------------------------------------------------------------
def _stability_direct(x, thr, off):
    from ullsam_amd import _lib
    from ullsam_amd.ops import _stream
    n, per = x.shape
    counts, score = _filled(2 * n, torch.int32), _filled(n, torch.float32)
    _lib.call("ullsam_stability_score", x.data_ptr(), n, per, float(thr), float(off), counts.data_ptr(), score.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _untouched(counts, 2 * n) and _untouched(score, n)
    return counts[:2 * n].cpu().numpy().reshape(n, 2).astype(np.int64), score[:n].cpu().numpy()


@pytest.mark.parametrize("pair", R.PAIRS + (R.FIX_PAIR,), ids=str)
@pytest.mark.parametrize("per", [4, 4 * 16385, 90000])
def test_stability_score_counts_are_exact(per, pair):
    """stability_count_kernel / stability_finish_kernel: a plane of one float4, one float4 past a full sweep of the 64 x 256-thread grid (the grid-stride
    loop's second trip), and a ragged number of sweeps; values ON hi and lo and one ulp either side, NaN, +-inf, +-0; a plane below every threshold
    (0 / 0: NaN); hi == lo and hi < lo; and (-1.0, 0.6), where hi must be float32 of the DOUBLE sum.  Counts and score against the oracle, exactly."""
    thr, off = pair
    x = R.stability_values(3, per, thr, off)
    t, hi, lo = R.thresholds(thr, off)
    ref_counts = np.stack([(x > hi).sum(-1), (x > lo).sum(-1)], -1)
    counts, score = _stability_direct(T(x), thr, off)
    print(f"per {per} {pair}: counts differ by {np.abs(counts - ref_counts).sum(0).tolist()}")
    assert np.array_equal(counts, ref_counts), (counts.tolist(), ref_counts.tolist())
    ref = AO.calculate_stability_score(x.reshape(3, 1, per), thr, off)
    assert np.isnan(ref[2]) and np.array_equal(score, ref, equal_nan=True)
    from ullsam_amd.utils import amg as A
    assert np.array_equal(A.calculate_stability_score(T(x).reshape(3, 4, per // 4), thr, off).cpu().numpy(), ref, equal_nan=True)


def test_stability_score_entry_rejections():
    """ullsam_stability_score reads float4s: per % 4 != 0 and a base pointer off 16 bytes raise."""
    from ullsam_amd import _lib
    buf = T(np.zeros(64, np.float32))
    with pytest.raises(_lib.UllsamError):
        _stability_direct(buf[:12].view(2, 6), 0.0, 1.0)
    with pytest.raises(_lib.UllsamError):
        _stability_direct(buf[1:17].view(2, 8), 0.0, 1.0)
    _stability_direct(buf[4:20].view(2, 8), 0.0, 1.0)


def _byte_masks():
    """(2, 32) masks with a single byte of value 1, 128 or 255 at each of the 64 positions: every byte of every 16-byte chunk, each bit pattern the
    chunk's `any bit -> bit 0` fold has to catch."""
    m = np.zeros((3 * 64, 64), np.uint8)
    for k, val in enumerate((1, 128, 255)):
        m[np.arange(64) + 64 * k, np.arange(64)] = val
    return m.reshape(-1, 2, 32)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned_vector_path", "one_byte_off_scalar_path"])
def test_box_and_rle_per_byte_position(shift):
    """mask_to_box_kernel<16> (ctz / clz over the four words of a chunk) and rle_pack_kernel<16> (byte fold, the column-end word of row 0) with a 16-byte
    aligned base; the same masks one byte off, where W % 16 == 0 must still take mask_to_box_kernel<1> / rle_pack_kernel<1>."""
    from ullsam_amd.utils import amg as A
    m = _byte_masks()
    buf = torch.zeros((m.size + 32,), dtype=torch.uint8, device=DEV)
    view = buf[shift:shift + m.size].view(m.shape)
    view.copy_(T(m))
    assert view.data_ptr() % 16 == shift and view.is_contiguous()
    assert np.array_equal(A.batched_mask_to_box(view).cpu().numpy(), AO.batched_mask_to_box(m))
    got = A.mask_to_rle_pytorch(view)
    assert got == AO.mask_to_rle(m != 0)
    assert np.array_equal(view.cpu().numpy(), m)


@pytest.mark.parametrize("shape", [(129, 1400), (200, 2100)], ids=["two_trips", "three_trips"])
@pytest.mark.parametrize("density", [0.5, 0.01])
def test_rle_emission_across_trips(shape, density):
    """rle_emit_kernel's trip loop (4096 words per trip: `base` carried from trip to trip, the parity of the shared sums): 4200 and 8400 words per mask,
    runs that cross the trip boundaries; rle_pack_kernel<1> (W % 16 != 0 on both) with a ragged last 64-column block and a short last row block.  The change
    words themselves against change_words, then the emitted RLEs (all, and a selection with a repeat) and the boxes against the oracle."""
    from ullsam_amd import _lib
    from ullsam_amd.ops import _stream
    from ullsam_amd.utils import amg as A
    H, W = shape
    rng = np.random.default_rng(H + int(density * 100))
    m = rng.random((3, H, W)) < density
    m[0, -1, -1] = True
    m[1, :, W // 2 - 3:W // 2 + 3] = True                         # six full columns: one run of 6 * H elements, many words without a change
    nyb = (H + 63) // 64
    assert (nyb * W > 4096) and (nyb * W > 8192) == (shape == (200, 2100))
    d = T(m)
    words, counts, first = _filled(3 * nyb * W, torch.int64), _filled(3, torch.int32), _filled(3, torch.uint8)
    _lib.call("ullsam_rle_pack", d.data_ptr(), 3, H, W, words.data_ptr(), counts.data_ptr(), first.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _untouched(words, 3 * nyb * W) and _untouched(counts, 3) and _untouched(first, 3)
    ref_words = R.change_words(m)
    assert np.array_equal(words[:3 * nyb * W].cpu().numpy().view(np.uint64).reshape(3, nyb, W), ref_words)
    ref = AO.mask_to_rle(m)
    assert counts[:3].cpu().numpy().tolist() == [len(R.words_to_positions(w, H)) for w in ref_words]
    assert first[:3].cpu().numpy().tolist() == m[:, 0, 0].astype(int).tolist()
    assert A.mask_to_rle_pytorch(d) == ref
    got = A._rles_from_words(words[:3 * nyb * W].view(3, nyb, W), [2, 0, 2], counts[:3].cpu().numpy()[[2, 0, 2]], first[:3].cpu().numpy()[[2, 0, 2]], H, W)
    assert got == [ref[2], ref[0], ref[2]]
    assert np.array_equal(A.batched_mask_to_box(d).cpu().numpy(), AO.batched_mask_to_box(m))


def _nms_direct(boxes, thr):
    from ullsam_amd import _lib
    from ullsam_amd.ops import _stream
    n = boxes.shape[0]
    nw = (n + 63) // 64
    mask = torch.full((n * nw + GUARD,), -1, dtype=torch.int64, device=DEV)          # ones: a word the launch does not write shows up
    b = T(np.asarray(boxes, np.float32))
    _lib.call("ullsam_nms_mask", b.data_ptr(), n, float(thr), mask.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool((mask[n * nw:] == -1).all().item())
    return mask[:n * nw].cpu().numpy().view(np.uint64).reshape(n, nw)


def _nms_shape_ok(bits, n):
    """Diagonal, lower triangle and the bits >= n are zero."""
    nw = bits.shape[1]
    full = ((bits[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(n, nw * 64)
    return not full[:, n:].any() and not np.tril(full[:, :n]).any()


@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_nms_mask_whole_matrix_is_exact(n):
    """nms_mask_kernel: the whole [N, ceil(N/64)] matrix, not the greedy scan's view of it.  One box, a full block, one box past it, two blocks and a ragged
    third (`ncol`, the skipped blocks below the diagonal, `start` on it); integer boxes with duplicates, nested pairs at IoU exactly 1/2 and 1/4 (`>` not
    `>=`), zero-area boxes and their duplicates (0 / 0), boxes that only touch; on these the float32 quotient equals the integer comparison
    (tests/test_amg_ref_cpu.py), so no band."""
    b = R.nms_int_boxes(n)
    for num, den in R.NMS_THRESHOLDS:
        bits = _nms_direct(b, num / den)
        assert _nms_shape_ok(bits, n)
        ref = R.nms_bits_exact(b, num, den)
        assert np.array_equal(bits, ref), f"n {n} thr {num}/{den}: rows {np.nonzero((bits != ref).any(-1))[0].tolist()[:8]} differ"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_nms_mask_float_boxes_match_the_float32_restatement(n):
    """nms_mask_kernel on the seeded float boxes of test_box_nms_matches_oracle: the whole matrix against nms_bits32, inter / ((ai + aj) - inter) > thr in float32."""
    fb = R.nms_float_boxes(n)
    bits = _nms_direct(fb, 0.7)
    assert _nms_shape_ok(bits, n) and np.array_equal(bits, R.nms_bits32(fb, 0.7))
