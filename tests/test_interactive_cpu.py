"""The interactive loop's host side (no GPU): utils.interactive.click_finish_host against the plain-loop definitions of tests/interactive_ref.py,
against Pillow's own NEAREST resize and against the app's overlay expression on whole arrays; the palette, the blend tables, the click
mapping; and the C ABI's new export."""
import colorsys
import os
import re

import numpy as np
import pytest

from tests import interactive_ref as R
from ullsam_amd.utils import interactive as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(shape):
    n, S, hw, side, top, left = R.SHAPES[shape]
    image, canvas = R.display_inputs(hw)
    return n, S, hw, side, top, left, image, canvas


def _host(low, S, hw, side, top, left, thr, image, canvas, first_id, paint, highlight, palette):
    lut_inst, lut_cur = I.blend_luts(palette)
    ids = canvas.copy()
    mask, overlay, stats = I.click_finish_host(low, S, hw, side, top, left, thr, image=image, canvas=ids, first_id=first_id, paint=paint,
                                               highlight=highlight, lut_inst=lut_inst, lut_cur=lut_cur, want_overlay=True)
    return mask, ids, overlay, stats


def _same(got, ref, what):
    for name, g, r in zip(("mask", "canvas", "overlay", "stats"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, r.dtype, g.shape, r.shape)
        assert np.array_equal(g, r), (what, name, int((g != r).sum()))


@pytest.mark.parametrize("shape", R.SMALL)
def test_host_form_equals_the_scalar_loops(shape):
    """Every pixel by scalar arithmetic (the definition as written), the row form of the same definition, and the host form: equal bits."""
    n, S, hw, side, top, left, image, canvas = _case(shape)
    args = (R.lows(n)["p3"], S, hw, side, top, left, 0.0, image, canvas, 50, True, True, R.TEST_PALETTE)
    ref = R.click_finish_loops(*args)
    _same(R.click_finish_rows(*args), ref, shape + " rows")
    _same(_host(*args), ref, shape + " host")


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_host_form_equals_the_definition_on_every_shape(shape):
    """The row form of the definition on every shape: every input set under every flag combination on the small shapes; on the two 1024-sized
    ones (a second and a half per run of the row loops) each input set once, the flag combinations spread over them."""
    n, S, hw, side, top, left, image, canvas = _case(shape)
    runs = [(name, fl) for name in ("p1", "p3", "p3_full_empty") for fl in R.FLAGS] if shape in R.SMALL else \
        [("p3", (True, True)), ("p3_full_empty", (True, False)), ("p1", (False, True))]
    low = R.lows(n)
    for name, (paint, highlight) in runs:
        args = (low[name], S, hw, side, top, left, 0.0, image, canvas, 50, paint, highlight, R.TEST_PALETTE)
        got, ref = _host(*args), R.click_finish_rows(*args)
        _same(got, ref, f"{shape} {name} paint={paint} highlight={highlight}")
        if not paint:
            assert np.array_equal(got[1], canvas)
    # another threshold moves the mask (the comparison is v > thr, not v > 0)
    args = (low["p1"], S, hw, side, top, left, 0.75, None, canvas, 1, False, False, R.TEST_PALETTE)
    got = I.click_finish_host(low["p1"], S, hw, side, top, left, 0.75)
    ref = R.click_finish_rows(*args)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[3]) and got[1] is None
    if shape != "degenerate":
        assert got[0].sum() < I.click_finish_host(low["p1"], S, hw, side, top, left, 0.0)[0].sum()


def test_masks_hold_the_special_values():
    """The inputs really contain what the cases are for: an empty and a full mask, and logits of exactly 0.0 (out) and +-1e-30 (in / out)."""
    n, S, hw, side, top, left, image, canvas = _case("identity")
    low = R.lows(n)
    m, _, st = I.click_finish_host(low["p3_full_empty"], S, hw, side, top, left)
    assert m[0].all() and not m[1].any() and 0 < m[2].sum() < m[2].size
    assert st[0].tolist() == [hw[0] * hw[1], 0, 0, hw[1] - 1, hw[0] - 1] and st[1].tolist() == [0, 0, 0, 0, 0]
    b = low["p3"][1]
    assert (b == 0).sum() > n and (b == np.float32(1e-30)).any() and (b == np.float32(-1e-30)).any()
    m, _, _ = I.click_finish_host(low["p3"], S, hw, side, top, left)
    assert not m[1][0].any() and m[1][-1, 0] == 1 and m[1][-1, -1] == 0          # rows of 0.0, the +tiny corner, the -tiny corner


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_mask_equals_pillow_nearest_of_the_frame_mask(shape):
    """postprocess_mask / export_mask (app.py:283-287, 807-820) by Pillow itself: the thresholded S x S frame mask resized to the padded square with
    Image.NEAREST, cut to the window.  Pillow has two NEAREST paths.  16-bit images (export_mask's own dtype, app.py:814) take source indices in
    doubles: that is the integer rule, and the masks are equal everywhere.  8-bit images step through the source in 16.16 fixed point, which
    falls one source pixel short where (d + 0.5) * n_in / n_out is an integer and the ratio has no exact 16.16 form (Pillow 12.2.0: display
    index 3 of 32 -> 7 reads source 15, not 16; index 666 of 1024 -> 1333 reads 511, not 512): the 8-bit result is held equal everywhere else."""
    Image = pytest.importorskip("PIL.Image")
    n, S, hw, side, top, left, _, _ = _case(shape)
    low = R.lows(n)["p3"]
    frame_mask, _, _ = I.click_finish_host(low, S, (S, S), S, 0, 0)            # side == S: the frame pixel is the display pixel
    got, _, _ = I.click_finish_host(low, S, hw, side, top, left)
    d = np.arange(side)
    tie = ((2 * d + 1) * S) % (2 * side) == 0                                   # (d + 0.5) * S / side is an integer
    ty, tx = tie[top:top + hw[0]], tie[left:left + hw[1]]
    for p in range(low.shape[0]):
        m = frame_mask[p].astype(np.uint16)
        pil = np.array(Image.fromarray(m * 255).resize((side, side), Image.NEAREST))
        assert np.array_equal(got[p], (pil[top:top + hw[0], left:left + hw[1]] > 0).astype(np.uint8)), (shape, p)
        pil8 = np.array(Image.fromarray(frame_mask[p] * 255).resize((side, side), Image.NEAREST))
        cut = (pil8[top:top + hw[0], left:left + hw[1]] > 0).astype(np.uint8)
        assert np.array_equal(got[p][~ty][:, ~tx], cut[~ty][:, ~tx]), (shape, p)


@pytest.mark.parametrize("shape", ["up_beyond_frame", "off_size"])
def test_overlay_equals_the_apps_expression_on_whole_arrays(shape):
    """visualize_masks (app.py:748-772) as the app runs it -- a loop over instance ids on whole arrays, then the current mask -- with the app's palette."""
    n, S, hw, side, top, left, image, canvas = _case(shape)
    low = R.lows(n)["p3"]
    colors = [tuple(int(c) for c in row) for row in I.default_palette()]
    assert len(colors) == 64
    for paint, highlight in R.FLAGS:
        mask, final_mask, got, _ = _host(low, S, hw, side, top, left, 0.0, image, canvas, 90, paint, highlight, None)
        overlay = image.copy()
        for instance_id in range(1, np.max(final_mask) + 1):
            instance_mask = (final_mask == instance_id)
            if np.any(instance_mask):
                color = colors[(instance_id - 1) % len(colors)]
                alpha = 0.5
                overlay[instance_mask] = ((1 - alpha) * overlay[instance_mask] + alpha * np.array(color)).astype(np.uint8)
        current_mask = mask[-1].astype(bool) if highlight else None
        if current_mask is not None and np.any(current_mask):
            alpha = 0.7
            overlay[current_mask] = ((1 - alpha) * overlay[current_mask] + alpha * np.array((0, 255, 0))).astype(np.uint8)
        assert np.array_equal(got, overlay), (shape, paint, highlight)


def test_default_palette_is_the_apps():
    pal = I.default_palette()
    assert pal.dtype == np.uint8 and pal.shape == (64, 3)
    for i in range(64):
        r, g, b = colorsys.hsv_to_rgb(i / 64, 0.8, 0.9)                             # app.py:84-95
        assert tuple(pal[i]) == (int(r * 255), int(g * 255), int(b * 255))
    assert len({tuple(c) for c in pal}) == 64


@pytest.mark.parametrize("palette", [None, R.TEST_PALETTE])
def test_blend_luts_equal_the_expression_for_all_byte_values(palette):
    lut_inst, lut_cur = I.blend_luts(palette)
    pal = I.default_palette() if palette is None else palette
    assert lut_inst.dtype == np.uint8 and lut_inst.shape == (len(pal), 3, 256) and lut_cur.dtype == np.uint8 and lut_cur.shape == (3, 256)
    for v in range(256):
        px = np.array([v, v, v], np.uint8)
        for i in range(len(pal)):
            assert np.array_equal(lut_inst[i, :, v], R.blend(px, tuple(int(c) for c in pal[i]), 0.5))
        assert np.array_equal(lut_cur[:, v], R.blend(px, (0, 255, 0), 0.7))
    with pytest.raises(ValueError):
        I.blend_luts(np.zeros((0, 3), np.uint8))


def test_click_coordinates_follow_the_app():
    """app.py:536-537: int(x * img_size / width); with the centred pad, the padded square's coordinate takes x's place."""
    S = 1024
    for size in (1024, 512, 1333, 61):                                             # square images: the app's own case
        pts = [[0, 0], [size - 1, size - 1], [size // 3, size // 2], [size - 1, 0]]
        got = I.frame_coords(pts, S, size)
        assert got.dtype == np.float32 and got.shape == (4, 2)
        for (x, y), g in zip(pts, got):
            assert g.tolist() == [int(x * S / size), int(y * S / size)]
    assert I.frame_coords([[1332, 1332]], S, 1333).tolist() == [[1023.0, 1023.0]]   # the last pixel stays inside the frame
    H, W = 1000, 1333                                                              # landscape: rows are padded
    top = (1333 - H) // 2
    got = I.frame_coords(np.array([[[0, 0], [W - 1, H - 1]]]), S, 1333, top, 0)
    assert got.shape == (1, 2, 2)
    assert got[0].tolist() == [[0.0, float(int(top * S / 1333))], [float(int((W - 1) * S / 1333)), float(int((H - 1 + top) * S / 1333))]]
    got = I.frame_coords([[46, 60]], 64, 61, 0, 7)                                 # portrait: columns are padded; the last pixel
    assert got.tolist() == [[float(int(53 * 64 / 61)), float(int(60 * 64 / 61))]]
    assert I.frame_coords([[10.5, 20.25]], S, 2048).tolist() == [[5.0, 10.0]]      # truncation, not rounding


def test_host_form_checks_its_arguments():
    low = np.zeros((1, 4, 4), np.float32)
    with pytest.raises(ValueError):
        I.click_finish_host(low, 16, (8, 8), 8, 1, 0)                              # the window leaves the square
    with pytest.raises(ValueError):
        I.click_finish_host(low, 16, (8, 8), paint=True)                           # no canvas to paint
    with pytest.raises(ValueError):
        I.click_finish_host(low, 16, (8, 8), want_overlay=True)                    # no image to blend
    with pytest.raises(ValueError):
        I.click_finish_host(low[0], 16, (8, 8))


def test_abi_declares_and_binds_click_finish():
    from ullsam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1)) == 14 == _lib.ABI_VERSION      # an added export leaves it alone
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+ullsam_click_finish\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "include/ullsam_hip.h must declare ullsam_click_finish"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args == len(_lib.SIGNATURES["ullsam_click_finish"]) == 23
    assert re.search(r"ullsam_click_finish[^;]*;\s*/\*[^*]*app\.py:\d+", hdr), "the declaration cites the app.py lines it replaces"
    from ullsam_amd import ops
    assert callable(ops.click_finish)
