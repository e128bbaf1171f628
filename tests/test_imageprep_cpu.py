"""Image preprocessing without a GPU: the package's vectorised host form of Pillow's antialiased 8-bit resize against the plain-loop definition
(tests/imageprep_ref.py), both against outputs recorded from Pillow (tests/golden/pil_resize.npz) and against Pillow itself where it is
installed; the min-max rule; ResizeLongestSide's coordinate arithmetic; the C entry names."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import imageprep_ref as R
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ullsam_resize_u8_aa_h", "ullsam_resize_u8_aa_v", "ullsam_minmax_u16", "ullsam_minmax_f32", "ullsam_normalize_to_u8_u16",
           "ullsam_normalize_to_u8_f32"]


@functools.lru_cache(maxsize=None)
def ref_resize(case):
    i, _, f = case
    return R.resize(R.case_image(case), R.SHAPES[i][1], f)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_host_form_equals_the_loop_definition_and_the_golden_file(case):
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    i, c, f = case
    img = R.case_image(case)
    want = ref_resize(case)
    got = resize_u8_aa_host(img, R.SHAPES[i][1], f)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    planar = np.ascontiguousarray(img.transpose(2, 0, 1)).transpose(1, 2, 0)        # the same image as a strided view of a planar buffer
    assert np.array_equal(resize_u8_aa_host(planar, R.SHAPES[i][1], f), want)
    if c == 1:
        assert np.array_equal(resize_u8_aa_host(img[:, :, 0], R.SHAPES[i][1], f), want[:, :, 0])
    if c == 3:
        g = U.gold("pil_resize")
        assert np.array_equal(g[R.case_id(case)], want) and np.array_equal(g[R.case_id(case)], got)


def test_bicubic_cases_reach_the_clamp_on_both_sides():
    """The case content is built so that the unclamped bicubic sum leaves 0..255 in both directions: the clamp is exercised, not assumed."""
    case = (2, 3, "bicubic")                                                        # (50, 31) -> (64, 64): an upscale keeps the 0 / 255 steps sharp
    out = ref_resize(case)
    assert (out == 0).any() and (out == 255).any()
    img = R.case_image(case).astype(np.int64)
    bounds, ks = R.coeffs(img.shape[1], R.SHAPES[2][1][1], "bicubic")
    acc = np.stack([sum(img[:, x0 + x] * k[x] for x in range(n)) for (x0, n), k in zip(bounds, ks)], 1) + (1 << 21)
    assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_host_form_and_loop_definition_equal_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    i, c, f = case
    (_, _), (oh, ow) = R.SHAPES[i]
    img = R.case_image(case)
    if c == 4:                                                                       # CMYK: four independent 8-bit bands (RGBA would premultiply)
        pil_in = Image.frombytes("CMYK", (img.shape[1], img.shape[0]), img.tobytes())
    else:
        pil_in = Image.fromarray(img[:, :, 0] if c == 1 else img)                    # modes L and RGB
    assert pil_in.mode == {1: "L", 3: "RGB", 4: "CMYK"}[c]
    want = np.array(pil_in.resize((ow, oh), R.PIL_FILTER[f])).reshape(oh, ow, c)
    assert np.array_equal(ref_resize(case), want)
    assert np.array_equal(resize_u8_aa_host(img, (oh, ow), f), want)


def test_tables_are_cached_and_the_skipped_pass_is_the_identity():
    from ullsam_amd import ops
    b, k = ops.aa_tables(100, 1, "bilinear")
    assert k.shape == (1, 201) and b.tolist() == [[0, 100]] and k.dtype == np.int32 and b.dtype == np.int32
    assert ops.aa_tables(100, 1, "bilinear")[1] is k
    b, k = ops.aa_tables(7, 7, "bicubic")
    assert b.tolist() == [[i, 1] for i in range(7)] and k.tolist() == [[1 << 22]] * 7
    for (n_in, n_out, f) in ((53, 16, "bicubic"), (31, 64, "bilinear"), (3, 5, "bicubic")):
        b, k = ops.aa_tables(n_in, n_out, f)
        rb, rk = R.coeffs(n_in, n_out, f)
        assert b.tolist() == [list(v) for v in rb]
        assert all(k[i, :n].tolist() == rk[i] and not k[i, n:].any() for i, (_, n) in enumerate(rb))
        assert 255 * int(np.abs(k.astype(np.int64)).sum(1).max()) < 2 ** 31          # the signed 32-bit sum cannot overflow
    with pytest.raises(ValueError):
        ops.aa_tables(4, 4, "lanczos")


def test_window_is_the_apps_centred_pad():
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    for (h, w) in ((45, 70), (70, 45)):
        img = R.make_image(h, w, 3, seed=5)
        size = max(h, w)
        padded = R.pad_to_square(img)
        assert padded.shape == (size, size, 3)
        got = resize_u8_aa_host(img, (32, 32), "bilinear", window=((size - h) // 2, (size - w) // 2, size, size))
        assert np.array_equal(got, R.resize(padded, (32, 32), "bilinear"))


@pytest.mark.parametrize("name", sorted(R.to_uint8_inputs()))
def test_to_uint8_equals_the_numpy_expression(name):
    from ullsam_amd.utils.imageprep import to_uint8
    a = R.to_uint8_inputs()[name]
    want = R.minmax_u8(a)
    got = to_uint8(a)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    t = to_uint8(torch.from_numpy(a))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and np.array_equal(t.numpy(), want)


def test_to_uint8_passes_uint8_through_and_drops_alpha():
    from ullsam_amd.utils.imageprep import to_uint8
    a = R.make_image(6, 5, 4)
    assert np.array_equal(to_uint8(a), a[:, :, :3])
    assert to_uint8(a[:, :, :3]) is not None and np.array_equal(to_uint8(a[:, :, 0]), a[:, :, 0])
    f = np.random.default_rng(0).random((6, 5, 4), dtype=np.float32)
    assert np.array_equal(to_uint8(f), R.minmax_u8(f)[:, :, :3])                    # min and max are taken with the alpha channel, as the app does


def test_preprocess_image_host_form_equals_the_golden_file():
    from ullsam_amd.utils.imageprep import preprocess_image
    (h, w, c), S = R.PREPROCESS_CASE
    img = R.make_image(h, w, c, seed=99)
    want = torch.from_numpy(U.gold("pil_resize")["preprocess"])
    got = preprocess_image(img, img_size=S)
    assert got.dtype == torch.float32 and got.shape == (1, 3, S, S) and torch.equal(got, want)
    assert torch.equal(preprocess_image(torch.from_numpy(img), img_size=S), want)
    grey = preprocess_image(img[:, :, 0], img_size=S)
    assert torch.equal(grey[0, 0], want[0, 0]) and torch.equal(grey[0, 1], grey[0, 0]) and torch.equal(grey[0, 2], grey[0, 0])
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    u8 = torch.from_numpy(R.resize(R.pad_to_square(img), (S, S))).long()
    norm = torch.stack([((torch.arange(256).float().div(255) - m) / s)[u8[:, :, i]] for i, (m, s) in enumerate(zip(mean, std))])[None]
    assert torch.equal(preprocess_image(img, img_size=S, mean=mean, std=std), norm)
    stretched = preprocess_image(img, img_size=S, pad_to_square=False)
    assert torch.equal(stretched[0], torch.from_numpy(R.resize(img, (S, S))).permute(2, 0, 1).float().div(255))


def test_resize_longest_side_coordinates_and_shapes():
    from ullsam_amd.utils.transforms import ResizeLongestSide

    def shape(oldh, oldw, L):                                                        # the reference's formula (utils/transforms.py:93-102)
        scale = L * 1.0 / max(oldh, oldw)
        return int(oldh * scale + 0.5), int(oldw * scale + 0.5)

    for (h, w, L) in ((129, 257, 64), (515, 770, 1024), (1024, 1024, 1024), (3, 4, 2), (600, 800, 1024), (2048, 1000, 1024)):
        assert ResizeLongestSide.get_preprocess_shape(h, w, L) == shape(h, w, L)
    assert ResizeLongestSide.get_preprocess_shape(3, 4, 2) == (2, 2)                # 1.5 rounds up
    assert ResizeLongestSide.get_preprocess_shape(129, 257, 64) == (32, 64)
    rng = np.random.default_rng(3)
    for (h, w, L) in ((129, 257, 64), (515, 770, 1024), (3, 4, 2)):
        t = ResizeLongestSide(L)
        nh, nw = shape(h, w, L)
        pts = rng.uniform(0, 300, (5, 2, 2))
        want = pts.copy()
        want[..., 0] = want[..., 0] * (nw / w)
        want[..., 1] = want[..., 1] * (nh / h)
        keep = pts.copy()
        got = t.apply_coords(pts, (h, w))
        assert got.dtype == np.float64 and np.array_equal(got, want) and np.array_equal(pts, keep)
        boxes = pts.reshape(-1, 4)
        assert np.array_equal(t.apply_boxes(boxes, (h, w)), want.reshape(-1, 4))
        ipts = rng.integers(0, 300, (4, 2))
        assert np.array_equal(t.apply_coords(ipts, (h, w)), np.stack([ipts[:, 0] * (nw / w), ipts[:, 1] * (nh / h)], 1))
        tp = torch.from_numpy(pts).float()
        wt = tp.clone()
        wt[..., 0] = wt[..., 0] * (nw / w)
        wt[..., 1] = wt[..., 1] * (nh / h)
        gt = t.apply_coords_torch(tp, (h, w))
        assert gt.dtype == torch.float32 and torch.equal(gt, wt) and torch.equal(tp, torch.from_numpy(keep).float())
        assert torch.equal(t.apply_boxes_torch(tp.reshape(-1, 4), (h, w)), wt.reshape(-1, 4))
    img = R.make_image(129, 257, 3)
    t = ResizeLongestSide(64)
    out = t.apply_image(img)
    assert isinstance(out, np.ndarray) and np.array_equal(out, R.resize(img, (32, 64)))
    out_t = t.apply_image(torch.from_numpy(img))
    assert isinstance(out_t, torch.Tensor) and not out_t.is_cuda and np.array_equal(out_t.numpy(), out)
    x = torch.from_numpy(U.rand_image((2, 3, 40, 30), 1))
    assert torch.equal(t.apply_image_torch(x), torch.nn.functional.interpolate(x, (64, 48), mode="bilinear", align_corners=False, antialias=True))


def test_header_binding_and_library_agree_on_the_imageprep_entry_points():
    from ullsam_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code)
        assert m, s
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[s]), s            # one ctypes entry per C parameter
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in SYMBOLS)
    for fn in ("resize_u8_aa", "normalize_to_u8", "aa_tables"):
        assert callable(getattr(ops, fn))
    with pytest.raises(_lib.UllsamError):                                          # the wrappers take GPU tensors only; the host form lives in utils.imageprep
        ops.resize_u8_aa(torch.zeros((4, 4, 3), dtype=torch.uint8), (2, 2))
    with pytest.raises(_lib.UllsamError):
        ops.normalize_to_u8(torch.zeros((4, 4), dtype=torch.float32))
