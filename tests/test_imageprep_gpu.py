"""Image preprocessing on the device (csrc/imageprep.hip) against the package's host form of the same definition, which tests/test_imageprep_cpu.py
pins to the loop definition, the golden file and Pillow.  Every comparison is bit-exact (torch.equal)."""
import functools

import numpy as np
import pytest
import torch

from tests import imageprep_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL = -12345.0


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def host_resize(case):
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    i, _, f = case
    return resize_u8_aa_host(R.case_image(case), R.SHAPES[i][1], f)


@functools.lru_cache(maxsize=None)
def host_lut():
    """[3, 256] on the host: ToTensor + Normalize over the 256 byte values, by the ops the reference's transform applies."""
    return torch.stack([(torch.arange(256).float().div(255) - m) / s for m, s in zip(MEAN, STD)])


def host_float(u8):
    """uint8 [OH, OW, C] -> float32 [3, OH, OW] gathered from host_lut (C == 1 replicates, the alpha of C == 4 is dropped)."""
    idx = torch.from_numpy(u8).long()
    c = u8.shape[2]
    return torch.stack([host_lut()[k][idx[:, :, 0 if c == 1 else k]] for k in range(3)])


def device_source(img, layout):
    """The image on the device as the [H, W, C] view ops.resize_u8_aa takes: of an interleaved or of a planar buffer."""
    if layout == "interleaved":
        return T(img)
    return T(img.transpose(2, 0, 1)).permute(1, 2, 0)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_device_equals_the_host_form(case, layout):
    """uint8 output and float output through a non-trivial table, for every case and both source layouts; where the output fits, the float output
    goes into slot 1 of a [3, 3, 40, 40] batch filled with a sentinel, which must survive everywhere else; two runs give the same bits."""
    from ullsam_amd import ops
    from ullsam_amd.utils.imageprep import normalize_lut
    i, c, f = case
    oh, ow = R.SHAPES[i][1]
    want = host_resize(case)
    src = device_source(R.case_image(case), layout)
    lut = normalize_lut(MEAN, STD)
    assert torch.equal(lut, host_lut())
    lut = lut.to(DEV)
    fits = oh <= 40 and ow <= 40
    runs = []
    for _ in range(2):
        batch = torch.full((3, 3, 40, 40), SENTINEL, device=DEV) if fits else None
        u8, f32 = ops.resize_u8_aa(src, (oh, ow), f, lut=lut, out=batch[1] if fits else None)
        runs.append((u8.cpu(), (batch if fits else f32).cpu()))
    u8, f32 = runs[0]
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.from_numpy(want))
    if fits:
        expect = torch.full((3, 3, 40, 40), SENTINEL)
        expect[1, :, :oh, :ow] = host_float(want)
        assert torch.equal(f32, expect)
    else:
        assert f32.shape == (3, oh, ow) and torch.equal(f32, host_float(want))
    assert torch.equal(runs[1][0], u8) and torch.equal(runs[1][1], f32)
    only_f32 = ops.resize_u8_aa(src, (oh, ow), f, lut=lut, want_u8=False)
    assert only_f32[0] is None and torch.equal(only_f32[1].cpu(), host_float(want))
    assert torch.equal(ops.resize_u8_aa(src, (oh, ow), f)[0].cpu(), u8)


@pytest.mark.parametrize("hw", [(45, 70), (70, 45)])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_source_window_is_the_centred_pad(hw, layout):
    """The pad to a square as a parameter of the horizontal pass, against the host form on an np.pad-ed copy; 70 - 45 is odd, so (size - h) // 2
    and its remainder differ."""
    from ullsam_amd import ops
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    h, w = hw
    size = max(h, w)
    img = R.make_image(h, w, 3, seed=5)
    window = ((size - h) // 2, (size - w) // 2, size, size)
    for f in R.FILTERS:
        want = resize_u8_aa_host(R.pad_to_square(img), (32, 32), f)
        got = ops.resize_u8_aa(device_source(img, layout), (32, 32), f, window=window)[0]
        assert torch.equal(got.cpu(), torch.from_numpy(want))
    crop = device_source(np.pad(img, ((3, 2), (4, 1), (0, 0)), constant_values=200), layout)[3:3 + h, 4:4 + w]      # a crop view: nothing outside it is read
    assert torch.equal(ops.resize_u8_aa(crop, (32, 32), window=window)[0].cpu(), torch.from_numpy(resize_u8_aa_host(R.pad_to_square(img), (32, 32))))


@pytest.mark.parametrize("name", sorted(R.to_uint8_inputs()) + ["u16_ramp"])
def test_normalize_to_u8_equals_the_numpy_expression(name):
    from ullsam_amd import ops
    from ullsam_amd.utils.imageprep import to_uint8
    a = (np.arange(257 * 129, dtype=np.uint16).reshape(257, 129) * 3 + 11).astype(np.uint16) if name == "u16_ramp" else R.to_uint8_inputs()[name]
    want = torch.from_numpy(R.minmax_u8(a))
    got = ops.normalize_to_u8(T(a))
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got.cpu(), want)
    assert torch.equal(ops.normalize_to_u8(T(a)).cpu(), want)
    assert torch.equal(to_uint8(T(a)).cpu(), want)


def test_preprocess_image_equals_the_golden_file():
    from ullsam_amd.utils.imageprep import preprocess_image
    (h, w, c), S = R.PREPROCESS_CASE
    img = R.make_image(h, w, c, seed=99)
    want = torch.from_numpy(U.gold("pil_resize")["preprocess"])
    got = preprocess_image(img, img_size=S, device=DEV)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (1, 3, S, S) and torch.equal(got.cpu(), want)
    assert torch.equal(preprocess_image(T(img), img_size=S).cpu(), want)
    assert torch.equal(preprocess_image(T(img.transpose(2, 0, 1)).permute(1, 2, 0), img_size=S).cpu(), want)
    batch = torch.full((2, 3, S, S), SENTINEL, device=DEV)
    preprocess_image(T(img), img_size=S, out=batch[1])
    assert torch.equal(batch[1].cpu(), want[0]) and bool((batch[0] == SENTINEL).all())
    for kw in (dict(mean=MEAN, std=STD), dict(pad_to_square=False), dict(filter="bicubic")):
        assert torch.equal(preprocess_image(img, img_size=S, device=DEV, **kw).cpu(), preprocess_image(img, img_size=S, **kw))
    rgba = np.concatenate([img, R.make_image(h, w, 1, seed=3)], 2)
    assert torch.equal(preprocess_image(rgba, img_size=S, device=DEV).cpu(), want)
    u16 = R.to_uint8_inputs()["u16_range65535"]
    assert torch.equal(preprocess_image(u16, img_size=S, device=DEV).cpu(), preprocess_image(u16, img_size=S))


def test_resize_longest_side_apply_image_on_the_device():
    from ullsam_amd.utils.transforms import ResizeLongestSide
    img = R.make_image(129, 257, 3)
    t = ResizeLongestSide(64)
    got = t.apply_image(T(img))
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (32, 64, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(t.apply_image(img)))


def test_real_size_image_equals_the_host_form():
    from ullsam_amd import ops
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    from ullsam_amd.utils.transforms import ResizeLongestSide
    img = R.make_image(515, 770, 3, seed=8)
    hw = ResizeLongestSide.get_preprocess_shape(515, 770, 1024)
    assert hw == (685, 1024)
    assert torch.equal(ops.resize_u8_aa(T(img), hw)[0].cpu(), torch.from_numpy(resize_u8_aa_host(img, hw)))


def _amg_kw():
    return dict(points_per_side=4, points_per_batch=64, pred_iou_thresh=-1e3, stability_score_thresh=0.5, stability_score_offset=0.05,
                output_mode="uncompressed_rle")


def test_generator_pil_resize_feeds_the_encoder_the_exact_crop():
    """image_resize="pil": the tokens _encode returns are those of forward_tokens on the host-form resize of the crop."""
    from tests.test_amg_gpu import _small_sam
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    from ullsam_amd.utils.imageprep import resize_u8_aa_host
    sam, _ = _small_sam()
    S = sam.image_encoder.img_size
    img = R.make_image(200, 333, 3, seed=12)
    gen = SamAutomaticMaskGenerator(sam, image_resize="pil", **_amg_kw())
    crop = T(img.transpose(2, 0, 1))[:, 10:190, 20:300]                             # a crop view of the planar uint8 image, as _process_crop passes it
    with torch.no_grad():
        tok, input_size = gen._encode(crop)
    nh, nw = int(180 * (S / 280) + 0.5), S
    assert input_size == (nh, nw)
    x = torch.from_numpy(resize_u8_aa_host(img[10:190, 20:300], (nh, nw))).permute(2, 0, 1).float().contiguous().to(DEV)
    mean = sam.pixel_mean.reshape(-1).float().contiguous()
    std = sam.pixel_std.reshape(-1).float().contiguous()
    with torch.no_grad():
        assert torch.equal(tok, sam.image_encoder.forward_tokens(x[None].contiguous(), mean, std))
        plain = SamAutomaticMaskGenerator(sam, **_amg_kw())._encode(crop.float())[0]
    assert not torch.equal(tok, plain)                                               # the two settings are different filters


def test_generator_settings_agree_when_no_resize_is_needed_and_pil_needs_uint8():
    from tests.test_amg_gpu import _small_sam
    from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
    sam, _ = _small_sam()
    S = sam.image_encoder.img_size
    img = R.make_image(100, S, 3, seed=13)
    a = SamAutomaticMaskGenerator(sam, **_amg_kw()).generate(img)
    b = SamAutomaticMaskGenerator(sam, image_resize="pil", **_amg_kw()).generate(img)
    c = SamAutomaticMaskGenerator(sam, image_resize="pil", **_amg_kw()).generate(torch.from_numpy(img.transpose(2, 0, 1).copy()))
    assert len(a) > 0 and a == b and a == c
    big = R.make_image(150, 200, 3, seed=14)
    assert len(SamAutomaticMaskGenerator(sam, image_resize="pil", **_amg_kw()).generate(big)) > 0
    with pytest.raises(ValueError):
        SamAutomaticMaskGenerator(sam, image_resize="pil", **_amg_kw()).generate(img.astype(np.float32))
    with pytest.raises(ValueError):
        SamAutomaticMaskGenerator(sam, image_resize="pil", **_amg_kw()).generate(torch.from_numpy(img.transpose(2, 0, 1).copy()).float())
    with pytest.raises(ValueError):
        SamAutomaticMaskGenerator(sam, image_resize="lanczos")
