"""Image preprocessing: what every entry point of the reference does on the host before the model sees an image -- min-max normalisation of
a non-8-bit image to uint8 (app.py:190-191, 226-228), the centred zero pad to a square (app.py:111-143, 232-239), Pillow's antialiased 8-bit
`Image.resize` and `ToTensor` + `Normalize` (app.py:242-249; the datasets' transform, train_joint_v2.py:271-275, 299-300) -- as kernels
(csrc/imageprep.hip) and as a vectorised numpy host form of the same definition.  Both are bit-exact with Pillow: the resize is integer
arithmetic over coefficient tables built on the host in float64 (ops.aa_tables), and the float conversion is a 256-entry table per channel
computed by the torch ops the reference uses.  PIL is not imported.

    x = preprocess_image(tile_u8, device="cuda")           # uint8 [H, W, 3] -> float32 [1, 3, 1024, 1024], as app.preprocess_image returns it

A numpy array or CPU tensor without device= takes the host form; a CUDA tensor or device=... takes the kernels.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

_LUT = {}


def _pass_host(a: np.ndarray, out_size: int, filter: str, in_size: int, origin: int) -> np.ndarray:
    """One pass along axis 1 of a uint8 [R, n, C] array that holds source columns origin .. origin + n - 1 of an axis of `in_size`."""
    if in_size == out_size:
        return a                                                      # the pass Pillow skips
    bounds, coef = ops.aa_tables(in_size, out_size, filter)
    acc = np.full((a.shape[0], out_size, a.shape[2]), 1 << (ops.AA_BITS - 1), np.int32)
    for j in range(coef.shape[1]):
        idx = np.minimum(bounds[:, 0] - origin + j, a.shape[1] - 1)   # (a tap past the count carries a zero coefficient)
        acc += a[:, idx, :].astype(np.int32) * coef[None, :, j, None]
    return np.clip(acc >> ops.AA_BITS, 0, 255).astype(np.uint8)


def resize_u8_aa_host(img: np.ndarray, out_hw, filter: str = "bilinear", window=None) -> np.ndarray:
    """The host form of ops.resize_u8_aa: uint8 [H, W, C] or [H, W] -> uint8 [OH, OW, C] or [OH, OW] = PIL's Image.resize(..., BILINEAR / BICUBIC)
    with channels independent.  window = (top, left, VH, VW) places the image in a zero image of that size first."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.size == 0:
        raise TypeError(f"resize_u8_aa_host takes a non-empty uint8 [H, W] or [H, W, C] array, got {img.dtype} {img.shape}")
    a = img[:, :, None] if img.ndim == 2 else img
    if window is not None:
        top, left, VH, VW = (int(v) for v in window)
        if not (top >= 0 and left >= 0 and top + a.shape[0] <= VH and left + a.shape[1] <= VW):
            raise ValueError(f"the image {a.shape[:2]} at {(top, left)} does not lie inside the window {(VH, VW)}")
        full = np.zeros((VH, VW, a.shape[2]), np.uint8)
        full[top:top + a.shape[0], left:left + a.shape[1]] = a
        a = full
    OH, OW = (int(v) for v in out_hw)
    VH, VW = a.shape[:2]
    row0, rows = ops.aa_row_span(VH, OH, filter)                      # the horizontal pass runs over the rows the vertical pass reads
    t = _pass_host(a[row0:row0 + rows], OW, filter, VW, 0)
    t = _pass_host(t.transpose(1, 0, 2), OH, filter, VH, row0).transpose(1, 0, 2)
    t = np.ascontiguousarray(t)
    return t[:, :, 0] if img.ndim == 2 else t


def _minmax_u8_numpy(a: np.ndarray) -> np.ndarray:
    return ((a - a.min()) / (a.max() - a.min() + 1e-8) * 255).astype(np.uint8)      # app.py:191, verbatim


def to_uint8(image):
    """The app's rule for an uploaded array (app.py:190-196): uint8 passes through; anything else becomes
    ((img - img.min()) / (img.max() - img.min() + 1e-8) * 255).astype(np.uint8) with numpy's types (a uint16 image: difference in uint16, quotient
    and product in float64; a float32 image: float32 throughout); then the alpha channel of [H, W, 4] is dropped.  numpy in, numpy out; CPU tensor in,
    CPU tensor out (both by the numpy expression itself); a CUDA tensor (uint8, uint16 or float32) runs ops.normalize_to_u8.  NaN is out of scope."""
    if isinstance(image, torch.Tensor):
        if image.is_cuda:
            if image.dtype != torch.uint8:
                with torch.cuda.device(image.device):
                    image = ops.normalize_to_u8(image.contiguous())
        else:
            a = image.numpy()
            image = image if a.dtype == np.uint8 else torch.from_numpy(_minmax_u8_numpy(a))
    else:
        image = np.asarray(image)
        if image.dtype != np.uint8:
            image = _minmax_u8_numpy(image)
    return image[:, :, :3] if image.ndim == 3 and image.shape[2] == 4 else image


def normalize_lut(mean=(0, 0, 0), std=(1, 1, 1)) -> torch.Tensor:
    """ToTensor + Normalize over the 256 possible values: float32 [3, 256] on the CPU, by the reference's own torch ops (uint8 -> float32, div(255),
    sub(mean), div(std)) -- so a gather from it equals the transform bit for bit, with no division on the device."""
    m = torch.as_tensor([float(v) for v in mean], dtype=torch.float32)
    s = torch.as_tensor([float(v) for v in std], dtype=torch.float32)
    if m.numel() != 3 or s.numel() != 3:
        raise ValueError("mean and std must have three entries")
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return v[None, :].repeat(3, 1).sub_(m[:, None]).div_(s[:, None]).contiguous()


def _lut_on(mean, std, device) -> torch.Tensor:
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), str(device))
    hit = _LUT.get(key)
    if hit is None:
        if len(_LUT) >= 16:
            _LUT.clear()
        hit = _LUT[key] = normalize_lut(mean, std).to(device)
    return hit


def preprocess_image(image, img_size: int = 1024, pad_to_square: bool = True, mean=(0, 0, 0), std=(1, 1, 1), filter: str = "bilinear",
                     out=None, device=None) -> torch.Tensor:
    """app.preprocess_image (app.py:213-249) and the datasets' transform(Image.open(...).convert('RGB')): image [H, W] or [H, W, 1 | 3 | 4], uint8 /
    uint16 / float32, numpy or tensor -> float32 [1, 3, S, S], S = img_size: to_uint8, grey replicated to RGB, (pad_to_square) the centred zero pad
    with pad_top = (size - h) // 2, pad_left = (size - w) // 2, Pillow's antialiased resize to S x S, ToTensor, Normalize(mean, std).
    A CUDA tensor, or any input with device=..., runs the kernels (the pad is a parameter of the horizontal pass, not a copy) and returns a tensor
    there; a numpy array or CPU tensor without device= runs the host form and returns a CPU tensor.  out: float32 [1, 3, S, S] or [3, S, S] to fill
    (a slot of a batch).  The result feeds InternVLSAMModel.forward(pixel_values=...) unchanged."""
    S = int(img_size)
    on_device = device is not None or (isinstance(image, torch.Tensor) and image.is_cuda)
    if on_device:
        if not isinstance(image, torch.Tensor):
            a = np.ascontiguousarray(image)
            image = torch.from_numpy(a)
        dev = torch.device(device) if device is not None else image.device
        if dev.type != "cuda":
            raise ValueError(f"preprocess_image: device {device!r} is not a GPU; leave device=None for the host form")
        image = image.to(dev)
    u8 = to_uint8(image)
    if u8.ndim not in (2, 3) or (u8.ndim == 3 and u8.shape[2] not in (1, 3)) or u8.shape[0] == 0 or u8.shape[1] == 0:
        raise ValueError(f"preprocess_image takes [H, W] or [H, W, 1 | 3 | 4], got {tuple(image.shape)}")
    h, w = int(u8.shape[0]), int(u8.shape[1])
    window = None
    if pad_to_square and h != w:
        size = max(h, w)
        window = ((size - h) // 2, (size - w) // 2, size, size)
    slot = None
    if out is not None:
        slot = out[0] if out.dim() == 4 and out.shape[0] == 1 else out
        if tuple(slot.shape) != (3, S, S) or slot.dtype != torch.float32:
            raise ValueError(f"out must be float32 [1, 3, {S}, {S}] or [3, {S}, {S}], got {tuple(out.shape)} {out.dtype}")
    if on_device:
        with torch.cuda.device(u8.device):
            _, f = ops.resize_u8_aa(u8, (S, S), filter, window, _lut_on(mean, std, u8.device), slot, want_u8=False)
        return out if out is not None and out.dim() == 4 else f[None]
    a = u8.numpy() if isinstance(u8, torch.Tensor) else u8
    r = resize_u8_aa_host(a, (S, S), filter, window)
    r = r[:, :, None] if r.ndim == 2 else r
    lut = normalize_lut(mean, std)
    idx = torch.from_numpy(np.ascontiguousarray(r)).long()
    f = torch.stack([lut[c][idx[:, :, c if r.shape[2] == 3 else 0]] for c in range(3)])
    if slot is not None:
        slot.copy_(f)
        return out if out.dim() == 4 else slot[None]
    return f[None]
