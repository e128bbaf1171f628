"""ResizeLongestSide with the reference's interface and semantics (utils/transforms.py).  apply_image is Pillow's antialiased 8-bit resize,
bit-exact: on a uint8 GPU tensor it runs the kernels of csrc/imageprep.hip, on a numpy array or CPU tensor the host form of the same
definition (utils.imageprep.resize_u8_aa_host) -- neither goes through PIL or torchvision."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
from torch.nn import functional as F

from .. import ops
from .imageprep import resize_u8_aa_host


class ResizeLongestSide:
    """Resizes images to the longest side 'target_length', and resizes coordinates and boxes with them; numpy arrays and batched torch tensors."""

    def __init__(self, target_length: int) -> None:
        self.target_length = target_length

    def apply_image(self, image):
        """uint8 HxWxC (C in 1, 3, 4; or HxW): np.array(resize(to_pil_image(image), target_size)) of utils/transforms.py:26-31, channels resampled
        independently.  A numpy array returns a numpy array, a CPU tensor a CPU tensor (host form); a CUDA tensor a CUDA tensor (kernels)."""
        target_size = self.get_preprocess_shape(image.shape[0], image.shape[1], self.target_length)
        if isinstance(image, torch.Tensor):
            if image.dtype != torch.uint8:
                raise TypeError(f"apply_image expects uint8, got {image.dtype}")
            if image.is_cuda:
                with torch.cuda.device(image.device):
                    out = ops.resize_u8_aa(image, target_size)[0]
                return out[:, :, 0] if image.dim() == 2 else out
            return torch.from_numpy(resize_u8_aa_host(image.numpy(), target_size))
        return resize_u8_aa_host(image, target_size)

    def _ratios(self, original_size: Tuple[int, ...]) -> Tuple[float, float]:
        """(x ratio, y ratio) = (new_w / old_w, new_h / old_h) as Python floats: the factors every coordinate method multiplies by."""
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(old_h, old_w, self.target_length)
        return new_w / old_w, new_h / old_h

    def apply_coords(self, coords: np.ndarray, original_size: Tuple[int, ...]) -> np.ndarray:
        """numpy [..., 2] as (x, y) in the original image of size original_size = (H, W) -> float64 coordinates in the resized image."""
        rx, ry = self._ratios(original_size)
        out = np.array(coords, dtype=float)                    # a copy, as the reference's deepcopy(...).astype(float)
        out[..., 0] = out[..., 0] * rx
        out[..., 1] = out[..., 1] * ry
        return out

    def apply_boxes(self, boxes: np.ndarray, original_size: Tuple[int, ...]) -> np.ndarray:
        """numpy [B, 4] XYXY -> [B, 4]: both corners through apply_coords."""
        return self.apply_coords(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)

    def apply_image_torch(self, image: torch.Tensor) -> torch.Tensor:
        """BxCxHxW float, on whatever device it is: the float path, F.interpolate with antialias.  As the reference says of it, it may not exactly
        match apply_image, which is the transformation the model expects; nothing in the reference calls it."""
        target_size = self.get_preprocess_shape(image.shape[2], image.shape[3], self.target_length)
        return F.interpolate(image, target_size, mode="bilinear", align_corners=False, antialias=True)

    def apply_coords_torch(self, coords: torch.Tensor, original_size: Tuple[int, ...]) -> torch.Tensor:
        """tensor [..., 2] as (x, y) -> float32 coordinates in the resized image, on the same device."""
        rx, ry = self._ratios(original_size)
        out = coords.detach().clone().to(torch.float)
        out[..., 0] = out[..., 0] * rx
        out[..., 1] = out[..., 1] * ry
        return out

    def apply_boxes_torch(self, boxes: torch.Tensor, original_size: Tuple[int, ...]) -> torch.Tensor:
        """tensor [B, 4] XYXY -> [B, 4]: both corners through apply_coords_torch."""
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)

    @staticmethod
    def get_preprocess_shape(oldh: int, oldw: int, long_side_length: int) -> Tuple[int, int]:
        """(newh, neww): both sides times long_side_length / max(oldh, oldw), rounded half up."""
        scale = long_side_length * 1.0 / max(oldh, oldw)
        return (int(oldh * scale + 0.5), int(oldw * scale + 0.5))
