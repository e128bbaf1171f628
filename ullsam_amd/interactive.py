"""The interactive loop of the reference's click-to-segment app (app.py:497-661 process_image, 665-725 save_instance, 728-785 visualize_masks,
836-882 clear / reset, 788-833 export_mask) as a session: the image encoder, the projector and the LLM prefill run ONCE per image, a click runs
the prompt encoder, the mask decoder and one finish kernel (ops.click_finish), and the mask, the label canvas and the overlay stay on the GPU.

    seg = InteractiveSegmenter(model, input_ids)            # the tokenised prompt with its <IMG_CONTEXT> span, as for model.forward
    seg.set_image(image)                                     # [H, W] or [H, W, 1 | 3 | 4], uint8 / uint16 / float32
    r = seg.click([[412, 300]], [1])                         # display-image pixels (x, y); r.mask, r.overlay, r.iou, r.area, r.box, r.low
    overlay = seg.save_instance()                            # the mask becomes instance count + 1 of seg.labels
    tif = seg.export_labels()                                # uint16 on the host

Definitions: DESIGN.md "7b, continued: the interactive loop".  Plain Sam is not covered (Sam.forward and the mask generator serve it).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .utils import imageprep
from .utils.interactive import blend_luts, frame_coords


@dataclass
class ClickResult:
    mask: torch.Tensor       # uint8 [H, W]
    overlay: torch.Tensor    # uint8 [H, W, 3]
    iou: torch.Tensor        # fp32 [1], the decoder's IoU prediction
    area: torch.Tensor       # int32 scalar
    box: torch.Tensor        # int32 [4], XYXY with inclusive maxima, zeros for an empty mask
    low: torch.Tensor        # fp32 [1, 1, 256, 256] logits (a mask_input for the next click)


class InteractiveSegmenter:
    def __init__(self, model, input_ids, attention_mask=None, use_llm_prompt: bool = True, palette=None, mask_threshold: float = 0.0):
        if model.training:
            raise ValueError("InteractiveSegmenter takes a model in eval() mode")
        self.model = model
        self.device = model.device
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.shape[0] != 1:
            raise ValueError(f"input_ids must be [1, S], got {tuple(ids.shape)}")
        self.input_ids = ids.to(self.device)
        self.attention_mask = torch.ones_like(self.input_ids) if attention_mask is None else torch.as_tensor(attention_mask).to(self.device)
        self.use_llm_prompt = bool(use_llm_prompt)
        self.mask_threshold = float(mask_threshold)
        self.frame = int(model.vision_model.img_size)
        lut_inst, lut_cur = blend_luts(palette)
        self.lut_inst = torch.from_numpy(lut_inst).to(self.device)
        self.lut_cur = torch.from_numpy(lut_cur).to(self.device)
        self.image = None
        self.image_cache: dict = {}
        self.count = 0
        self._current = None          # (low fp32 [1, LH, LW], mask uint8 [H, W]) of the last click
        self._no_low = torch.zeros((1, 1, 1), dtype=torch.float32, device=self.device)   # render without a current mask: the kernel wants P >= 1

    # -- per image ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def set_image(self, image) -> None:
        m, dev = self.model, self.device
        if not isinstance(image, torch.Tensor):
            image = torch.from_numpy(np.ascontiguousarray(image))
        with torch.cuda.device(dev):
            u8 = imageprep.to_uint8(image.to(dev))              # also drops the alpha channel of [H, W, 4]: 1 or 3 channels are left below
            if u8.dim() not in (2, 3) or (u8.dim() == 3 and u8.shape[2] not in (1, 3)) or u8.shape[0] == 0 or u8.shape[1] == 0:
                raise ValueError(f"set_image takes [H, W] or [H, W, 1 | 3 | 4], got {tuple(image.shape)}")
            H, W = int(u8.shape[0]), int(u8.shape[1])
            self.image = (u8.reshape(H, W, 1) if u8.dim() == 2 else u8).expand(H, W, 3).contiguous()   # grey replicated (convert("RGB"))
            self.H, self.W = H, W
            self.side = max(H, W)
            self.top, self.left = (self.side - H) // 2, (self.side - W) // 2
            x = imageprep.preprocess_image(u8, img_size=self.frame, device=dev).to(m.dtype)
            ids = self.input_ids
            out = m(pixel_values=x, input_ids=ids, attention_mask=self.attention_mask, image_flags=(ids == m.img_context_token_id)[..., None].long(),
                    return_dict=True, use_cache=False, output_hidden_states=True)
            pe = m.prompt_encoder
            # the image embedding as the model API hands it to the mask decoder: in the model's dtype (forward's image_embeddings), read back as fp32
            self.image_tokens = ops.cast(ops.cast(out.image_tokens, m.dtype), torch.float32)
            self.dense_pe = pe.dense_pe_tokens()
            self.dense = pe.dense_tokens(1, None, out.dense_feature_tokens if self.use_llm_prompt else None)
            self.image_cache = {}
            self.labels = torch.zeros((H, W), dtype=torch.int32, device=dev)
        self.count = 0
        self._current = None

    def _need_image(self):
        if self.image is None:
            raise RuntimeError("call set_image first")

    # -- per prompt -----------------------------------------------------------------------------------------------------------------------
    def _to_frame(self, xy) -> torch.Tensor:
        """Display pixels -> frame pixels in Python floats on the host (utils.interactive.frame_coords), uploaded once: coordinates that
        arrive as device tensors (prompts_from_labels) make one round trip of a few numbers here."""
        a = xy.detach().cpu().numpy() if isinstance(xy, torch.Tensor) else np.asarray(xy)
        return torch.from_numpy(frame_coords(a, self.frame, self.side, self.top, self.left)).to(self.device)

    @torch.no_grad()
    def predict(self, points=None, labels=None, boxes=None, mask_input=None, multimask_output: bool = False):
        """points [P, n, 2] in display pixels (x, y), labels [P, n], boxes [P, 4], mask_input [P, 1, 256, 256] logits ->
        (low fp32 [P, M, 256, 256], iou fp32 [P, M]) on the device, M = 3 with multimask_output else 1.  No encoder and no LLM run here."""
        self._need_image()
        if points is None and boxes is None:
            raise ValueError("predict needs points or boxes")
        m, dev = self.model, self.device
        pe, g = m.prompt_encoder, m.prompt_encoder.image_embedding_size
        with torch.cuda.device(dev):
            pts = None
            if points is not None:
                if labels is None:
                    raise ValueError("points need labels")
                xy = self._to_frame(points)
                if xy.dim() != 3:
                    raise ValueError(f"points must be [P, n, 2], got {tuple(xy.shape)}")
                pts = (xy, torch.as_tensor(labels).to(dev).to(torch.int32).reshape(xy.shape[0], xy.shape[1]))
            bx = None if boxes is None else self._to_frame(torch.as_tensor(boxes).reshape(-1, 2, 2)).reshape(-1, 4)
            sparse = pe.sparse_tokens(pts, bx)
            if mask_input is None:
                dense, cache = self.dense, self.image_cache       # the same objects on every call: the decoder's image-side cache survives
            else:
                dense, cache = pe.dense_tokens(sparse.shape[0], torch.as_tensor(mask_input).to(dev), None), None
            low, iou = m.mask_decoder.predict_masks_tokens(self.image_tokens, self.dense_pe, sparse, dense, (int(g[0]), int(g[1])), image_cache=cache,
                                                           mask_range=(1, m.mask_decoder.num_mask_tokens) if multimask_output else (0, 1))
        return low, iou

    def _finish(self, low3, **kw):
        return ops.click_finish(low3, self.frame, (self.H, self.W), self.side, self.top, self.left, self.mask_threshold, image=self.image,
                                canvas=self.labels, lut_inst=self.lut_inst, lut_cur=self.lut_cur, **kw)

    @torch.no_grad()
    def click(self, points=None, labels=None, boxes=None, mask_input=None) -> ClickResult:
        """One prompt (points [n, 2] or [1, n, 2] with labels, and / or a box [4]) -> its mask and the overlay with the mask highlighted; the mask
        becomes the current mask."""
        pts = lbl = None
        if points is not None:
            pts = torch.as_tensor(points)
            pts = pts[None] if pts.dim() == 2 else pts
            lbl = torch.as_tensor(labels).reshape(1, -1)
        low, iou = self.predict(pts, lbl, None if boxes is None else torch.as_tensor(boxes).reshape(1, 4), mask_input, multimask_output=False)
        if low.shape[0] != 1:
            raise ValueError("click takes one prompt; use predict_instances for several")
        low3 = low[:, 0].contiguous()
        with torch.cuda.device(self.device):
            mask, overlay, stats = self._finish(low3, highlight=True, want_overlay=True)
        self._current = (low3, mask[0])
        return ClickResult(mask=mask[0], overlay=overlay, iou=iou[0], area=stats[0, 0], box=stats[0, 1:5], low=low)

    @property
    def current_mask(self) -> Optional[torch.Tensor]:
        return None if self._current is None else self._current[1]

    def save_instance(self) -> torch.Tensor:
        """save_instance (app.py:692-717): the current mask becomes instance count + 1 of the canvas and is cleared; the overlay without a highlight."""
        self._need_image()
        if self._current is None:
            raise RuntimeError("no current mask: click first")
        self.count += 1
        with torch.cuda.device(self.device):
            _, overlay, _ = self._finish(self._current[0], first_id=self.count, paint=True, want_mask=False, want_overlay=True, want_stats=False)
        self._current = None
        return overlay

    @torch.no_grad()
    def predict_instances(self, points, labels, boxes=None):
        """P prompts -> instances count + 1 .. count + P of the canvas in one finish launch (a later prompt lies on top, as P successive
        save_instance calls leave it).  Returns (ids int32 [P], iou fp32 [P], area int32 [P], box int32 [P, 4]) on the device."""
        low, iou = self.predict(points, labels, boxes)
        P = low.shape[0]
        low3 = low[:, 0].contiguous()
        stats = torch.empty((P, 5), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for p0 in range(0, P, ops.CLICK_MAX_P):
                p1 = min(P, p0 + ops.CLICK_MAX_P)
                self._finish(low3[p0:p1], first_id=self.count + 1 + p0, paint=True, want_mask=False, stats=stats[p0:p1])
            ids = torch.arange(self.count + 1, self.count + 1 + P, dtype=torch.int32, device=self.device)
        self.count += P
        return ids, iou[:, 0], stats[:, 0], stats[:, 1:5]

    # -- state ----------------------------------------------------------------------------------------------------------------------------
    def render(self, highlight: bool = True) -> torch.Tensor:
        """The overlay of the present state (visualize_masks, app.py:748-772, without the click markers)."""
        self._need_image()
        with torch.cuda.device(self.device):
            show = highlight and self._current is not None
            # without paint and highlight no mask enters the overlay: the logits passed then only satisfy the kernel's P >= 1
            return self._finish(self._current[0] if show else self._no_low, highlight=show, want_mask=False, want_overlay=True, want_stats=False)[1]

    def export_labels(self) -> np.ndarray:
        """The canvas as uint16 on the host (app.py:826)."""
        self._need_image()
        if self.count > 65535:
            raise ValueError(f"{self.count} instances do not fit uint16")
        return self.labels.cpu().numpy().astype(np.uint16)

    def reset_instances(self) -> None:
        """reset_instances (app.py:864-882)."""
        self._need_image()
        self.labels.zero_()
        self.count = 0
        self._current = None

    def clear_points(self) -> None:
        """clear_points (app.py:836-861): the current mask is dropped, the instances stay."""
        self._current = None
