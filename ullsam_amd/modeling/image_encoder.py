"""SAM ViT image encoder on HIP kernels.

API mirror of modeling/image_encoder.py: ImageEncoderViT(...) ctor kwargs (:18-36), `.img_size`,
forward(x[B,3,S,S]) -> [B,out_chans,S/16,S/16]; identical state_dict keys (pos_embed, patch_embed.proj.*,
blocks.N.{norm1,attn.{qkv,proj,rel_pos_h,rel_pos_w},norm2,mlp.lin1,mlp.lin2}.*, neck.{0,1,2,3}.*).

Dataflow (per image N = g*g tokens, D = embed_dim), all activations token-major (NHWC), residual stream fp32:
  patch im2col -> GEMM(+bias +pos_embed) -> L x [ LN -> GEMM qkv -> fused (windowed|global) attention with in-kernel
  rel-pos and window pad semantics -> GEMM proj (+residual) -> LN -> GEMM lin1+GELU -> GEMM lin2 (+residual) ]
  -> GEMM 1x1 -> LN -> im2col3x3 -> GEMM -> LN.
window_partition / window_unpartition / F.pad never materialise (fused into the attention kernel's gather).
"""
from __future__ import annotations

from typing import Optional, Tuple, Type

import torch
from torch import nn

from .. import ops
from ..packing import pack_conv3x3
from .common import LayerNorm, LayerNorm2d, Linear, MLPBlock, Packed


class _Conv2dParams(Packed):
    """Parameter holder with nn.Conv2d's state_dict layout."""

    def __init__(self, cin, cout, k, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None
        nn.init.normal_(self.weight, std=(cin * k * k) ** -0.5)


class PatchEmbed(Packed):
    """image_encoder.py:364-395."""

    def __init__(self, kernel_size=(16, 16), stride=(16, 16), padding=(0, 0), in_chans=3, embed_dim=768):
        super().__init__()
        assert kernel_size == stride and padding == (0, 0), "SAM's PatchEmbed is a non-overlapping conv"
        self.patch = kernel_size[0]
        self.proj = _Conv2dParams(in_chans, embed_dim, kernel_size[0])


class Attention(Packed):
    """image_encoder.py:185-222 (parameters only; compute is fused in ImageEncoderViT.forward_tokens)."""

    def __init__(self, dim, num_heads=8, qkv_bias=True, use_rel_pos=False, rel_pos_zero_init=True, input_size=None):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = Linear(dim, dim)
        self.use_rel_pos = use_rel_pos
        if use_rel_pos:
            assert input_size is not None, "Input size must be provided if using relative positional encoding."
            self.rel_pos_h = nn.Parameter(torch.zeros(2 * input_size[0] - 1, self.head_dim))
            self.rel_pos_w = nn.Parameter(torch.zeros(2 * input_size[1] - 1, self.head_dim))

    def rel_table(self, name: str, p: torch.Tensor, size: int, dtype: torch.dtype) -> torch.Tensor:
        """The table get_rel_pos indexes (image_encoder.py:292-322) in the compute dtype: `p` itself when it has the 2 * size - 1 rows the window / grid needs, otherwise
        (:306-318, a checkpoint whose tables were trained at another resolution) its linear interpolation to that length -- F.interpolate(mode="linear"),
        align_corners=False -- computed once per weight version on the resize kernel: [hd planes] x [1 x L] resized to [1 x n] is the same one-dimensional tap arithmetic."""
        n = 2 * size - 1
        if p.shape[0] == n:
            return self.cdt(name, p, dtype)

        def make():
            t = p.detach().float().t().contiguous().reshape(p.shape[1], 1, p.shape[0])
            out, _ = ops.resize_bilinear(t, (1, n))
            return out.reshape(p.shape[1], n).t().contiguous().to(dtype)
        return self.pk(f"{name}:interp{n}", p, make)


class Block(Packed):
    """image_encoder.py:119-182."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, norm_layer=LayerNorm, act_layer=nn.GELU,
                 use_rel_pos=False, rel_pos_zero_init=True, window_size=0, input_size=None):
        super().__init__()
        self.norm1 = _make_norm(norm_layer, dim)
        self.attn = Attention(dim, num_heads, qkv_bias, use_rel_pos, rel_pos_zero_init,
                              input_size if window_size == 0 else (window_size, window_size))
        self.norm2 = _make_norm(norm_layer, dim)
        self.mlp = MLPBlock(embedding_dim=dim, mlp_dim=int(dim * mlp_ratio), act=act_layer)
        self.window_size = window_size


def _make_norm(norm_layer, dim) -> LayerNorm:
    """Accept the reference's `partial(torch.nn.LayerNorm, eps=1e-6)` (build_sam.py:72) as well as our own class."""
    probe = norm_layer(dim)
    eps = getattr(probe, "eps", 1e-5)
    return LayerNorm(dim, eps=eps)


class ImageEncoderViT(Packed):
    def __init__(self, img_size: int = 1024, patch_size: int = 16, in_chans: int = 3, embed_dim: int = 768, depth: int = 12,
                 num_heads: int = 12, mlp_ratio: float = 4.0, out_chans: int = 256, qkv_bias: bool = True,
                 norm_layer: Type[nn.Module] = nn.LayerNorm, act_layer: Type[nn.Module] = nn.GELU, use_abs_pos: bool = True,
                 use_rel_pos: bool = False, rel_pos_zero_init: bool = True, window_size: int = 0,
                 global_attn_indexes: Tuple[int, ...] = ()) -> None:
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.embed_dim, self.num_heads, self.out_chans = embed_dim, num_heads, out_chans
        self.patch_embed = PatchEmbed((patch_size, patch_size), (patch_size, patch_size), in_chans=in_chans, embed_dim=embed_dim)
        self.pos_embed: Optional[nn.Parameter] = None
        g = img_size // patch_size
        if use_abs_pos:
            self.pos_embed = nn.Parameter(torch.zeros(1, g, g, embed_dim))
        self.blocks = nn.ModuleList()
        for i in range(depth):
            self.blocks.append(Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                     norm_layer=norm_layer, act_layer=act_layer, use_rel_pos=use_rel_pos,
                                     rel_pos_zero_init=rel_pos_zero_init,
                                     window_size=window_size if i not in global_attn_indexes else 0, input_size=(g, g)))
        self.neck = nn.Sequential(_Conv2dParams(embed_dim, out_chans, 1, bias=False), LayerNorm2d(out_chans),
                                  _Conv2dParams(out_chans, out_chans, 3, bias=False), LayerNorm2d(out_chans))
        if not use_rel_pos:
            raise NotImplementedError("the HIP attention kernel implements SAM's use_rel_pos=True configuration")
        # fp8 (OCP e4m3) operands for the LayerNorm-fed linears (qkv, lin1) of a bf16 model: BASELINE.json configs[4] "fp8 MFMA ViT path".
        # Off by default (the headline metric is bf16); not part of the state_dict.  proj / lin2 stay bf16: their inputs are not
        # row-normalised, a per-row scale would have to be found in the producing kernel's epilogue.
        self.fp8_linears = False
        # diagnostic tap (the reference's blocks are nn.Modules that take forward hooks; here the blocks are fused into forward_tokens):
        # when set, called as stage_probe(block_index, x) with the fp32 residual stream [B*N, D] after every block.  Not part of the state_dict.
        self.stage_probe = None

    @property
    def compute_dtype(self) -> torch.dtype:
        return self.patch_embed.proj.weight.dtype

    # ------------------------------------------------------------------
    def forward_tokens(self, x: torch.Tensor, pixel_mean: Optional[torch.Tensor] = None,
                       pixel_std: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B,3,Hs<=S,Ws<=S] (any float dtype) -> image embedding, token-major fp32 [B, g*g, out_chans].
        pixel_mean/std (fp32 [3]) fuse Sam.preprocess (normalise, then zero-pad to S x S; sam.py:164-174)."""
        dt = self.compute_dtype
        S, p = self.img_size, self.patch_size
        g = S // p
        N = g * g
        B = x.shape[0]
        D = self.embed_dim
        cols = ops.patch_im2col(x.float().contiguous(), S, p, dt, pixel_mean, pixel_std)
        pe = self.patch_embed.proj
        wp = self.pk("patch_w", pe.weight, lambda: pe.weight.detach().reshape(D, -1).to(dt).contiguous())
        pos = None if self.pos_embed is None else self.f32("pos", self.pos_embed).reshape(N, D)
        xres = ops.gemm(cols, wp, None if pe.bias is None else self.f32("patch_b", pe.bias), residual=pos, res_row_mod=N, out_f32=True)
        fp8 = bool(self.fp8_linears) and dt == torch.bfloat16 and D % 128 == 0
        M, hp = xres.shape[0], False   # hp: this block's lin1 output travels to lin2 as K-panels
        for bi, blk in enumerate(self.blocks):
            at = blk.attn
            if fp8:
                q8, sa = ops.rows_fp8(xres, *blk.norm1.wb(), blk.norm1.eps)
                qkv = ops.gemm_fp8(q8, sa, *at.qkv.w8(), at.qkv.b())
            else:
                # (the norm writes xn as the K-panels the qkv launch reads, where that launch reads panels: ops.activation_panels_plan)
                ap, _ = ops.activation_panels_plan(M, 3 * D, D, dt, bias=at.qkv.b() is not None)
                xn = ops.norm(xres, *blk.norm1.wb(), blk.norm1.eps, dt, out_panels=ap)
                qkv = ops.gemm(xn, at.qkv.w(dt), at.qkv.b(), w_panels=at.qkv.wp(dt, M), a_panels=ap, m=M)
            qb = at.qkv.bias if at.qkv.bias is not None else torch.zeros(3 * D, device=x.device)
            n_rel = blk.window_size if blk.window_size > 0 else g
            att = ops.vit_attention(qkv, at.rel_table("rh", at.rel_pos_h, n_rel, dt), at.rel_table("rw", at.rel_pos_w, n_rel, dt), at.cdt("qb", qb, dt),
                                    B, self.num_heads, at.head_dim, g, g, blk.window_size)
            ops.gemm(att, at.proj.w(dt), at.proj.b(), residual=xres, out_f32=True, out=xres, w_panels=at.proj.wp(dt, att.shape[0]))
            if fp8:
                q8, sa = ops.rows_fp8(xres, *blk.norm2.wb(), blk.norm2.eps)
                h = ops.gemm_fp8(q8, sa, *blk.mlp.lin1.w8(), blk.mlp.lin1.b(), act=blk.mlp.act_code)
            else:
                # norm -> lin1 -> lin2 on K-panels: each producer writes what the next launch reads, where both launches agree
                w1, w2 = blk.mlp.lin1.w(dt), blk.mlp.lin2.w(dt)
                ap, cp = ops.activation_panels_plan(M, w1.shape[0], D, dt, act=blk.mlp.act_code, bias=blk.mlp.lin1.b() is not None)
                hp = cp and ops.activation_panels_plan(M, D, w2.shape[1], dt, out_f32=True, bias=blk.mlp.lin2.b() is not None, residual=True)[0]
                xn = ops.norm(xres, *blk.norm2.wb(), blk.norm2.eps, dt, out_panels=ap)
                h = ops.gemm(xn, w1, blk.mlp.lin1.b(), act=blk.mlp.act_code, w_panels=blk.mlp.lin1.wp(dt, M), a_panels=ap, out_panels=hp, m=M)
            ops.gemm(h, blk.mlp.lin2.w(dt), blk.mlp.lin2.b(), residual=xres, out_f32=True, out=xres, w_panels=blk.mlp.lin2.wp(dt, M), a_panels=hp, m=M)
            if self.stage_probe is not None:
                self.stage_probe(bi, xres)
        n0, n1, n2, n3 = self.neck[0], self.neck[1], self.neck[2], self.neck[3]
        C = self.out_chans
        w0 = self.pk("neck0", n0.weight, lambda: n0.weight.detach().reshape(C, D).to(dt).contiguous())
        y = ops.gemm(ops.cast(xres, dt), w0, out_f32=True)
        yn = ops.norm(y, *n1.wb(), n1.eps, dt)
        w2 = self.pk("neck2", n2.weight, lambda: pack_conv3x3(n2.weight.detach()).to(dt).contiguous())
        z = ops.gemm(ops.im2col3x3(yn, B, g, g, C), w2, out_f32=True)
        out = ops.norm(z, *n3.wb(), n3.eps, torch.float32)
        return out.reshape(B, N, C)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .. import training
        if training.wants_autograd(self, x):     # train() mode with gradients on (train_joint_v2.py:1015-1021): the differentiable graph
            return training.vision_forward(self, x)
        with torch.no_grad():
            B = x.shape[0]
            g = self.img_size // self.patch_size
            tok = self.forward_tokens(x)
            return ops.transpose(tok, B, g * g, self.out_chans).reshape(B, self.out_chans, g, g).to(self.compute_dtype)
