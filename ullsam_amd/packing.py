"""Host-side weight re-layouts for the HIP kernels (done once per weight version; torch is plumbing here)."""
from __future__ import annotations

import torch


def pack_w13(w1: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """[2I, K] with alternating 64-row blocks (w1 block t, w3 block t): a 128-column GEMM tile then holds the gate and
    up projections of the same 64 outputs, so silu(w1 x) * w3 x (modeling_internlm2.py:261-264) is fused in the epilogue."""
    I, K = w1.shape
    assert w3.shape == (I, K) and I % 64 == 0
    return torch.stack([w1.reshape(I // 64, 64, K), w3.reshape(I // 64, 64, K)], dim=1).reshape(2 * I, K).contiguous()


def pack_ring_panels(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 -> the same values ordered [N/16][K/32][16 rows][32 k] (the ring GEMM's K-panels, csrc/gemm_ring8p.h): weight row R,
    element k sits at ((R // 16) * (K // 32) + k // 32) * 512 + (R % 16) * 32 + k % 32, so one (16-row block, 32-deep k step) cell is one
    contiguous KiB -- what one LDS-DMA request of the kernel reads.  The result keeps the SHAPE [N, K] (callers derive FLOPs and bytes
    from it) and starts on a 1 KiB boundary; unpack_ring_panels is the inverse."""
    N, K = w.shape
    if w.dtype != torch.bfloat16 or N % 16 != 0 or K % 32 != 0:
        raise ValueError(f"pack_ring_panels: bf16 [N, K] with N % 16 == 0 and K % 32 == 0 needed, got {w.dtype} {tuple(w.shape)}")
    buf = torch.empty(N * K + 512, dtype=w.dtype, device=w.device)   # (the caching allocator aligns to 512 bytes only)
    skip = (-buf.data_ptr() % 1024) // 2
    out = buf[skip:skip + N * K].view(N, K)
    out.view(N // 16, K // 32, 16, 32).copy_(w.detach().reshape(N // 16, 16, K // 32, 32).permute(0, 2, 1, 3))
    return out


def unpack_ring_panels(p: torch.Tensor) -> torch.Tensor:
    """The row-major [N, K] weight of pack_ring_panels' output."""
    N, K = p.shape
    return p.view(N // 16, K // 32, 16, 32).permute(0, 2, 1, 3).reshape(N, K).contiguous()


def empty_activation_panels(M: int, K: int, device) -> torch.Tensor:
    """An uninitialised bf16 activation-panel buffer for M rows of K elements: shape [ceil(M / 16) * 16, K], 1 KiB aligned.  The rows past M are padding: the
    producers never write them and no consumer lets them reach a stored value, so they need no zero fill."""
    if K % 32 != 0 or M <= 0:
        raise ValueError(f"empty_activation_panels: M > 0 and K % 32 == 0 needed, got {M} x {K}")
    Mp = (M + 15) // 16 * 16
    buf = torch.empty(Mp * K + 512, dtype=torch.bfloat16, device=device)   # (the caching allocator aligns to 512 bytes only)
    skip = (-buf.data_ptr() % 1024) // 2
    return buf[skip:skip + Mp * K].view(Mp, K)


def pack_activation_panels(x: torch.Tensor) -> torch.Tensor:
    """[M, K] bf16 -> the ring GEMM's activation K-panels [ceil(M / 16)][K / 32][16 rows][32 k] (pack_ring_panels' cell, the row count rounded up to 16): row r,
    element k sits at ((r // 16) * (K // 32) + k // 32) * 512 + (r % 16) * 32 + k % 32.  The result has the shape [ceil(M / 16) * 16, K] (padding rows zero here)
    and starts on a 1 KiB boundary.  For tests and tools: in the product the producing kernel writes this layout, nothing repacks."""
    if x.dim() != 2 or x.dtype != torch.bfloat16 or x.shape[1] % 32 != 0:
        raise ValueError(f"pack_activation_panels: bf16 [M, K] with K % 32 == 0 needed, got {x.dtype} {tuple(x.shape)}")
    M, K = x.shape
    out = empty_activation_panels(M, K, x.device)
    Mp = out.shape[0]
    src = x.detach()
    if Mp != M:
        src = torch.cat([src, torch.zeros((Mp - M, K), dtype=x.dtype, device=x.device)])
    out.view(Mp // 16, K // 32, 16, 32).copy_(src.reshape(Mp // 16, 16, K // 32, 32).permute(0, 2, 1, 3))
    return out


def unpack_activation_panels(p: torch.Tensor, M: int) -> torch.Tensor:
    """The row-major [M, K] activation of a panel buffer [ceil(M / 16) * 16, K]."""
    Mp, K = p.shape
    if p.dtype != torch.bfloat16 or K % 32 != 0 or Mp != (M + 15) // 16 * 16:
        raise ValueError(f"unpack_activation_panels: a bf16 panel buffer of {M} rows needed, got {p.dtype} {tuple(p.shape)}")
    return p.view(Mp // 16, K // 32, 16, 32).permute(0, 2, 1, 3).reshape(Mp, K)[:M].contiguous()


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [Cout, Cin, 3, 3] -> [Cout, (ky, kx, Cin)] matching ullsam_im2col3x3's column order."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def pack_convT_k2s2(w: torch.Tensor, b: torch.Tensor):
    """ConvTranspose2d(k=2, s=2) weight [Cin, Cout, 2, 2] -> GEMM weight [(ky, kx, Cout), Cin] and bias tiled x4
    (stride == kernel: each output pixel gets exactly one tap, mask_decoder.py:53-59)."""
    cin, cout = w.shape[0], w.shape[1]
    return w.permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous(), b.repeat(4).contiguous()
