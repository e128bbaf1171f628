"""Thin torch-tensor wrappers over the C ABI (include/ullsam_hip.h).

torch is plumbing only: device memory, the current HIP stream, dtype bookkeeping.  Every function here launches
HIP kernels from libullsam_hip.so; none falls back to torch math.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import _lib

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SWIGLU = 0, 1, 2, 3
ACT_SPLITK_OK = 256   # ullsam_hip.h ULLSAM_ACT_SPLITK_OK
_DT = {torch.float32: 0, torch.bfloat16: 1}


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"ullsam_amd supports float32 and bfloat16 compute, got {dtype}") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=None):
    if not t.is_cuda:
        raise _lib.UllsamError(f"{name} must live on the GPU (ullsam_amd has no CPU path)")
    if t.device.index != torch.cuda.current_device():
        # kernels launch on the current device's current stream: a tensor of another GPU would be dereferenced on the wrong one
        raise _lib.UllsamError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                               f"run the call under `with torch.cuda.device({t.device.index}):`")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t


_WS = {}

# The ring GEMM's weights once more as K-panels (packing.pack_ring_panels, csrc/gemm_ring8p.h): one more bf16 copy of every weight whose launches reach a
# ring kernel (DESIGN.md section 3 has the memory bill).  ULLSAM_RING_PANELS=0 in the environment -- or set_ring_panels(False) -- is the off switch: no copy is
# built and every launch reads the row-major weight.  Same results either way, bit for bit.
_RING_PANELS = os.environ.get("ULLSAM_RING_PANELS", "1") != "0"


def set_ring_panels(on: bool) -> None:
    """Process-wide: build and use K-panel copies of the ring GEMM's weights (default), or not.  Copies already built stay in their owners' caches."""
    global _RING_PANELS
    _RING_PANELS = bool(on)
    _lib.call("ullsam_set_gemm_tuning", 4, 1 if on else 0)


def ring_panels_wanted(M: int, N: int, K: int, dtype: torch.dtype) -> bool:
    """Whether a launch of this shape reads K-panels if it is handed them: the shapes the dispatch of csrc/gemm.hip gives to a ring kernel on whole tiles
    (bf16, >= 1024 rows, N a multiple of a tile width).  A copy built for a launch that ends on another kernel costs memory only -- that kernel reads `w`."""
    return _RING_PANELS and dtype == torch.bfloat16 and M >= 1024 and K >= 256 and K % 64 == 0 and (N % 256 == 0 or N % 320 == 0)


# Activations as K-panels (packing.pack_activation_panels, csrc/gemm_ring8p.h): a bf16 activation that one ring GEMM reads is written in the panel layout by the
# kernel that produces it (a norm, or the GELU / SwiGLU epilogue of the GEMM before), so the consumer's LDS-DMA requests read whole lines.  No copy, no extra pass:
# the only memory cost is up to 15 padding rows per buffer.  ULLSAM_ACTIVATION_PANELS=0 -- or set_activation_panels(False) -- is the off switch: every launch
# then runs exactly as without the layout.  Same results either way, bit for bit.
_ACT_PANELS = os.environ.get("ULLSAM_ACTIVATION_PANELS", "1") != "0"


def set_activation_panels(on: bool) -> None:
    """Process-wide: producers write and ring GEMMs read activations as K-panels where activation_panels_plan says so (default), or never."""
    global _ACT_PANELS
    _ACT_PANELS = bool(on)
    _lib.call("ullsam_set_gemm_tuning", 5, 1 if on else 0)


def activation_panels_plan(M: int, N: int, K: int, dtype: torch.dtype, act: int = ACT_NONE, out_f32: bool = False, bias: bool = False,
                           residual: bool = False, rope: bool = False):
    """(reads A as panels, can write C as panels) for the launch gemm() / gemm_qkv_rope() (rope=True) would make with operands from empty_activation_panels:
    the answer of the library's own dispatch (ullsam_gemm_act_panels_query).  (False, False) with the switch off, outside bf16 and while autograd records
    (the training step keeps row-major activations)."""
    if not _ACT_PANELS or dtype != torch.bfloat16 or torch.is_grad_enabled():
        return False, False
    import ctypes
    ra, wc = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("ullsam_gemm_act_panels_query", dt_code(dtype), M, N, K, 4 if rope else act, int(out_f32), int(bias), int(residual), 1, 128 << 20,
              ctypes.addressof(ra), ctypes.addressof(wc))
    return bool(ra.value), bool(wc.value)


def empty_activation_panels(M: int, K: int, device) -> torch.Tensor:
    """The buffer a producer writes M rows of K bf16 elements into as panels: [ceil(M / 16) * 16, K], 1 KiB aligned (packing.empty_activation_panels)."""
    from .packing import empty_activation_panels as _e
    return _e(M, K, device)


def _gemm_workspace(device) -> torch.Tensor:
    """Caller-owned scratch for the GEMM's split-K forms (one 128 MiB buffer per device AND stream: launches on different
    streams may overlap; the ring kernel's split-K keeps up to 8 fp32 planes of the output there, e.g. 4 x 1081 x 4096 x 4 B = 71 MB)."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(128 << 20, dtype=torch.uint8, device=device)
    return ws


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         act: int = ACT_NONE, out_f32: bool = False, out: Optional[torch.Tensor] = None, res_row_mod: int = 0, splitk_ok: bool = False,
         w_panels: Optional[torch.Tensor] = None, a_panels: bool = False, out_panels: bool = False, m: Optional[int] = None) -> torch.Tensor:
    """out[M, N'] = act(a[M,K] @ w[N,K]^T + bias) + residual   (N' = N/2 for ACT_SWIGLU).  a_panels: `a` is an activation-panel buffer ([ceil(M / 16) * 16, K],
    empty_activation_panels) holding m rows; out_panels: the result is one (of M rows) -- both only where activation_panels_plan said so for this launch.  w_panels: `w` once more as packing.pack_ring_panels lays it
    out (bf16) -- the ring kernels read it instead of `w` where they can, every other kernel reads `w`; same bits either way.  splitk_ok: a launch of few tiles under a long K may run as K ranges
    summed apart (ULLSAM_ACT_SPLITK_OK, include/ullsam_hip.h): not bit-equal to the one-launch kernels -- the training step's frozen linears only."""
    _chk(a, "a"); _chk(w, "w", a.dtype)
    M, K = a.shape
    if a_panels:
        assert m is not None and a.shape[0] == (m + 15) // 16 * 16, (a.shape, m)
        M = m
    N = w.shape[0]
    assert w.shape[1] == K, (a.shape, w.shape)
    n_out = N // 2 if act == ACT_SWIGLU else N
    odt = torch.float32 if out_f32 else a.dtype
    if out_panels:
        assert out is None and not out_f32
        out = empty_activation_panels(M, n_out, a.device)
    elif out is None:
        out = torch.empty((M, n_out), dtype=odt, device=a.device)
    else:
        _chk(out, "out", odt)
        assert out.shape == (M, n_out)
    if bias is not None:
        _chk(bias, "bias", torch.float32)
    ldr = 0
    if residual is not None:
        _chk(residual, "residual", torch.float32)
        ldr = residual.shape[-1]
    ws = _gemm_workspace(a.device)
    if w_panels is not None:
        _chk(w_panels, "w_panels", torch.bfloat16)
        assert w_panels.shape == w.shape and a.dtype == torch.bfloat16, (w_panels.shape, w.shape, a.dtype)
    if a_panels or out_panels:
        _lib.call("ullsam_gemm_act_panels", dt_code(a.dtype), a.data_ptr(), K, w.data_ptr(), K, _p(w_panels), out.data_ptr(), n_out, int(out_f32),
                  _p(bias), _p(residual), ldr, res_row_mod, act | (ACT_SPLITK_OK if splitk_ok else 0), M, N, K, ws.data_ptr(), ws.numel(),
                  int(a_panels), int(out_panels), _stream())
        return out
    if w_panels is not None:
        _lib.call("ullsam_gemm_panels", dt_code(a.dtype), a.data_ptr(), K, w.data_ptr(), K, w_panels.data_ptr(), out.data_ptr(), n_out, int(out_f32),
                  _p(bias), _p(residual), ldr, res_row_mod, act | (ACT_SPLITK_OK if splitk_ok else 0), M, N, K, ws.data_ptr(), ws.numel(), _stream())
        return out
    _lib.call("ullsam_gemm", dt_code(a.dtype), a.data_ptr(), K, w.data_ptr(), K, out.data_ptr(), n_out, int(out_f32),
              _p(bias), _p(residual), ldr, res_row_mod, act | (ACT_SPLITK_OK if splitk_ok else 0), M, N, K, ws.data_ptr(), ws.numel(), _stream())
    return out


def rows_fp8(x: torch.Tensor, ln_w: Optional[torch.Tensor] = None, ln_b: Optional[torch.Tensor] = None, eps: float = 0.0):
    """(optional LayerNorm, then) per-row e4m3 quantisation: x fp32 / bf16 [rows, D] -> (uint8 [rows, D] holding e4m3 bytes, fp32 scales [rows])."""
    _chk(x, "x")
    D = x.shape[-1]
    rows = x.numel() // D
    q = torch.empty((rows, D), dtype=torch.uint8, device=x.device)
    sc = torch.empty((rows,), dtype=torch.float32, device=x.device)
    if ln_w is not None:
        _chk(ln_w, "ln_w", torch.float32); _chk(ln_b, "ln_b", torch.float32)
    _lib.call("ullsam_rows_fp8", x.data_ptr(), dt_code(x.dtype), D, q.data_ptr(), D, sc.data_ptr(), _p(ln_w), _p(ln_b), rows, D, float(eps), _stream())
    return q, sc


def gemm_fp8(a8: torch.Tensor, a_scale: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor] = None,
             act: int = ACT_NONE, out_dtype: torch.dtype = torch.bfloat16, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, N] = act((a8 @ w8^T) * a_scale[:, None] * w_scale[None, :] + bias) (+ residual); a8 / w8 are e4m3 bytes."""
    _chk(a8, "a8", torch.uint8); _chk(w8, "w8", torch.uint8); _chk(a_scale, "a_scale", torch.float32); _chk(w_scale, "w_scale", torch.float32)
    M, K = a8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and a_scale.numel() == M and w_scale.numel() == N
    out_f32 = out_dtype == torch.float32
    out = torch.empty((M, N), dtype=out_dtype, device=a8.device)
    if bias is not None:
        _chk(bias, "bias", torch.float32)
    ldr = 0
    if residual is not None:
        _chk(residual, "residual", torch.float32)
        ldr = residual.shape[-1]
    _lib.call("ullsam_gemm_fp8", a8.data_ptr(), K, a_scale.data_ptr(), w8.data_ptr(), K, w_scale.data_ptr(), out.data_ptr(), N, int(out_f32),
              _p(bias), _p(residual), ldr, act, M, N, K, _stream())
    return out


def norm(x: torch.Tensor, w: Optional[torch.Tensor], b: Optional[torch.Tensor], eps: float, out_dtype: torch.dtype,
         rms: bool = False, act: int = ACT_NONE, post_scale: Optional[torch.Tensor] = None,
         post_shift: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_panels: bool = False) -> torch.Tensor:
    """out_panels: the bf16 result as an activation-panel buffer [ceil(rows / 16) * 16, D] for the ring GEMM that reads it (activation_panels_plan said so)."""
    _chk(x, "x")
    D = x.shape[-1]
    rows = x.numel() // D
    if out_panels:
        assert out is None and out_dtype == torch.bfloat16
        out = empty_activation_panels(rows, D, x.device)
        for t in (w, b, post_scale, post_shift):
            if t is not None:
                _chk(t, "norm param", torch.float32)
        _lib.call("ullsam_norm_panels", x.data_ptr(), dt_code(x.dtype), D, out.data_ptr(), _p(w), _p(b), rows, D, float(eps), int(rms), act,
                  _p(post_scale), _p(post_shift), 1, _stream())
        return out
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    for t in (w, b, post_scale, post_shift):
        if t is not None:
            _chk(t, "norm param", torch.float32)
    _lib.call("ullsam_norm", x.data_ptr(), dt_code(x.dtype), D, out.data_ptr(), dt_code(out.dtype), D, _p(w), _p(b), rows, D,
              float(eps), int(rms), act, _p(post_scale), _p(post_shift), _stream())
    return out


def norm_fanout(x: torch.Tensor, w, b, eps: float, cdt: torch.dtype, pe: Optional[torch.Tensor], want_f32: bool = True,
                want_c: bool = True):
    """y = LayerNorm(x fp32 [rows, D]) -> (y fp32 | None, y in cdt | None, (y + pe[row % pe_rows]) in cdt | None) in one pass.
    With cdt == float32 the compute-dtype copy is the fp32 result itself."""
    _chk(x, "x", torch.float32)
    D = x.shape[-1]
    rows = x.numel() // D
    f32c = cdt == torch.float32
    out_f = torch.empty((rows, D), dtype=torch.float32, device=x.device) if (want_f32 or (f32c and want_c)) else None
    out_c = torch.empty((rows, D), dtype=cdt, device=x.device) if (want_c and not f32c) else None
    out_pe = torch.empty((rows, D), dtype=cdt, device=x.device) if pe is not None else None
    if pe is not None:
        _chk(pe, "pe", torch.float32)
    _lib.call("ullsam_norm_fanout", x.data_ptr(), rows, D, _p(w), _p(b), float(eps), _p(out_f), _p(out_c), _p(out_pe), dt_code(cdt),
              _p(pe), pe.numel() // D if pe is not None else 0, _stream())
    return out_f, (out_f if f32c else out_c), out_pe


def i2t_block(xin: torch.Tensor, res: torch.Tensor, wq: torch.Tensor, bq, ktok: torch.Tensor, vtok: torch.Tensor, wo: torch.Tensor, bo,
              lnw, lnb, eps: float, key_pe: Optional[torch.Tensor], P: int, T: int, N: int, scale: float, shared: bool, want_f32: bool = True,
              want_c: bool = True):
    """The image -> token half of a two-way block in one pass (csrc/decoder.hip i2t_block_kernel): xin = (keys + pe) bf16, res = keys fp32, both
    [P*N, 256] or [N, 256] when `shared`; ktok / vtok fp32 [P*T, 128]; -> (keys' fp32 | None, keys' bf16 | None, (keys' + pe) bf16 | None)."""
    _chk(xin, "xin", torch.bfloat16); _chk(res, "res", torch.float32); _chk(wq, "wq", torch.bfloat16); _chk(wo, "wo", torch.bfloat16)
    _chk(ktok, "ktok", torch.float32); _chk(vtok, "vtok", torch.float32)
    assert wq.shape == (128, 256) and wo.shape == (256, 128) and ktok.numel() == P * T * 128 and vtok.numel() == P * T * 128
    assert xin.numel() == (N if shared else P * N) * 256 and res.numel() == xin.numel()
    rows = P * N
    out_f = torch.empty((rows, 256), dtype=torch.float32, device=xin.device) if want_f32 else None
    out_c = torch.empty((rows, 256), dtype=torch.bfloat16, device=xin.device) if want_c else None
    out_pe = torch.empty((rows, 256), dtype=torch.bfloat16, device=xin.device) if key_pe is not None else None
    if key_pe is not None:
        _chk(key_pe, "key_pe", torch.float32)
    _lib.call("ullsam_i2t_block", xin.data_ptr(), N if shared else 0, res.data_ptr(), N if shared else 0, wq.data_ptr(), _p(bq), ktok.data_ptr(), vtok.data_ptr(),
              wo.data_ptr(), _p(bo), _p(lnw), _p(lnb), float(eps), _p(key_pe), key_pe.numel() // 256 if key_pe is not None else 0, _p(out_f), _p(out_c), _p(out_pe),
              P, T, N, float(scale), _stream())
    return out_f, out_c, out_pe


def kv_proj(xk: torch.Tensor, xv: torch.Tensor, wk: torch.Tensor, bk, wv: torch.Tensor, bv):
    """K = xk wk^T + bk, V = xv wv^T + bv in one pass over the image side (csrc/decoder.hip kv_proj_kernel): xk / xv bf16 [rows, 256], wk / wv bf16 [128, 256] -> bf16 [rows, 128] x 2."""
    _chk(xk, "xk", torch.bfloat16); _chk(xv, "xv", torch.bfloat16); _chk(wk, "wk", torch.bfloat16); _chk(wv, "wv", torch.bfloat16)
    rows = xk.numel() // 256
    assert xk.shape[-1] == 256 and xv.shape == xk.shape and wk.shape == (128, 256) and wv.shape == (128, 256)
    K = torch.empty((rows, 128), dtype=torch.bfloat16, device=xk.device)
    V = torch.empty((rows, 128), dtype=torch.bfloat16, device=xk.device)
    _lib.call("ullsam_kv_proj", xk.data_ptr(), xv.data_ptr(), wk.data_ptr(), wv.data_ptr(), _p(bk), _p(bv), K.data_ptr(), V.data_ptr(), rows, _stream())
    return K, V


def pack_mfma_rows(w: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight [out, in] (out padded to a multiple of 16 with zero rows; in % 32 == 0) -> bf16 in MFMA A-fragment order [out / 16][in / 32][lane = 16 g + m][8]:
    lane (m, g) of row tile t and k-step s holds w[16 t + m][32 s + 8 g .. + 7], and a wave's fragment load is one contiguous KiB (csrc/dectok.hip lin_tiles).
    A re-layout (reshape / permute / copy), done once per weight version by the callers' pack caches."""
    o, i = w.shape
    assert i % 32 == 0
    w = w.detach().to(torch.bfloat16)
    if o % 16:
        w = torch.cat([w, torch.zeros(((-o) % 16, i), dtype=w.dtype, device=w.device)], 0)
    return w.reshape(-1, 16, i // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def _fw(lin) -> torch.Tensor:
    return lin.pk("w:mfma_rows", lin.weight, lambda: pack_mfma_rows(lin.weight))


def dec_tok_attn(queries, qpe, sa, norm, q2_lin, P: int, T: int, skip_pe: bool, mode: int = 0):
    """Fused token-side self-attention half of a two-way block (csrc/dectok.hip): queries / qpe fp32 [P*T, 256]; sa = the block's self-attention module
    (q / k / v / out projections, bf16), norm = norm1, q2_lin = the token -> image attention's q projection.  -> (queries' fp32 [P*T, 256], q fp32 [P*T, 128]).
    mode 1: only the q projection of (queries + qpe) (the final attention): -> (queries, q)."""
    _chk(queries, "queries", torch.float32); _chk(qpe, "qpe", torch.float32)
    bf = torch.bfloat16
    q2 = torch.empty((P * T, 128), dtype=torch.float32, device=queries.device)
    if mode == 1:
        _lib.call("ullsam_dec_tok_attn", queries.data_ptr(), qpe.data_ptr(), None, q2.data_ptr(), None, None, None, None, None, None, None, None, None, None, 0.0,
                  _fw(q2_lin).data_ptr(), _p(q2_lin.b()), P, T, 0, 1, _stream())
        return queries, q2
    out = torch.empty_like(queries)
    lw, lb = norm.wb()
    _lib.call("ullsam_dec_tok_attn", queries.data_ptr(), qpe.data_ptr(), out.data_ptr(), q2.data_ptr(), _fw(sa.q_proj).data_ptr(), _p(sa.q_proj.b()),
              _fw(sa.k_proj).data_ptr(), _p(sa.k_proj.b()), _fw(sa.v_proj).data_ptr(), _p(sa.v_proj.b()), _fw(sa.out_proj).data_ptr(), _p(sa.out_proj.b()),
              lw.data_ptr(), lb.data_ptr(), float(norm.eps), _fw(q2_lin).data_ptr(), _p(q2_lin.b()), P, T, int(skip_pe), 0, _stream())
    return out, q2


def dec_tok_mlp(queries, attn, qpe, out_lin, norm2, mlp, norm3, k_lin, v_lin, P: int, T: int):
    """Fused second half of a block's token side (csrc/dectok.hip): queries fp32 [P*T, 256] (after norm1), attn fp32 [P*T, 128] (token -> image attention output) ->
    out projection + residual, norm2, MLP + residual, norm3, and the image -> token k / v projections: (queries' [P*T, 256], k [P*T, 128], v [P*T, 128]) fp32.
    mlp None: out projection + residual + norm2 only (the final attention with norm_final_attn): -> queries'."""
    _chk(queries, "queries", torch.float32); _chk(attn, "attn", torch.float32)
    bf = torch.bfloat16
    out = torch.empty_like(queries)
    w2, b2 = norm2.wb()
    if mlp is None:
        _lib.call("ullsam_dec_tok_mlp", queries.data_ptr(), attn.data_ptr(), None, out.data_ptr(), None, None, _fw(out_lin).data_ptr(), _p(out_lin.b()), w2.data_ptr(), b2.data_ptr(),
                  float(norm2.eps), None, None, None, None, None, None, 0.0, None, None, None, None, P, T, 0, _stream())
        return out
    _chk(qpe, "qpe", torch.float32)
    k = torch.empty((P * T, 128), dtype=torch.float32, device=queries.device)
    v = torch.empty_like(k)
    w3, b3 = norm3.wb()
    _lib.call("ullsam_dec_tok_mlp", queries.data_ptr(), attn.data_ptr(), qpe.data_ptr(), out.data_ptr(), k.data_ptr(), v.data_ptr(), _fw(out_lin).data_ptr(), _p(out_lin.b()),
              w2.data_ptr(), b2.data_ptr(), float(norm2.eps), _fw(mlp.lin1).data_ptr(), _p(mlp.lin1.b()), _fw(mlp.lin2).data_ptr(), _p(mlp.lin2.b()), w3.data_ptr(), b3.data_ptr(),
              float(norm3.eps), _fw(k_lin).data_ptr(), _p(k_lin.b()), _fw(v_lin).data_ptr(), _p(v_lin.b()), P, T, 1, _stream())
    return out, k, v


def dec_heads(hs: torch.Tensor, w_ptrs: torch.Tensor, b_ptrs: torch.Tensor, P: int, T: int, n_iou: int, m0: int = 0, nm: int = 4):
    """The hypernetwork MLPs of masks m0 .. m0 + nm - 1 + the IoU head in one launch (csrc/dectok.hip): hs fp32 [P, T, 256]; w_ptrs / b_ptrs = HOST int64
    tensors of 15 device pointers (chain-major, three layers each; built and kept alive by MaskDecoder).  -> (hyper fp32 [P, nm, 32], iou fp32 [P, n_iou])."""
    _chk(hs, "hs", torch.float32)
    hyper = torch.empty((P, nm, 32), dtype=torch.float32, device=hs.device)
    iou = torch.empty((P, n_iou), dtype=torch.float32, device=hs.device)
    _lib.call("ullsam_dec_heads", hs.data_ptr(), w_ptrs.data_ptr(), b_ptrs.data_ptr(), hyper.data_ptr(), iou.data_ptr(), P, T, n_iou, m0, nm, _stream())
    return hyper, iou


def concat_token_rows(prefix: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """[n0, C] fp32 shared rows in front of [P, n1, C] fp32 per-prompt rows -> [P, n0 + n1, C]: the decoder's token matrix in one launch."""
    _chk(prefix, "prefix", torch.float32); _chk(rows, "rows", torch.float32)
    P, n1, C = rows.shape
    out = torch.empty((P, prefix.shape[0] + n1, C), dtype=torch.float32, device=rows.device)
    _lib.call("ullsam_concat_token_rows", prefix.data_ptr(), prefix.shape[0], rows.data_ptr() if n1 else None, n1, out.data_ptr(), P, C, _stream())
    return out


def vit_attention(qkv: torch.Tensor, rel_h: torch.Tensor, rel_w: torch.Tensor, qkv_bias: torch.Tensor, B: int, heads: int,
                  hd: int, gh: int, gw: int, window: int) -> torch.Tensor:
    _chk(qkv, "qkv"); _chk(rel_h, "rel_h", qkv.dtype); _chk(rel_w, "rel_w", qkv.dtype); _chk(qkv_bias, "qkv_bias", qkv.dtype)
    D = heads * hd
    assert qkv.numel() == B * gh * gw * 3 * D
    n = window if window > 0 else gh
    assert rel_h.shape == (2 * n - 1, hd) and rel_w.shape[1] == hd
    out = torch.empty((B * gh * gw, D), dtype=qkv.dtype, device=qkv.device)
    _lib.call("ullsam_vit_attention", dt_code(qkv.dtype), qkv.data_ptr(), out.data_ptr(), rel_h.data_ptr(), rel_w.data_ptr(),
              qkv_bias.data_ptr(), B, heads, hd, gh, gw, window, _stream())
    return out


def causal_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, key_mask: Optional[torch.Tensor],
                     B: int, H: int, KVH: int, hd: int, Sq: int, Sk: int, q_pos0: int) -> torch.Tensor:
    _chk(q, "q"); _chk(k_cache, "k_cache", q.dtype); _chk(v_cache, "v_cache", q.dtype)
    cap = k_cache.shape[2]
    if key_mask is not None:
        _chk(key_mask, "key_mask", torch.int32)
        assert key_mask.shape == (B, Sk)
    out = torch.empty((B * Sq, H * hd), dtype=q.dtype, device=q.device)
    _lib.call("ullsam_causal_attention", dt_code(q.dtype), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
              _p(key_mask), B, H, KVH, hd, Sq, Sk, cap, q_pos0, _stream())
    return out


def naive_attention(q, k, v, B, H, KVH, hd, Sq, Sk, qs, ks, vs, os_, scale, key_mask=None, out=None):
    """Generic strided attention; qs/ks/vs/os_ = (batch, token, head) element strides."""
    _chk(q, "q"); _chk(k, "k", q.dtype); _chk(v, "v", q.dtype)
    if out is None:
        out = torch.empty((B * Sq, H * hd), dtype=q.dtype, device=q.device)
    if key_mask is not None:
        _chk(key_mask, "key_mask", torch.int32)
    _lib.call("ullsam_naive_attention", dt_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _p(key_mask),
              B, H, KVH, hd, Sq, Sk, *qs, *ks, *vs, *os_, float(scale), _stream())
    return out


def fewkeys_attention(q, k, v, B, H, hd, Sq, Sk, scale, q_shared: bool = False):
    """q fp32 [B (or 1 when q_shared), Sq, H*hd], k/v fp32 [B, Sk, H*hd] -> fp32 [B*Sq, H*hd]."""
    for t in (q, k, v):
        _chk(t, "qkv", torch.float32)
    out = torch.empty((B * Sq, H * hd), dtype=torch.float32, device=q.device)
    _lib.call("ullsam_fewkeys_attention", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, hd, Sq, Sk,
              float(scale), 0 if q_shared else Sq * H * hd, _stream())
    return out


def decode_attention(q, kc, vc, key_mask, B, H, KVH, hd, Sk):
    """q bf16 [B, H*hd] (one new token per sequence), kc / vc bf16 caches [B, KVH, cap, hd], key_mask int32 [B, Sk] | None -> bf16 [B, H*hd]."""
    _chk(q, "q", torch.bfloat16); _chk(kc, "k cache", torch.bfloat16); _chk(vc, "v cache", torch.bfloat16)
    if key_mask is not None:
        _chk(key_mask, "key_mask", torch.int32)
    G, P = H // KVH, B * KVH
    nsplit = max(1, min(32, -(-256 // P), Sk // 64))     # one workgroup per CU (8 splits at batch 4: 3.605 ms per step against 3.639 with 16, 3.63 with 4)
    ws = torch.empty((P * nsplit * G * (hd + 2),), dtype=torch.float32, device=q.device)
    out = torch.empty((B, H * hd), dtype=torch.bfloat16, device=q.device)
    _lib.call("ullsam_decode_attention", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), _p(key_mask), out.data_ptr(), B, H, KVH, hd, Sk,
              kc.shape[2], float(hd) ** -0.5, ws.data_ptr(), nsplit, _stream())
    return out


def tok2img_attention(q, k, v, P, H, hd, T, N, scale, kv_shared: bool = False):
    """q fp32 [P*T, H*hd]; k, v [P (or 1 when kv_shared) * N, H*hd] fp32 or bf16 -> fp32 [P*T, H*hd]."""
    _chk(q, "q", torch.float32); _chk(k, "k"); _chk(v, "v", k.dtype)
    C = H * hd
    nsplit = max(1, min(8, N // 128))          # independent of P: the partition of the keys (and with it the order of the softmax merge) must not depend on how many prompts share the launch
    ws = torch.empty((P * nsplit * T * (C + 2 * H),), dtype=torch.float32, device=q.device)
    out = torch.empty((P * T, C), dtype=torch.float32, device=q.device)
    bs = 0 if kv_shared else N * C
    _lib.call("ullsam_tok2img_attention", dt_code(k.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), P, H, hd, T, N,
              bs, bs, float(scale), ws.data_ptr(), nsplit, _stream())
    return out


def patch_im2col(pixels: torch.Tensor, S: int, patch: int, dtype: torch.dtype, mean=None, std=None) -> torch.Tensor:
    _chk(pixels, "pixels", torch.float32)
    B, C, Hs, Ws = pixels.shape
    g = S // patch
    out = torch.empty((B * g * g, C * patch * patch), dtype=dtype, device=pixels.device)
    _lib.call("ullsam_patch_im2col", dt_code(dtype), pixels.data_ptr(), out.data_ptr(), B, C, Hs, Ws, S, patch, _p(mean), _p(std),
              _stream())
    return out


def im2col3x3(x: torch.Tensor, B: int, H: int, W: int, C: int) -> torch.Tensor:
    _chk(x, "x")
    out = torch.empty((B * H * W, 9 * C), dtype=x.dtype, device=x.device)
    _lib.call("ullsam_im2col3x3", dt_code(x.dtype), x.data_ptr(), out.data_ptr(), B, H, W, C, _stream())
    return out


def add_cast(a: torch.Tensor, b: Optional[torch.Tensor], out_dtype: torch.dtype, rows: Optional[int] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = a[r % a_rows] + b[r % b_rows] (b optional, fp32), converted to out_dtype."""
    _chk(a, "a")
    cols = a.shape[-1]
    a_rows = a.numel() // cols
    b_rows = 0
    if b is not None:
        _chk(b, "b", torch.float32)
        assert b.shape[-1] == cols
        b_rows = b.numel() // cols
    if rows is None:
        rows = max(a_rows, b_rows)
    if out is None:
        out = torch.empty((rows, cols), dtype=out_dtype, device=a.device)
    _lib.call("ullsam_add_cast", a.data_ptr(), dt_code(a.dtype), a_rows, _p(b), b_rows, out.data_ptr(), dt_code(out.dtype), rows,
              cols, _stream())
    return out


def cast(a: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    if a.dtype == out_dtype:
        return a
    return add_cast(a.reshape(-1, a.shape[-1]), None, out_dtype).reshape(a.shape)


def transpose(x: torch.Tensor, B: int, R: int, C: int) -> torch.Tensor:
    """fp32 [B, R, C] -> [B, C, R]."""
    _chk(x, "x", torch.float32)
    out = torch.empty((B, C, R), dtype=torch.float32, device=x.device)
    _lib.call("ullsam_transpose_f32", x.data_ptr(), out.data_ptr(), B, R, C, _stream())
    return out


def transpose_to_bf16(x: torch.Tensor, pad_to: int = 1) -> torch.Tensor:
    """fp32 / bf16 [R, C] -> bf16 [C, R rounded up to pad_to] (zero filled), cast and transposed in one pass."""
    _chk(x, "x")
    R, Cn = x.shape
    Rp = -(-R // pad_to) * pad_to
    out = torch.empty((Cn, Rp), dtype=torch.bfloat16, device=x.device)
    _lib.call("ullsam_transpose_to_bf16", dt_code(x.dtype), x.data_ptr(), out.data_ptr(), R, Cn, Rp, _stream())
    return out


def cast_transpose_bf16(x: torch.Tensor, pad_to: int = 64, row_major: bool = True, colsum: bool = False):
    """fp32 [R, C] -> (bf16 [R, C] | None, bf16 [C, R rounded up to pad_to] zero filled, fp32 [C] column sums | None) in one pass over x (csrc/vit_misc.hip
    cast_transpose_bf16_kernel); C % 4 == 0 and pad_to % 4 == 0."""
    _chk(x, "x", torch.float32)
    R, Cn = x.shape
    assert Cn % 4 == 0 and pad_to % 4 == 0
    Rp = -(-R // pad_to) * pad_to
    rm = torch.empty((R, Cn), dtype=torch.bfloat16, device=x.device) if row_major else None
    xt = torch.empty((Cn, Rp), dtype=torch.bfloat16, device=x.device)
    cs = ws = None
    if colsum:
        cs = torch.empty((Cn,), dtype=torch.float32, device=x.device)
        ws = torch.empty((-(-Rp // 64) * Cn,), dtype=torch.float32, device=x.device)
    _lib.call("ullsam_cast_transpose_bf16", x.data_ptr(), _p(rm), xt.data_ptr(), _p(cs), _p(ws), R, Cn, Rp, _stream())
    return rm, xt, cs


def pixel_shuffle_ln(x_nhwc: torch.Tensor, w, b, B, H, W, C, eps, dtype) -> torch.Tensor:
    _chk(x_nhwc, "x", torch.float32)
    out = torch.empty((B * (H // 2) * (W // 2), 4 * C), dtype=dtype, device=x_nhwc.device)
    _lib.call("ullsam_pixel_shuffle_ln", dt_code(dtype), x_nhwc.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), B, H, W, C,
              float(eps), _stream())
    return out


def pixel_unshuffle(x: torch.Tensor, B, H, W, C) -> torch.Tensor:
    _chk(x, "x", torch.float32)
    out = torch.empty((B, H * W, C), dtype=torch.float32, device=x.device)
    _lib.call("ullsam_pixel_unshuffle", x.data_ptr(), out.data_ptr(), B, H, W, C, _stream())
    return out


def scan_image_tokens(ids: torch.Tensor, img_id: int):
    _chk(ids, "input_ids", torch.int64)
    B, S = ids.shape
    rank = torch.empty((B, S), dtype=torch.int32, device=ids.device)
    rng = torch.empty((B, 2), dtype=torch.int32, device=ids.device)
    _lib.call("ullsam_scan_image_tokens", ids.data_ptr(), rank.data_ptr(), rng.data_ptr(), B, S, int(img_id), _stream())
    return rank, rng


def embed_tokens(table: torch.Tensor, ids: torch.Tensor, rank: Optional[torch.Tensor], vit: Optional[torch.Tensor]) -> torch.Tensor:
    _chk(table, "tok_embeddings"); _chk(ids, "ids", torch.int64)
    B, S = ids.shape
    V, D = table.shape
    n_img = 0
    if vit is not None:
        _chk(vit, "vit_embeds", torch.float32)
        n_img = vit.numel() // (B * D)
    out = torch.empty((B * S, D), dtype=torch.float32, device=ids.device)
    _lib.call("ullsam_embed_tokens", dt_code(table.dtype), table.data_ptr(), ids.data_ptr(), _p(rank), _p(vit), out.data_ptr(), B, S, D,
              max(n_img, 1), V, _stream())
    return out


def gather_rows(x: torch.Tensor, rng: torch.Tensor, B: int, S: int, n: int) -> torch.Tensor:
    _chk(x, "x"); _chk(rng, "range", torch.int32)
    D = x.shape[-1]
    out = torch.empty((B * n, D), dtype=x.dtype, device=x.device)
    _lib.call("ullsam_gather_rows", x.data_ptr(), out.data_ptr(), rng.data_ptr(), B, S, n, D * x.element_size(), _stream())
    return out


def rope_split(qkv, k_cache, v_cache, pos, cos_tab, sin_tab, B, S, KVH, G, hd, cache_pos0) -> torch.Tensor:
    _chk(qkv, "qkv"); _chk(pos, "position_ids", torch.int32); _chk(cos_tab, "cos", torch.float32); _chk(sin_tab, "sin", torch.float32)
    q = torch.empty((B * S, KVH * G * hd), dtype=qkv.dtype, device=qkv.device)
    _lib.call("ullsam_rope_split", dt_code(qkv.dtype), qkv.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
              pos.data_ptr(), cos_tab.data_ptr(), sin_tab.data_ptr(), B, S, KVH, G, hd, k_cache.shape[2], cache_pos0, cos_tab.shape[0], _stream())
    return q


def gemm_qkv_rope(x: torch.Tensor, wqkv: torch.Tensor, bias: Optional[torch.Tensor], k_cache, v_cache, pos, cos_tab, sin_tab, B, S, KVH, G,
                  cache_pos0, w_panels: Optional[torch.Tensor] = None, a_panels: bool = False) -> torch.Tensor:
    """q = rope(split(x @ wqkv^T + bias)) with k (rotated) / v appended to the caches, all in the GEMM's epilogue (head_dim 128).
    a_panels: x is an activation-panel buffer of B * S rows (see gemm)."""
    _chk(x, "x"); _chk(wqkv, "wqkv", x.dtype); _chk(pos, "position_ids", torch.int32); _chk(cos_tab, "cos", torch.float32); _chk(sin_tab, "sin", torch.float32)
    _chk(k_cache, "k_cache", x.dtype); _chk(v_cache, "v_cache", x.dtype)
    K = x.shape[1]
    assert wqkv.shape == (KVH * (G + 2) * 128, K) and x.shape[0] == ((B * S + 15) // 16 * 16 if a_panels else B * S) and cos_tab.shape[1] == 128
    if bias is not None:
        _chk(bias, "bias", torch.float32)
    q = torch.empty((B * S, KVH * G * 128), dtype=x.dtype, device=x.device)
    ws = _gemm_workspace(x.device)
    if w_panels is not None:   # wqkv once more as packing.pack_ring_panels lays it out (see gemm)
        _chk(w_panels, "w_panels", torch.bfloat16)
        assert w_panels.shape == wqkv.shape and x.dtype == torch.bfloat16
    if a_panels:
        _lib.call("ullsam_gemm_qkv_rope_act_panels", dt_code(x.dtype), x.data_ptr(), K, wqkv.data_ptr(), K, _p(w_panels), _p(bias), B, S, K, KVH, G, pos.data_ptr(),
                  cos_tab.data_ptr(), sin_tab.data_ptr(), cos_tab.shape[0], q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.shape[2],
                  cache_pos0, ws.data_ptr(), ws.numel(), 1, _stream())
        return q
    if w_panels is not None:
        _lib.call("ullsam_gemm_qkv_rope_panels", dt_code(x.dtype), x.data_ptr(), K, wqkv.data_ptr(), K, w_panels.data_ptr(), _p(bias), B, S, K, KVH, G, pos.data_ptr(),
                  cos_tab.data_ptr(), sin_tab.data_ptr(), cos_tab.shape[0], q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.shape[2],
                  cache_pos0, ws.data_ptr(), ws.numel(), _stream())
        return q
    _lib.call("ullsam_gemm_qkv_rope", dt_code(x.dtype), x.data_ptr(), K, wqkv.data_ptr(), K, _p(bias), B, S, K, KVH, G, pos.data_ptr(),
              cos_tab.data_ptr(), sin_tab.data_ptr(), cos_tab.shape[0], q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.shape[2],
              cache_pos0, ws.data_ptr(), ws.numel(), _stream())
    return q


def decode_fusable(M: int, K: int, dtype: torch.dtype) -> bool:
    """Shapes the decode-step kernels with the fused RMSNorm prologue / RoPE epilogue take (csrc/gemm.hip launch_gemm_skinny)."""
    return dtype == torch.bfloat16 and 1 <= M <= 4 and K <= 4096 and K % 2048 == 0


def decode_w8_ok(M: int, K: int) -> bool:
    """Shapes ullsam_gemm_w8 takes: exactly those at which a bf16 ops.gemm runs on the decode-step (skinny) kernels (csrc/gemm.hip gemm_impl)."""
    return 1 <= M <= 8 and K % 512 == 0 and (4 if M <= 4 else 8) * K * 2 <= 144 * 1024


def gemm_rmsnorm(x: torch.Tensor, norm_w: torch.Tensor, eps: float, w: torch.Tensor, act: int = ACT_NONE) -> torch.Tensor:
    """act(bf16(RMSNorm(x) * norm_w) @ w^T) for a decode step's M <= 4 fp32 rows: the norm is computed while the weight stream starts."""
    _chk(x, "x", torch.float32); _chk(norm_w, "norm_w", torch.float32); _chk(w, "w", torch.bfloat16)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and decode_fusable(M, K, w.dtype), (x.shape, w.shape)
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty((M, n_out), dtype=torch.bfloat16, device=x.device)
    _lib.call("ullsam_gemm_rmsnorm", x.data_ptr(), K, norm_w.data_ptr(), float(eps), w.data_ptr(), K, out.data_ptr(), n_out, 0, None, None, 0,
              act, M, N, K, _stream())
    return out


def decode_qkv_rope(x: torch.Tensor, norm_w: Optional[torch.Tensor], eps: float, wqkv: torch.Tensor, bias: Optional[torch.Tensor], k_cache, v_cache,
                    pos, cos_tab, sin_tab, B, KVH, G, cache_pos0) -> torch.Tensor:
    """One new token per sequence (B <= 4): q = rope(split(h @ wqkv^T + bias)), k (rotated) / v appended to the caches at cache_pos0, where
    h = bf16(RMSNorm(x) * norm_w) for fp32 x (norm_w given) or x itself (bf16, norm_w None)."""
    _chk(wqkv, "wqkv", torch.bfloat16); _chk(pos, "position_ids", torch.int32); _chk(cos_tab, "cos", torch.float32); _chk(sin_tab, "sin", torch.float32)
    _chk(k_cache, "k_cache", torch.bfloat16); _chk(v_cache, "v_cache", torch.bfloat16)
    _chk(x, "x", torch.float32 if norm_w is not None else torch.bfloat16)
    K = x.shape[1]
    assert wqkv.shape == (KVH * (G + 2) * 128, K) and x.shape[0] == B and cos_tab.shape[1] == 128 and decode_fusable(B, K, wqkv.dtype)
    if bias is not None:
        _chk(bias, "bias", torch.float32)
    if norm_w is not None:
        _chk(norm_w, "norm_w", torch.float32)
    q = torch.empty((B, KVH * G * 128), dtype=torch.bfloat16, device=x.device)
    _lib.call("ullsam_decode_qkv_rope", None if norm_w is not None else x.data_ptr(), x.data_ptr() if norm_w is not None else None, K, _p(norm_w),
              float(eps), wqkv.data_ptr(), K, _p(bias), B, K, KVH, G, pos.data_ptr(), cos_tab.data_ptr(), sin_tab.data_ptr(), cos_tab.shape[0],
              q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.shape[2], cache_pos0, _stream())
    return q


def rows_fp8_pow2(w: torch.Tensor):
    """Weight-only e4m3 for the decode steps: w fp32 / bf16 [N, K] -> (uint8 [N, K] holding e4m3 bytes, fp32 scales [N]); per row the scale is the
    smallest power of two with amax / scale <= 448 (1 for a zero row), so `q * scale` of a bf16 weight is exact in bf16."""
    _chk(w, "w")
    assert w.dim() == 2 and w.shape[1] % 4 == 0, w.shape
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    sc = torch.empty((N,), dtype=torch.float32, device=w.device)
    _lib.call("ullsam_rows_fp8_pow2", w.data_ptr(), dt_code(w.dtype), K, q.data_ptr(), K, sc.data_ptr(), N, K, _stream())
    return q, sc


def gemm_w8(a: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
            act: int = ACT_NONE, out_f32: bool = False, out: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None, eps: float = 0.0) -> torch.Tensor:
    """ops.gemm / ops.gemm_rmsnorm of a decode step (M <= 8 rows) on e4m3 weights: act((h @ w8^T) * w_scale + bias) + residual, where h is the bf16 `a`
    [M, K] (norm_w None) or bf16(RMSNorm(a) * norm_w) of the fp32 rows `a` (M <= 4, K <= 4096).  Shapes the decode kernels do not take raise."""
    _chk(a, "a", torch.float32 if norm_w is not None else torch.bfloat16); _chk(w8, "w8", torch.uint8); _chk(w_scale, "w_scale", torch.float32)
    M, K = a.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and w_scale.numel() == N, (a.shape, w8.shape, w_scale.shape)
    n_out = N // 2 if act == ACT_SWIGLU else N
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty((M, n_out), dtype=odt, device=a.device)
    else:
        _chk(out, "out", odt)
        assert out.shape == (M, n_out)
    if bias is not None:
        _chk(bias, "bias", torch.float32)
        assert bias.numel() == N
    ldr = 0
    if residual is not None:
        _chk(residual, "residual", torch.float32)
        assert residual.shape == (M, n_out)
        ldr = residual.shape[-1]
    if norm_w is not None:
        _chk(norm_w, "norm_w", torch.float32)
        assert norm_w.numel() == K
    _lib.call("ullsam_gemm_w8", None if norm_w is not None else a.data_ptr(), a.data_ptr() if norm_w is not None else None, K, _p(norm_w), float(eps),
              w8.data_ptr(), K, w_scale.data_ptr(), out.data_ptr(), n_out, int(out_f32), _p(bias), _p(residual), ldr, act, M, N, K, _stream())
    return out


def decode_qkv_rope_w8(x: torch.Tensor, norm_w: Optional[torch.Tensor], eps: float, wqkv8: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor],
                       k_cache, v_cache, pos, cos_tab, sin_tab, B, KVH, G, cache_pos0) -> torch.Tensor:
    """decode_qkv_rope on e4m3 wqkv bytes [KVH * (G + 2) * 128, K] with their per-row scales."""
    _chk(wqkv8, "wqkv8", torch.uint8); _chk(w_scale, "w_scale", torch.float32); _chk(pos, "position_ids", torch.int32)
    _chk(cos_tab, "cos", torch.float32); _chk(sin_tab, "sin", torch.float32)
    _chk(k_cache, "k_cache", torch.bfloat16); _chk(v_cache, "v_cache", torch.bfloat16)
    _chk(x, "x", torch.float32 if norm_w is not None else torch.bfloat16)
    K = x.shape[1]
    N = KVH * (G + 2) * 128
    assert wqkv8.shape == (N, K) and w_scale.numel() == N and x.shape[0] == B and cos_tab.shape[1] == 128 and decode_fusable(B, K, torch.bfloat16)
    assert pos.numel() >= B and k_cache.shape[0] >= B and k_cache.shape[1] == KVH and k_cache.shape[3] == 128 and v_cache.shape == k_cache.shape
    if bias is not None:
        _chk(bias, "bias", torch.float32)
        assert bias.numel() == N
    if norm_w is not None:
        _chk(norm_w, "norm_w", torch.float32)
    q = torch.empty((B, KVH * G * 128), dtype=torch.bfloat16, device=x.device)
    _lib.call("ullsam_decode_qkv_rope_w8", None if norm_w is not None else x.data_ptr(), x.data_ptr() if norm_w is not None else None, K, _p(norm_w),
              float(eps), wqkv8.data_ptr(), K, w_scale.data_ptr(), _p(bias), B, K, KVH, G, pos.data_ptr(), cos_tab.data_ptr(), sin_tab.data_ptr(),
              cos_tab.shape[0], q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.shape[2], cache_pos0, _stream())
    return q


def argmax(logits: torch.Tensor) -> torch.Tensor:
    _chk(logits, "logits", torch.float32)
    R, V = logits.shape
    out = torch.empty((R,), dtype=torch.int64, device=logits.device)
    _lib.call("ullsam_argmax", logits.data_ptr(), out.data_ptr(), R, V, V, _stream())
    return out


def sample_topk_topp(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, seeds: torch.Tensor, step: int,
                     u: Optional[torch.Tensor] = None, return_debug: bool = False):
    """One token id per row of fp32 logits [R, V] by temperature / top-k / top-p sampling in one launch (ullsam_sample_topk_topp in the header has the
    definition).  seeds: int64 [R] on the device, read as unsigned 64-bit Philox keys (sampling.row_seeds); step: the Philox counter; u: fp32 [R] uniforms
    that replace the generator's.  return_debug: also (u used, candidate ids [R, top_k], their final probabilities [R, top_k])."""
    _chk(logits, "logits", torch.float32); _chk(seeds, "seeds", torch.int64)
    assert logits.dim() == 2, "logits must be [rows, V]"
    R, V = logits.shape
    assert seeds.numel() == R and seeds.device == logits.device
    if u is not None:
        _chk(u, "u", torch.float32)
        assert u.numel() == R and u.device == logits.device
    dev = logits.device
    out = torch.empty((R,), dtype=torch.int64, device=dev)
    u_out = cand_ids = cand_p = None
    if return_debug:
        u_out = torch.empty((R,), dtype=torch.float32, device=dev)
        cand_ids = torch.empty((R, max(int(top_k), 0)), dtype=torch.int64, device=dev)
        cand_p = torch.empty((R, max(int(top_k), 0)), dtype=torch.float32, device=dev)
    _lib.call("ullsam_sample_topk_topp", logits.data_ptr(), out.data_ptr(), R, V, V, float(temperature), int(top_k), float(top_p), seeds.data_ptr(),
              int(step) & 0xFFFFFFFFFFFFFFFF, _p(u), _p(u_out), _p(cand_ids), _p(cand_p), _stream())
    return (out, u_out, cand_ids, cand_p) if return_debug else out


def small_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], act: int = ACT_NONE,
                 res: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, "x", torch.float32); _chk(w, "w", torch.float32)
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _lib.call("ullsam_small_linear", x.data_ptr(), K, w.data_ptr(), _p(b), _p(res), N, out.data_ptr(), N, M, N, K, act, _stream())
    return out


def skinny_linear(x: torch.Tensor, wt: torch.Tensor, b: Optional[torch.Tensor], act: int = ACT_NONE,
                  res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 Linear for tens..hundreds of rows; wt = weight^T [K, N] fp32."""
    _chk(x, "x", torch.float32); _chk(wt, "wt", torch.float32)
    K, N = wt.shape
    M = x.numel() // K
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _lib.call("ullsam_skinny_linear", x.data_ptr(), K, wt.data_ptr(), _p(b), _p(res), N, out.data_ptr(), N, M, N, K, act, _stream())
    return out


def sparse_embed(coords, labels, boxes, G, emb, P, Np, pad, C, img_w, img_h) -> torch.Tensor:
    n_out = Np + pad + (2 if boxes is not None else 0)
    out = torch.empty((P, n_out, C), dtype=torch.float32, device=G.device)
    _lib.call("ullsam_sparse_embed", _p(coords), _p(labels), _p(boxes), G.data_ptr(), emb.data_ptr(), out.data_ptr(), P, Np, pad, C,
              float(img_w), float(img_h), _stream())
    return out


def dense_pe(G: torch.Tensor, H: int, W: int) -> torch.Tensor:
    C = G.shape[1] * 2
    out = torch.empty((H * W, C), dtype=torch.float32, device=G.device)
    _lib.call("ullsam_dense_pe", G.data_ptr(), out.data_ptr(), H, W, C, _stream())
    return out


def mask_downscale(masks: torch.Tensor, H: int, W: int, C: int, params) -> torch.Tensor:
    _chk(masks, "masks", torch.float32)
    P = masks.shape[0]
    c1, c2 = params[0].shape[0], params[4].shape[0]
    out = torch.empty((P, H * W, C), dtype=torch.float32, device=masks.device)
    _lib.call("ullsam_mask_downscale", masks.data_ptr(), out.data_ptr(), P, H, W, C, c1, c2, *[t.data_ptr() for t in params], _stream())
    return out


def hyper_masks(up2: torch.Tensor, hyper: torch.Tensor, NB: int, NM: int, H: int, W: int, CU: int) -> torch.Tensor:
    out = torch.empty((NB, NM, 4 * H, 4 * W), dtype=torch.float32, device=up2.device)
    _lib.call("ullsam_hyper_masks", dt_code(up2.dtype), up2.data_ptr(), hyper.data_ptr(), out.data_ptr(), NB, NM, H, W, CU, _stream())
    return out


def up1_ln_gelu(src: torch.Tensor, w0: torch.Tensor, b0, lnw, lnb, eps: float) -> torch.Tensor:
    """First transposed convolution (as Linear 256 -> 4 x 64) + LayerNorm2d + GELU in one pass (bf16): src [rows, 256], w0 [256, 256] -> bf16 [rows * 4, 64]."""
    _chk(src, "src", torch.bfloat16); _chk(w0, "w0", torch.bfloat16)
    rows = src.shape[0]
    assert src.shape == (rows, 256) and w0.shape == (256, 256)
    out = torch.empty((rows * 4, 64), dtype=torch.bfloat16, device=src.device)
    _lib.call("ullsam_up1_ln_gelu", src.data_ptr(), w0.data_ptr(), _p(b0), _p(lnw), _p(lnb), float(eps), out.data_ptr(), rows, _stream())
    return out


def up2_hyper_masks(u1: torch.Tensor, w1: torch.Tensor, b1, hyper: torch.Tensor, NB: int, NM: int, H: int, W: int) -> torch.Tensor:
    """Second transposed convolution (as Linear 64 -> 4 x 32) + GELU + hypernetwork product in one pass (bf16): u1 [NB*H*W*4, 64], w1 [128, 64], hyper fp32
    [NB, NM, 32] -> fp32 [NB, NM, 4H, 4W]."""
    _chk(u1, "u1", torch.bfloat16); _chk(w1, "w1", torch.bfloat16); _chk(hyper, "hyper", torch.float32)
    assert u1.shape == (NB * H * W * 4, 64) and w1.shape == (128, 64) and hyper.numel() == NB * NM * 32
    out = torch.empty((NB, NM, 4 * H, 4 * W), dtype=torch.float32, device=u1.device)
    _lib.call("ullsam_up2_hyper_masks", u1.data_ptr(), w1.data_ptr(), _p(b1), hyper.data_ptr(), out.data_ptr(), NB, NM, H, W, _stream())
    return out


def resize_bilinear(x: torch.Tensor, out_hw, valid_hw=None, want_float=True, threshold: Optional[float] = None):
    """x fp32 [..., IH, IW] (optionally only the top-left valid_hw region is the source image)."""
    _chk(x, "x", torch.float32)
    IHs, IWs = x.shape[-2:]
    N = x.numel() // (IHs * IWs)
    IH, IW = valid_hw if valid_hw is not None else (IHs, IWs)
    OH, OW = out_hw
    out = torch.empty(x.shape[:-2] + (OH, OW), dtype=torch.float32, device=x.device) if want_float else None
    mask = torch.empty(x.shape[:-2] + (OH, OW), dtype=torch.uint8, device=x.device) if threshold is not None else None
    _lib.call("ullsam_resize_bilinear", x.data_ptr(), IHs * IWs, IWs, IH, IW, _p(out), _p(mask), N, OH, OW,
              float(threshold if threshold is not None else 0.0), _stream())
    return out, mask


def mask_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """CalcIoU (train_joint_v2.py:683-694) over uint8 masks [N, ...] -> fp64 [N]."""
    _chk(a, "a", torch.uint8); _chk(b, "b", torch.uint8)
    N = a.shape[0]
    per = a.numel() // N
    counts = torch.empty((N, 2), dtype=torch.int64, device=a.device)
    _lib.call("ullsam_mask_iou_counts", a.data_ptr(), b.data_ptr(), counts.data_ptr(), N, per, _stream())
    c = counts.double()
    return (c[:, 0] + 1e-7) / (c[:, 1] + 1e-7)


# ---- connected regions of binary masks (csrc/regions.hip) ---------------------------------------------------------------------
REGION_CHUNK_PIXELS = 1 << 25    # pixels labelled per call: 8 masks of 2048^2
REGION_MODES = {"holes": 0, "islands": 1}


def region_chunk(h: int, w: int) -> int:
    """How many [h, w] masks one labelling call takes, so that the workspace does not grow with the number of records."""
    return max(1, min(REGION_CHUNK_PIXELS // max(h * w, 1), 4096))


def region_workspace(n: int, h: int, w: int, device) -> torch.Tensor:
    """Caller-owned scratch of `remove_small_regions`, one buffer per device and stream, grown on demand: n * (8 * h * w + 16) bytes
    = int32 labels + int32 areas (16 + 16 MiB per 2048^2 mask) + 16 bytes per mask.  With n <= region_chunk(h, w) that is at most
    8 * max(h * w, 2^25) bytes + 64 KiB (256 MiB up to 2048^2 frames), whatever the number of records."""
    need = n * (8 * h * w + 16)
    key = ("regions", str(device), torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < need:
        _WS.pop(key, None)
        ws = _WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def rle_to_mask(counts: torch.Tensor, offsets: torch.Tensor, h: int, w: int):
    """Uncompressed column-major RLEs (all counts concatenated, int32; offsets int64 [N + 1]) -> (masks uint8 [N, h, w], status int32 [N]).
    status is 1 for a record whose counts are negative or do not sum to h * w (its mask then holds the in-range part): the caller reads it."""
    _chk(counts, "counts", torch.int32); _chk(offsets, "offsets", torch.int64)
    n = offsets.numel() - 1
    assert n >= 0 and h > 0 and w > 0
    masks = torch.empty((n, h, w), dtype=torch.uint8, device=counts.device)
    status = torch.empty((n,), dtype=torch.int32, device=counts.device)
    _lib.call("ullsam_rle_to_mask", counts.data_ptr(), offsets.data_ptr(), n, h, w, masks.data_ptr(), status.data_ptr(), _stream())
    return masks, status


def label_regions(masks: torch.Tensor, background: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """masks uint8 [N, H, W] -> int32 labels [N, H, W]: the index of the raster-first pixel of the pixel's 8-connected region, -1 outside
    the working set (the non-zero pixels, or the zero pixels with background=True).  N <= 65535 (utils.amg.label_regions chunks)."""
    _chk(masks, "masks", torch.uint8)
    n, h, w = masks.shape
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.int32, device=masks.device)
    else:
        _chk(out, "out", torch.int32)
        assert out.shape == masks.shape
    _lib.call("ullsam_label_regions", masks.data_ptr(), n, h, w, int(bool(background)), out.data_ptr(), _stream())
    return out


def remove_small_regions(masks: torch.Tensor, area_thresh: int, mode: str, out: Optional[torch.Tensor] = None,
                         changed: Optional[torch.Tensor] = None):
    """One call of the region kernels over masks uint8 [N, H, W], N <= region_chunk(H, W) -> (masks uint8 [N, H, W], changed uint8 [N],
    labels int32 [N, H, W]: a view of the workspace, valid until the next call on this stream).  `out` may be `masks`."""
    _chk(masks, "masks", torch.uint8)
    n, h, w = masks.shape
    if out is None:
        out = torch.empty_like(masks)
    else:
        _chk(out, "out", torch.uint8)
        assert out.shape == masks.shape
    if changed is None:
        changed = torch.empty((n,), dtype=torch.uint8, device=masks.device)
    else:
        _chk(changed, "changed", torch.uint8)
        assert changed.numel() == n
    ws = region_workspace(n, h, w, masks.device)
    _lib.call("ullsam_remove_small_regions", masks.data_ptr(), out.data_ptr(), n, h, w, int(area_thresh), REGION_MODES[mode], ws.data_ptr(),
              ws.numel(), changed.data_ptr(), _stream())
    return out, changed, ws[:n * h * w * 4].view(torch.int32).view(n, h, w)


# ---- instance label maps and their contingency table (csrc/labels.hip) ---------------------------------------------------------
LABEL_MAX_RECORDS = 65535
OVERLAP_MAX_CELLS = 1 << 26


def _out_i32(out: Optional[torch.Tensor], shape, device, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.int32, device=device)
    _chk(out, name, torch.int32)
    assert tuple(out.shape) == tuple(shape), (name, tuple(out.shape), tuple(shape))
    return out


def _flags_i32(flags: Optional[torch.Tensor], n: int, dev) -> torch.Tensor:
    """The caller's flags int32 [n], or n zeros."""
    return torch.zeros((n,), dtype=torch.int32, device=dev) if flags is None else _out_i32(flags, (n,), dev, "flags")


def _scan_sums(n: int, chunk: int, dev) -> torch.Tensor:
    """The per-workgroup sums of a device-wide scan over n values, `chunk` to a workgroup."""
    return torch.empty((max(1, -(-n // chunk)),), dtype=torch.int32, device=dev)


def _num_ids(num, what: str) -> int:
    k = DISTANCE_INF if num is None else int(num)
    if not 0 <= k <= DISTANCE_INF:
        raise _lib.UllsamError(f"{what}: num = {num} must lie in 0..2^31 - 1")
    return k


def _volume_zhw(volume: torch.Tensor, what: str):
    _chk(volume, "volume", torch.int32)
    if volume.dim() != 3:
        raise ValueError(f"{what}: volume must be [Z, H, W], got {tuple(volume.shape)}")
    z, h, w = volume.shape
    if not all(1 <= n <= MEASURE3D_MAX_SIDE for n in (z, h, w)) or z * h * w > MEASURE3D_MAX_VOXELS:
        raise _lib.UllsamError(f"{what}: a volume of {z} x {h} x {w} (each side in 1..{MEASURE3D_MAX_SIDE}, at most 2^31 - 1 voxels)")
    return z, h, w


def rle_paint_labels(counts: torch.Tensor, offsets: torch.Tensor, rank: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None):
    """Uncompressed column-major RLEs of one [h, w] frame (counts int32 concatenated, offsets int64 [N + 1]) and their paint ranks (int32 [N],
    a permutation of 0..N-1, larger = on top) -> (raw int32 [w, h] -- TRANSPOSED -- = 1 + the largest rank covering the pixel, 0 where none does;
    status int32 [N] = 1 for a record whose counts are negative / do not sum to h * w or whose rank is out of range: the caller reads it)."""
    _chk(counts, "counts", torch.int32); _chk(offsets, "offsets", torch.int64); _chk(rank, "rank", torch.int32)
    n = offsets.numel() - 1
    assert 0 <= n <= LABEL_MAX_RECORDS and rank.numel() == n and h > 0 and w > 0
    out = _out_i32(out, (w, h), counts.device, "out")
    status = _out_i32(status, (n,), counts.device, "status")
    _lib.call("ullsam_rle_paint_labels", counts.data_ptr(), offsets.data_ptr(), rank.data_ptr(), n, h, w, out.data_ptr(), status.data_ptr(), _stream())
    return out, status


def label_stats(raw: torch.Tensor, n: int):
    """raw int32 [w, h] (transposed, labels 0..n) -> (areas int32 [n + 1], boxes int32 [n + 1, 4] inclusive XYXY) per RAW label; a label that is not
    visible has area 0 and the box (INT_MAX, INT_MAX, -1, -1)."""
    _chk(raw, "raw", torch.int32)
    w, h = raw.shape
    areas = torch.empty((n + 1,), dtype=torch.int32, device=raw.device)
    boxes = torch.empty((n + 1, 4), dtype=torch.int32, device=raw.device)
    _lib.call("ullsam_label_stats", raw.data_ptr(), n, h, w, areas.data_ptr(), boxes.data_ptr(), _stream())
    return areas, boxes


def label_compact(areas_raw: torch.Tensor, boxes_raw: torch.Tensor, rank: torch.Tensor, min_visible_area: int = 0, k_out: Optional[torch.Tensor] = None):
    """Drop the raw labels whose visible area is 0 or < min_visible_area and renumber the others 1..K in paint order -> (map int32 [N + 1]: raw -> final
    label, label_of_record int32 [N], areas int32 [N], boxes int32 [N, 4] -- their first K entries hold the final labels' -- and K int32 [1])."""
    _chk(areas_raw, "areas_raw", torch.int32); _chk(boxes_raw, "boxes_raw", torch.int32); _chk(rank, "rank", torch.int32)
    n = rank.numel()
    assert areas_raw.numel() == n + 1 and boxes_raw.numel() == 4 * (n + 1)
    dev = rank.device
    lmap = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    of_record = torch.empty((n,), dtype=torch.int32, device=dev)
    areas = torch.zeros((n,), dtype=torch.int32, device=dev)
    boxes = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    k_out = _out_i32(k_out, (1,), dev, "k_out")
    _lib.call("ullsam_label_compact", areas_raw.data_ptr(), boxes_raw.data_ptr(), rank.data_ptr(), n, int(min_visible_area), lmap.data_ptr(),
              of_record.data_ptr(), areas.data_ptr(), boxes.data_ptr(), k_out.data_ptr(), _stream())
    return lmap, of_record, areas, boxes, k_out


def label_remap(raw: torch.Tensor, lmap: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """raw int32 [w, h] (transposed), lmap int32 [N + 1] -> labels int32 [h, w] = lmap[raw[x, y]]."""
    _chk(raw, "raw", torch.int32); _chk(lmap, "lmap", torch.int32)
    w, h = raw.shape
    out = _out_i32(out, (h, w), raw.device, "out")
    _lib.call("ullsam_label_remap", raw.data_ptr(), lmap.data_ptr(), lmap.numel() - 1, h, w, out.data_ptr(), _stream())
    return out


def label_overlap(a: torch.Tensor, b: torch.Tensor, na: int, nb: int):
    """Label images a, b int32 [h, w] with ids in 0..na / 0..nb -> (T int64 [na + 1, nb + 1], T[i, j] = #{p: a[p] = i and b[p] = j}; status int32 [1] = 1
    when some id lies outside its range -- that pixel is skipped; the caller reads it)."""
    _chk(a, "a", torch.int32); _chk(b, "b", torch.int32)
    assert a.dim() == 2 and a.shape == b.shape, (a.shape, b.shape)
    na, nb = int(na), int(nb)
    if na < 0 or nb < 0 or (na + 1) * (nb + 1) > OVERLAP_MAX_CELLS:
        raise _lib.UllsamError(f"label_overlap: the table [{na + 1}, {nb + 1}] must have between 1 and 2^26 cells")
    h, w = a.shape
    table = torch.empty((na + 1, nb + 1), dtype=torch.int64, device=a.device)
    status = torch.empty((1,), dtype=torch.int32, device=a.device)
    _lib.call("ullsam_label_overlap", a.data_ptr(), b.data_ptr(), h, w, na, nb, table.data_ptr(), status.data_ptr(), _stream())
    return table, status


def resize_nearest_i32(x: torch.Tensor, out_hw, window=None) -> torch.Tensor:
    """Nearest resize of an int32 image [ih, iw] to [oh, ow] by src = min(((2 dst + 1) * in) // (2 * out), in - 1) per axis (PIL's Image.NEAREST,
    torch's nearest-exact); window = (top, left, h, w) returns only that part of the resized image."""
    _chk(x, "x", torch.int32)
    assert x.dim() == 2
    ih, iw = x.shape
    oh, ow = (int(v) for v in out_hw)
    top, left, h, w = (0, 0, oh, ow) if window is None else (int(v) for v in window)
    if not (ih > 0 and iw > 0 and oh > 0 and ow > 0 and top >= 0 and left >= 0 and h >= 0 and w >= 0 and top + h <= oh and left + w <= ow):
        raise _lib.UllsamError(f"resize_nearest_i32: window {(top, left, h, w)} does not lie inside the resized image {(oh, ow)}")
    out = torch.empty((h, w), dtype=torch.int32, device=x.device)
    _lib.call("ullsam_resize_nearest_i32", x.data_ptr(), iw, ih, iw, oh, ow, top, left, h, w, out.data_ptr(), w, _stream())
    return out


# ---- per-tile label maps stitched into one label image (csrc/mosaic.hip; utils.mosaic drives these) -----------------------------------------
MOSAIC_MAX_TILES = 65535
MOSAIC_MAX_IDS = 2 ** 31 - 2
MOSAIC_FLAGS = 4          # bad id / descriptor, table overflow, distinct pairs, (free: utils.mosaic keeps K there)


def mosaic_table_slots(max_pairs: int) -> int:
    """The pair table's capacity: the power of two >= 2 * max_pairs."""
    return 1 << max(1, (2 * int(max_pairs) - 1).bit_length())


def _mosaic_tiles(tiles: torch.Tensor, base: torch.Tensor):
    _chk(tiles, "tiles", torch.int32); _chk(base, "base", torch.int32)
    assert tiles.dim() == 3 and base.numel() == tiles.shape[0] + 1, (tuple(tiles.shape), base.numel())
    t, th, tw = tiles.shape
    if not (1 <= t <= MOSAIC_MAX_TILES and th > 0 and tw > 0):
        raise _lib.UllsamError(f"mosaic: tiles {tuple(tiles.shape)} must be [1..{MOSAIC_MAX_TILES}, th > 0, tw > 0]")
    return t, th, tw


def mosaic_seams(tiles: torch.Tensor, base: torch.Tensor, g: int, seams: torch.Tensor, max_rows: int, max_pairs: int,
                 flags: Optional[torch.Tensor] = None):
    """tiles int32 [T, th, tw], base int32 [T + 1] (exclusive sum of the tiles' id counts, g = base[T]), seams int32 [S, 9] (ullsam_hip.h) ->
    (keys int64 [slots] -- dir << 63 | g_a << 32 | g_b, 0 = empty --, counts int32 [slots], areas int32 [g + 1, 4], flags int32 [4]); the caller reads flags."""
    t, th, tw = _mosaic_tiles(tiles, base)
    _chk(seams, "seams", torch.int32)
    assert seams.dim() == 2 and seams.shape[1] == 9 and 0 <= g <= MOSAIC_MAX_IDS and max_pairs >= 1
    dev = tiles.device
    cap = mosaic_table_slots(max_pairs)
    keys = torch.empty((cap,), dtype=torch.int64, device=dev)
    counts = torch.empty((cap,), dtype=torch.int32, device=dev)
    areas = torch.empty((g + 1, 4), dtype=torch.int32, device=dev)
    flags = _out_i32(flags, (MOSAIC_FLAGS,), dev, "flags")
    _lib.call("ullsam_mosaic_seams", tiles.data_ptr(), t, th, tw, base.data_ptr(), g, seams.data_ptr(), seams.shape[0], int(max_rows), keys.data_ptr(),
              counts.data_ptr(), cap, int(max_pairs), areas.data_ptr(), flags.data_ptr(), _stream())
    return keys, counts, areas, flags


def mosaic_union(keys: torch.Tensor, g: int, counts: Optional[torch.Tensor] = None, areas: Optional[torch.Tensor] = None, iou=(1, 2),
                 flags: Optional[torch.Tensor] = None):
    """Pair keys int64 [n] (0 = none) over the ids 1..g -> (parent int32 [g + 1]: the smallest id of every id's component, flags).  With counts / areas
    (mosaic_seams' outputs) a pair merges when n > 0 and n * den >= num * (A_s + A_t - n), iou = (num, den); without them every pair merges."""
    _chk(keys, "keys", torch.int64)
    assert (counts is None) == (areas is None)
    if areas is not None:
        _chk(counts, "counts", torch.int32); _chk(areas, "areas", torch.int32)
        assert counts.numel() == keys.numel() and areas.numel() == 4 * (g + 1)
    num, den = (int(v) for v in iou)
    if not (0 < num <= den < 2 ** 31):
        raise _lib.UllsamError(f"mosaic_union: iou = (num, den) needs 0 < num <= den < 2^31, got {(num, den)}")
    parent = torch.empty((g + 1,), dtype=torch.int32, device=keys.device)
    flags = torch.zeros((MOSAIC_FLAGS,), dtype=torch.int32, device=keys.device) if flags is None else _out_i32(flags, (MOSAIC_FLAGS,), keys.device, "flags")
    _lib.call("ullsam_mosaic_union", keys.data_ptr(), _p(counts), keys.numel(), _p(areas), g, num, den, parent.data_ptr(), flags.data_ptr(), _stream())
    return parent, flags


def mosaic_stats(tiles: torch.Tensor, base: torch.Tensor, g: int, cores: torch.Tensor, max_rows: int, parent: torch.Tensor, h: int, w: int,
                 flags: Optional[torch.Tensor] = None):
    """cores int32 [T, 6] (ullsam_hip.h), parent as mosaic_union leaves it -> (areas_raw int32 [g + 1], boxes_raw int32 [g + 1, 4] inclusive XYXY) of the core
    pixels per representative."""
    t, th, tw = _mosaic_tiles(tiles, base)
    _chk(cores, "cores", torch.int32); _chk(parent, "parent", torch.int32)
    assert tuple(cores.shape) == (t, 6) and parent.numel() == g + 1
    dev = tiles.device
    areas = torch.empty((g + 1,), dtype=torch.int32, device=dev)
    boxes = torch.empty((g + 1, 4), dtype=torch.int32, device=dev)
    flags = torch.zeros((MOSAIC_FLAGS,), dtype=torch.int32, device=dev) if flags is None else _out_i32(flags, (MOSAIC_FLAGS,), dev, "flags")
    _lib.call("ullsam_mosaic_stats", tiles.data_ptr(), t, th, tw, base.data_ptr(), g, cores.data_ptr(), int(max_rows), parent.data_ptr(), int(h), int(w),
              areas.data_ptr(), boxes.data_ptr(), flags.data_ptr(), _stream())
    return areas, boxes, flags


def mosaic_compact(areas_raw: torch.Tensor, boxes_raw: torch.Tensor, parent: torch.Tensor, min_visible_area: int = 0, k_out: Optional[torch.Tensor] = None):
    """-> (label_of_global int32 [g + 1], areas int32 [g], boxes int32 [g, 4] -- their first K entries are the final labels' --, K int32 [1])."""
    _chk(areas_raw, "areas_raw", torch.int32); _chk(boxes_raw, "boxes_raw", torch.int32); _chk(parent, "parent", torch.int32)
    g = parent.numel() - 1
    assert g >= 0 and areas_raw.numel() == g + 1 and boxes_raw.numel() == 4 * (g + 1)
    dev = parent.device
    log = torch.empty((g + 1,), dtype=torch.int32, device=dev)
    areas = torch.zeros((g,), dtype=torch.int32, device=dev)
    boxes = torch.zeros((g, 4), dtype=torch.int32, device=dev)
    k_out = _out_i32(k_out, (1,), dev, "k_out")
    _lib.call("ullsam_mosaic_compact", areas_raw.data_ptr(), boxes_raw.data_ptr(), parent.data_ptr(), g, int(min_visible_area), log.data_ptr(),
              areas.data_ptr(), boxes.data_ptr(), k_out.data_ptr(), _stream())
    return log, areas, boxes, k_out


def mosaic_paste(tiles: torch.Tensor, base: torch.Tensor, g: int, cores: torch.Tensor, max_rows: int, label_of_global: torch.Tensor, h: int, w: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels int32 [h, w]: every tile's core copied through label_of_global (the cores must partition the frame: nothing else is written)."""
    t, th, tw = _mosaic_tiles(tiles, base)
    _chk(cores, "cores", torch.int32); _chk(label_of_global, "label_of_global", torch.int32)
    assert tuple(cores.shape) == (t, 6) and label_of_global.numel() == g + 1
    out = _out_i32(out, (int(h), int(w)), tiles.device, "out")
    _lib.call("ullsam_mosaic_paste", tiles.data_ptr(), t, th, tw, base.data_ptr(), g, cores.data_ptr(), int(max_rows), label_of_global.data_ptr(),
              int(h), int(w), out.data_ptr(), _stream())
    return out


# ---- per-plane label maps linked into 3-D objects (csrc/stack.hip; utils.stack drives these) --------------------------------------------------
STACK_MAX_PLANES = 65535
STACK_MAX_SIDE = 46340    # H * W < 2^31: an area, an overlap and a union fit 32 bits, n * u fits unsigned 64
STACK_FLAGS = 4           # bad id / table entry, table overflow, distinct pairs, (free: utils.stack keeps K there)


def _stack_planes(planes: torch.Tensor, base: torch.Tensor, g: int):
    _chk(planes, "planes", torch.int32); _chk(base, "base", torch.int32)
    assert planes.dim() == 3 and base.numel() == planes.shape[0] + 1, (tuple(planes.shape), base.numel())
    z, h, w = planes.shape
    if not (1 <= z <= STACK_MAX_PLANES and 1 <= h <= STACK_MAX_SIDE and 1 <= w <= STACK_MAX_SIDE):
        raise _lib.UllsamError(f"stack: planes {tuple(planes.shape)} must be [1..{STACK_MAX_PLANES}, 1..{STACK_MAX_SIDE}, 1..{STACK_MAX_SIDE}]")
    if not 0 <= int(g) <= MOSAIC_MAX_IDS:
        raise _lib.UllsamError(f"stack: g = {g} must lie in 0..2^31 - 2")
    return z, h, w


def _stack_iou(iou, what: str):
    num, den = (int(v) for v in iou)
    if not (0 < num <= den < 2 ** 31):
        raise _lib.UllsamError(f"{what}: iou = (num, den) needs 0 < num <= den < 2^31, got {(num, den)}")
    return num, den


def stack_pairs(planes: torch.Tensor, base: torch.Tensor, g: int, max_pairs: int, flags: Optional[torch.Tensor] = None):
    """planes int32 [Z, H, W], base int32 [Z + 1] (exclusive sum of the planes' id counts, g = base[Z]) -> (keys int64 [slots] -- g_a << 32 | g_b,
    a in plane z and b in plane z + 1, 0 = empty --, counts int32 [slots], areas int32 [g + 1], flags int32 [4]); the caller reads flags."""
    z, h, w = _stack_planes(planes, base, g)
    assert max_pairs >= 1
    dev = planes.device
    cap = mosaic_table_slots(max_pairs)
    keys = torch.empty((cap,), dtype=torch.int64, device=dev)
    counts = torch.empty((cap,), dtype=torch.int32, device=dev)
    areas = torch.empty((g + 1,), dtype=torch.int32, device=dev)
    flags = _out_i32(flags, (STACK_FLAGS,), dev, "flags")
    _lib.call("ullsam_stack_pairs", planes.data_ptr(), z, h, w, base.data_ptr(), int(g), keys.data_ptr(), counts.data_ptr(), cap, int(max_pairs),
              areas.data_ptr(), flags.data_ptr(), _stream())
    return keys, counts, areas, flags


def _stack_table(keys: torch.Tensor, counts: torch.Tensor, areas: torch.Tensor, g: int):
    _chk(keys, "keys", torch.int64); _chk(counts, "counts", torch.int32); _chk(areas, "areas", torch.int32)
    assert counts.numel() == keys.numel() and areas.numel() == g + 1 and 0 <= g <= MOSAIC_MAX_IDS


def stack_best(keys: torch.Tensor, counts: torch.Tensor, areas: torch.Tensor, g: int, iou=(1, 4), flags: Optional[torch.Tensor] = None):
    """A pair table (stack_pairs' outputs, or hand-made: keys int64 [n], counts int32 [n], areas int32 [g + 1]) -> (succ int32 [g + 1], pred int32
    [g + 1], flags): the partner of every id's best candidate in the next / the previous plane, 0 where it has none (ullsam_hip.h stack_best)."""
    _stack_table(keys, counts, areas, g)
    num, den = _stack_iou(iou, "stack_best")
    succ = torch.empty((g + 1,), dtype=torch.int32, device=keys.device)
    pred = torch.empty((g + 1,), dtype=torch.int32, device=keys.device)
    flags = _flags_i32(flags, STACK_FLAGS, keys.device)
    _lib.call("ullsam_stack_best", keys.data_ptr(), counts.data_ptr(), keys.numel(), areas.data_ptr(), int(g), num, den, succ.data_ptr(), pred.data_ptr(),
              flags.data_ptr(), _stream())
    return succ, pred, flags


def stack_link(g: int, succ: Optional[torch.Tensor] = None, pred: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None,
               counts: Optional[torch.Tensor] = None, areas: Optional[torch.Tensor] = None, iou=(1, 4), flags: Optional[torch.Tensor] = None):
    """-> (parent int32 [g + 1]: the smallest id of every id's object, flags).  With succ / pred (stack_best's): the mutual links, objects are chains.
    With keys / counts / areas instead: every candidate of the table is a link."""
    assert (succ is None) == (pred is None) and (succ is None) != (keys is None)
    num, den = _stack_iou(iou, "stack_link")
    if succ is not None:
        _chk(succ, "succ", torch.int32); _chk(pred, "pred", torch.int32)
        assert succ.numel() == g + 1 and pred.numel() == g + 1 and 0 <= g <= MOSAIC_MAX_IDS
        dev, n = succ.device, 0
    else:
        _stack_table(keys, counts, areas, g)
        dev, n = keys.device, keys.numel()
    parent = torch.empty((g + 1,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, STACK_FLAGS, dev)
    _lib.call("ullsam_stack_link", _p(succ), _p(pred), _p(keys), _p(counts), n, _p(areas), int(g), num, den, parent.data_ptr(), flags.data_ptr(), _stream())
    return parent, flags


def stack_stats(planes: torch.Tensor, base: torch.Tensor, g: int, parent: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """parent as stack_link leaves it -> (voxels_raw int64 [g + 1], zrange_raw int32 [g + 1, 2], boxes_raw int32 [g + 1, 4] inclusive XYXY, flags) per
    representative."""
    z, h, w = _stack_planes(planes, base, g)
    _chk(parent, "parent", torch.int32)
    assert parent.numel() == g + 1
    dev = planes.device
    voxels = torch.empty((g + 1,), dtype=torch.int64, device=dev)
    zrange = torch.empty((g + 1, 2), dtype=torch.int32, device=dev)
    boxes = torch.empty((g + 1, 4), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, STACK_FLAGS, dev)
    _lib.call("ullsam_stack_stats", planes.data_ptr(), z, h, w, base.data_ptr(), int(g), parent.data_ptr(), voxels.data_ptr(), zrange.data_ptr(),
              boxes.data_ptr(), flags.data_ptr(), _stream())
    return voxels, zrange, boxes, flags


def stack_compact(voxels_raw: torch.Tensor, zrange_raw: torch.Tensor, boxes_raw: torch.Tensor, parent: torch.Tensor, min_planes: int = 1,
                  min_volume: int = 0, k_out: Optional[torch.Tensor] = None):
    """-> (label_of_global int32 [g + 1], voxels int64 [g], zrange int32 [g, 2], boxes int32 [g, 4] -- their first K entries are the final objects' --,
    K int32 [1])."""
    _chk(voxels_raw, "voxels_raw", torch.int64); _chk(zrange_raw, "zrange_raw", torch.int32); _chk(boxes_raw, "boxes_raw", torch.int32)
    _chk(parent, "parent", torch.int32)
    g = parent.numel() - 1
    assert g >= 0 and voxels_raw.numel() == g + 1 and zrange_raw.numel() == 2 * (g + 1) and boxes_raw.numel() == 4 * (g + 1)
    dev = parent.device
    log = torch.empty((g + 1,), dtype=torch.int32, device=dev)
    voxels = torch.zeros((g,), dtype=torch.int64, device=dev)
    zrange = torch.zeros((g, 2), dtype=torch.int32, device=dev)
    boxes = torch.zeros((g, 4), dtype=torch.int32, device=dev)
    k_out = _out_i32(k_out, (1,), dev, "k_out")
    _lib.call("ullsam_stack_compact", voxels_raw.data_ptr(), zrange_raw.data_ptr(), boxes_raw.data_ptr(), parent.data_ptr(), g, int(min_planes),
              int(min_volume), log.data_ptr(), voxels.data_ptr(), zrange.data_ptr(), boxes.data_ptr(), k_out.data_ptr(), _stream())
    return log, voxels, zrange, boxes, k_out


def stack_relabel(planes: torch.Tensor, base: torch.Tensor, g: int, label_of_global: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """volume int32 [Z, H, W]: every plane copied through label_of_global."""
    z, h, w = _stack_planes(planes, base, g)
    _chk(label_of_global, "label_of_global", torch.int32)
    assert label_of_global.numel() == g + 1
    out = _out_i32(out, (z, h, w), planes.device, "out")
    _lib.call("ullsam_stack_relabel", planes.data_ptr(), z, h, w, base.data_ptr(), int(g), label_of_global.data_ptr(), out.data_ptr(), _stream())
    return out


# ---- exact squared Euclidean distance transforms of a label image (csrc/distance.hip; utils.distance drives these) ----------------------------
DISTANCE_MAX_SIDE = 32767  # every finite squared distance <= 2 * 32766^2 < 2^31 - 1
DISTANCE_INF = 2 ** 31 - 1
DISTANCE_INF16 = 0xFFFF    # "none" in the 16-bit column maps
DISTANCE_LDS_HALO = 128    # the row pass stages its segment in LDS while floor(sqrt(limit)) <= this
DISTANCE_FLAGS = 4         # bad id, (three free)
DISTANCE_MODES = {"inner": 0, "feature": 1, "expand": 2, "shrink": 3, "depth": 4}
DISTANCE_ROUTES = {"auto": 0, "lds": 1, "global": 2}


def _distance_frame(labels: torch.Tensor, num, what: str):
    _chk(labels, "labels", torch.int32)
    assert labels.dim() == 2, tuple(labels.shape)
    h, w = labels.shape
    if not (1 <= h <= DISTANCE_MAX_SIDE and 1 <= w <= DISTANCE_MAX_SIDE):
        raise _lib.UllsamError(f"{what}: a frame of {h} x {w} (each side must lie in 1..{DISTANCE_MAX_SIDE})")
    return h, w, _num_ids(num, what)


def distance_columns(labels: torch.Tensor, feature: bool = False, edge: bool = False, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """labels int32 [H, W] -> (g uint16 [H, W], nearest int32 [H, W] or None, flags): the column pass (ullsam_hip.h distance_columns).  feature False: g =
    the vertical distance of a labelled pixel to the nearest pixel of its column with another label; True: to the nearest labelled pixel, whose
    label is `nearest`.  0xFFFF = none.  flags (zeroed by the caller, or made here): [0] = a label below 0 or above num."""
    h, w, k = _distance_frame(labels, num, "distance_columns")
    dev = labels.device
    g = torch.empty((h, w), dtype=torch.uint16, device=dev)
    nearest = torch.empty((h, w), dtype=torch.int32, device=dev) if feature else None
    flags = _flags_i32(flags, DISTANCE_FLAGS, dev)
    _lib.call("ullsam_distance_columns", labels.data_ptr(), h, w, int(bool(feature)), int(bool(edge)), k, g.data_ptr(), _p(nearest), flags.data_ptr(), _stream())
    return g, nearest, flags


def distance_rows(labels: torch.Tensor, g: torch.Tensor, nearest: Optional[torch.Tensor], mode: str, edge: bool = False, limit: Optional[int] = None,
                  route: str = "auto", num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """The row pass over distance_columns' maps (ullsam_hip.h distance_rows) -> (outputs, flags).  mode "inner": D2 int32 [H, W]; "feature": (D2, nearest
    label), (INF, 0) beyond limit; "expand": the labels grown by limit = r2; "shrink": the labels whose D2 > limit = r2; "depth": best int64 [num]
    (the bits of D2 << 32 | 0xFFFFFFFF - index; distance_depth_decode reads it).  limit None = unbounded (required for "inner" and "depth").  route
    "auto" / "lds" / "global": where the scan reads from; the outputs do not depend on it."""
    h, w, k = _distance_frame(labels, num, "distance_rows")
    m = DISTANCE_MODES[mode]
    feat = mode in ("feature", "expand")
    dev = labels.device
    _chk(g, "g", torch.uint16)
    assert tuple(g.shape) == (h, w), tuple(g.shape)
    if feat:
        _chk(nearest, "nearest", torch.int32)
        assert tuple(nearest.shape) == (h, w), tuple(nearest.shape)
    lim = DISTANCE_INF if limit is None else int(limit)
    if not 0 <= lim <= DISTANCE_INF:
        raise _lib.UllsamError(f"distance_rows: limit = {limit} must lie in 0..2^31 - 1")
    flags = _flags_i32(flags, DISTANCE_FLAGS, dev)
    out0 = out1 = best = None
    if mode == "depth":
        if num is None or k > MOSAIC_MAX_IDS:
            raise _lib.UllsamError("distance_rows: the depths need num in 0..2^31 - 2")
        best = torch.empty((k,), dtype=torch.int64, device=dev)
    else:
        out0 = torch.empty((h, w), dtype=torch.int32, device=dev)
        if mode == "feature":
            out1 = torch.empty((h, w), dtype=torch.int32, device=dev)
    _lib.call("ullsam_distance_rows", labels.data_ptr(), g.data_ptr(), _p(nearest) if feat else None, h, w, m, int(bool(edge)), lim, DISTANCE_ROUTES[route], k,
              _p(out0), _p(out1), _p(best), flags.data_ptr(), _stream())
    out = best if mode == "depth" else ((out0, out1) if mode == "feature" else out0)
    return out, flags


def distance_depth_decode(best: torch.Tensor, w: int):
    """best int64 [K] (distance_rows' "depth" output) of a frame of width w -> (r2 int32 [K], xy int32 [K, 2]); an absent id: 0 and (-1, -1)."""
    _chk(best, "best", torch.int64)
    k = best.numel()
    r2 = torch.empty((k,), dtype=torch.int32, device=best.device)
    xy = torch.empty((k, 2), dtype=torch.int32, device=best.device)
    _lib.call("ullsam_distance_depth_decode", best.data_ptr(), k, int(w), r2.data_ptr(), xy.data_ptr(), _stream())
    return r2, xy


# ---- the same transforms of a label volume with anisotropic voxels (csrc/distance3d.hip; utils.distance3d drives these) -----------------------
DISTANCE3D_MAX_VOXELS = 2 ** 31 - 1   # the linear index of a voxel fits 32 bits (the depths' words)
DISTANCE3D_MAX_SPACING = 46340        # s^2 < 2^31
DISTANCE3D_MAX_B = 2 ** 31 - 2        # sum of s_a^2 (n_a - 1 + e_a)^2: every finite squared distance fits int32


def _distance3d_volume(volume: torch.Tensor, num, what: str):
    _chk(volume, "volume", torch.int32)
    assert volume.dim() == 3, tuple(volume.shape)
    z, h, w = volume.shape
    if not all(1 <= n <= DISTANCE_MAX_SIDE for n in (z, h, w)) or z * h * w > DISTANCE3D_MAX_VOXELS:
        raise _lib.UllsamError(f"{what}: a volume of {z} x {h} x {w} (each side in 1..{DISTANCE_MAX_SIDE}, at most 2^31 - 1 voxels)")
    return z, h, w, _num_ids(num, what)


def _distance3d_metric(shape, spacing, edge, what: str):
    s = tuple(int(v) for v in spacing)
    e = tuple(int(bool(v)) for v in edge)
    if len(s) != 3 or len(e) != 3 or not all(1 <= v <= DISTANCE3D_MAX_SPACING for v in s):
        raise _lib.UllsamError(f"{what}: spacing {spacing!r} and edge {edge!r} must be triples (z, y, x), each spacing in 1..{DISTANCE3D_MAX_SPACING}")
    b = sum(v * v * (n - 1 + ea) ** 2 for v, n, ea in zip(s, shape, e))
    if b > DISTANCE3D_MAX_B:
        raise _lib.UllsamError(f"{what}: the largest squared distance {b} must be at most 2^31 - 2")
    return s, e


def _distance3d_limit(limit, what: str) -> int:
    lim = DISTANCE_INF if limit is None else int(limit)
    if not 0 <= lim <= DISTANCE_INF:
        raise _lib.UllsamError(f"{what}: limit = {limit} must lie in 0..2^31 - 1")
    return lim


def distance3d_z(volume: torch.Tensor, feature: bool = False, edge: bool = False, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """volume int32 [Z, H, W] -> (g uint16 [Z, H, W], nearest int32 [Z, H, W] or None, flags): the z pass (ullsam_hip.h distance3d_z), in voxels.  feature
    False: g = the distance of a labelled voxel to the end of its run of equal label along z, plus 1 (edge: the z edge counts); True: to the nearest
    labelled voxel of the column, whose label is `nearest`.  0xFFFF = none.  flags as in distance_columns."""
    z, h, w, k = _distance3d_volume(volume, num, "distance3d_z")
    dev = volume.device
    g = torch.empty((z, h, w), dtype=torch.uint16, device=dev)
    nearest = torch.empty((z, h, w), dtype=torch.int32, device=dev) if feature else None
    flags = _flags_i32(flags, DISTANCE_FLAGS, dev)
    _lib.call("ullsam_distance3d_z", volume.data_ptr(), z, h, w, int(bool(feature)), int(bool(edge)), k, g.data_ptr(), _p(nearest), flags.data_ptr(), _stream())
    return g, nearest, flags


def distance3d_y(volume: torch.Tensor, g: torch.Tensor, nearest: Optional[torch.Tensor], spacing=(1, 1, 1), edge=(False, False, False),
                 limit: Optional[int] = None):
    """The y pass over distance3d_z's maps (ullsam_hip.h distance3d_y) -> (h int32 [Z, H, W], hlabel int32 [Z, H, W] or None).  nearest None: the
    inner distance within every (z, y) plane; otherwise the distance to the nearest labelled voxel of the plane and the smallest label that attains
    it.  spacing, edge: triples (z, y, x).  limit None = unbounded; otherwise no scan looks farther than floor(sqrt(limit) / sy) voxels."""
    z, h, w, _ = _distance3d_volume(volume, None, "distance3d_y")
    feature = nearest is not None
    s, e = _distance3d_metric((z, h, w), spacing, edge, "distance3d_y")
    lim = _distance3d_limit(limit, "distance3d_y")
    dev = volume.device
    _chk(g, "g", torch.uint16)
    assert tuple(g.shape) == (z, h, w), tuple(g.shape)
    if feature:
        _chk(nearest, "nearest", torch.int32)
        assert tuple(nearest.shape) == (z, h, w), tuple(nearest.shape)
    out = torch.empty((z, h, w), dtype=torch.int32, device=dev)
    hlabel = torch.empty((z, h, w), dtype=torch.int32, device=dev) if feature else None
    _lib.call("ullsam_distance3d_y", volume.data_ptr(), g.data_ptr(), _p(nearest), z, h, w, int(feature), *s, *e, lim, out.data_ptr(), _p(hlabel), _stream())
    return out, hlabel


def distance3d_x(volume: torch.Tensor, h: torch.Tensor, hlabel: Optional[torch.Tensor], mode: str, spacing=(1, 1, 1), edge=(False, False, False),
                 limit: Optional[int] = None, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """The x pass over distance3d_y's maps (ullsam_hip.h distance3d_x) -> (outputs, flags), with distance_rows' modes: "inner": D2 int32 [Z, H, W];
    "feature": (D2, nearest label), (INF, 0) beyond limit; "expand": the labels grown by limit = r2; "shrink": the labels whose D2 > limit = r2;
    "depth": best int64 [num] (distance3d_depth_decode reads it).  limit None = unbounded (required for "inner" and "depth")."""
    z, hh, w, k = _distance3d_volume(volume, num, "distance3d_x")
    m = DISTANCE_MODES[mode]
    feat = mode in ("feature", "expand")
    s, e = _distance3d_metric((z, hh, w), spacing, edge, "distance3d_x")
    lim = _distance3d_limit(limit, "distance3d_x")
    dev = volume.device
    _chk(h, "h", torch.int32)
    assert tuple(h.shape) == (z, hh, w), tuple(h.shape)
    if feat:
        _chk(hlabel, "hlabel", torch.int32)
        assert tuple(hlabel.shape) == (z, hh, w), tuple(hlabel.shape)
    flags = _flags_i32(flags, DISTANCE_FLAGS, dev)
    out0 = out1 = best = None
    if mode == "depth":
        if num is None or k > MOSAIC_MAX_IDS:
            raise _lib.UllsamError("distance3d_x: the depths need num in 0..2^31 - 2")
        best = torch.empty((k,), dtype=torch.int64, device=dev)
    else:
        out0 = torch.empty((z, hh, w), dtype=torch.int32, device=dev)
        if mode == "feature":
            out1 = torch.empty((z, hh, w), dtype=torch.int32, device=dev)
    _lib.call("ullsam_distance3d_x", volume.data_ptr(), h.data_ptr(), _p(hlabel) if feat else None, z, hh, w, m, *s, *e, lim, k, _p(out0), _p(out1), _p(best),
              flags.data_ptr(), _stream())
    out = best if mode == "depth" else ((out0, out1) if mode == "feature" else out0)
    return out, flags


def distance3d_depth_decode(best: torch.Tensor, h: int, w: int):
    """best int64 [K] (distance3d_x's "depth" output) of a volume of height h and width w -> (r2 int32 [K], xyz int32 [K, 3]); an absent id: 0 and
    (-1, -1, -1)."""
    _chk(best, "best", torch.int64)
    k = best.numel()
    r2 = torch.empty((k,), dtype=torch.int32, device=best.device)
    xyz = torch.empty((k, 3), dtype=torch.int32, device=best.device)
    _lib.call("ullsam_distance3d_depth_decode", best.data_ptr(), k, int(h), int(w), r2.data_ptr(), xyz.data_ptr(), _stream())
    return r2, xyz


# ---- splitting the touching objects of a label image (csrc/split.hip; utils.split drives these) -----------------------------------------------
SPLIT_FLAGS = 8            # bad id / entry, pair refused, pairs claimed, chain too long, representatives counted, list cursor, (two free)
SPLIT_MAX_DEPTH = 32767
SPLIT_ROUTES = {"auto": 0, "lds": 1, "global": 2}


def _split_map(t: torch.Tensor, name: str, like: torch.Tensor, dtype=torch.int32):
    _chk(t, name, dtype)
    assert t.numel() == like.numel(), (name, tuple(t.shape), tuple(like.shape))


def split_ascent(labels: torch.Tensor, d2: torch.Tensor, num: Optional[int] = None, route: str = "auto", flags: Optional[torch.Tensor] = None):
    """labels, d2 int32 [H, W] (d2 = distance_rows' "inner" map) -> (up int32 [H, W], flags int32 [8]): up[p] = the linear index of the pixel of
    greatest (d2, -index) among p and its 8 neighbours with p's label; p itself on the background (ullsam_hip.h split_ascent).  route "auto" /
    "lds" / "global": where the 3 x 3 neighbourhood is read from; the output does not depend on it."""
    h, w, k = _distance_frame(labels, num, "split_ascent")
    _split_map(d2, "d2", labels)
    flags = _flags_i32(flags, SPLIT_FLAGS, labels.device)
    up = torch.empty((h, w), dtype=torch.int32, device=labels.device)
    _lib.call("ullsam_split_ascent", labels.data_ptr(), d2.data_ptr(), h, w, k, SPLIT_ROUTES[route], up.data_ptr(), flags.data_ptr(), _stream())
    return up, flags


def split_flatten(up: torch.Tensor, steps: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """up int32, n pointers -> (up, flags): every pointer replaced, in place, by the root of its chain, after at most `steps` hops (default n)."""
    _chk(up, "up", torch.int32)
    n = up.numel()
    flags = _flags_i32(flags, SPLIT_FLAGS, up.device)
    _lib.call("ullsam_split_flatten", up.data_ptr(), n, n if steps is None else int(steps), flags.data_ptr(), _stream())
    return up, flags


def split_passes(labels: torch.Tensor, d2: torch.Tensor, up: torch.Tensor, max_pairs: int, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """up flattened -> (keys int64 [slots] -- smaller root << 32 | larger root, 0 = empty --, vals int32 [slots] = the pass: the largest min(d2, d2)
    over the 8-adjacent pixel pairs of one label across the two basins, flags); the caller reads flags[1], flags[2]."""
    h, w, k = _distance_frame(labels, num, "split_passes")
    _split_map(d2, "d2", labels); _split_map(up, "up", labels)
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise _lib.UllsamError(f"split_passes: max_pairs must lie in 1..2^30, got {max_pairs}")
    dev = labels.device
    cap = mosaic_table_slots(max_pairs)
    keys = torch.empty((cap,), dtype=torch.int64, device=dev)
    vals = torch.empty((cap,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SPLIT_FLAGS, dev)
    _lib.call("ullsam_split_passes", labels.data_ptr(), d2.data_ptr(), up.data_ptr(), h, w, k, keys.data_ptr(), vals.data_ptr(), cap, max_pairs,
              flags.data_ptr(), _stream())
    return keys, vals, flags


def split_round(keys: torch.Tensor, vals: torch.Tensor, labels: torch.Tensor, d2: torch.Tensor, up: torch.Tensor, min_depth: int, best: torch.Tensor,
                changed: torch.Tensor, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """One round of merging (ullsam_hip.h split_round) over a pair table (split_passes', or hand-made: keys int64 [m], vals int32 [m]) and maps of n
    pixels: up (flattened) gets up[X] = Y for every absorbed representative, changed int32 [1] is set to 1 when there is one.  best int64 [n] is
    zero on entry and on return.  -> flags; the caller flattens `up` before the next round."""
    _chk(keys, "keys", torch.int64); _chk(vals, "vals", torch.int32); _chk(labels, "labels", torch.int32)
    _split_map(d2, "d2", labels); _split_map(up, "up", labels); _split_map(best, "best", labels, torch.int64)
    _chk(changed, "changed", torch.int32)
    assert vals.numel() == keys.numel() and changed.numel() >= 1
    k = DISTANCE_INF if num is None else int(num)
    h = int(min_depth)
    if not (0 <= h <= SPLIT_MAX_DEPTH and 0 <= k <= DISTANCE_INF):
        raise _lib.UllsamError(f"split_round: min_depth = {min_depth} must lie in 0..{SPLIT_MAX_DEPTH} and num in 0..2^31 - 1")
    flags = _flags_i32(flags, SPLIT_FLAGS, labels.device)
    _lib.call("ullsam_split_round", keys.data_ptr(), vals.data_ptr(), keys.numel(), labels.data_ptr(), d2.data_ptr(), labels.numel(), k, h, best.data_ptr(),
              up.data_ptr(), changed.data_ptr(), flags.data_ptr(), _stream())
    return flags


def split_collect(labels: torch.Tensor, up: torch.Tensor, parts: Optional[int] = None, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """parts None: flags[4] += the number of representatives (up[p] = p on a labelled pixel) -> flags.  parts = that number: -> (list int64 [parts] =
    label << 32 | p of every representative, in no particular order -- sorting it gives the order of the parts --, flags)."""
    _chk(labels, "labels", torch.int32); _split_map(up, "up", labels)
    k = DISTANCE_INF if num is None else int(num)
    flags = _flags_i32(flags, SPLIT_FLAGS, labels.device)
    lst = None if parts is None else torch.zeros((int(parts),), dtype=torch.int64, device=labels.device)
    _lib.call("ullsam_split_collect", labels.data_ptr(), up.data_ptr(), labels.numel(), k, _p(lst) if lst is not None and lst.numel() else None,
              0 if lst is None else lst.numel(), flags.data_ptr(), _stream())
    return flags if parts is None else (lst, flags)


def split_relabel(parts_sorted: torch.Tensor, labels: torch.Tensor, d2: torch.Tensor, up: torch.Tensor, num: int, flags: Optional[torch.Tensor] = None):
    """parts_sorted int64 [K'] (split_collect's list, sorted), up flattened -> (out int32 [H, W], parent int32 [K'], peak_r2 int32 [K'], peak_xy
    int32 [K', 2], parts_of int32 [num], flags): part i gets id i + 1 (ullsam_hip.h split_relabel)."""
    h, w, k = _distance_frame(labels, num, "split_relabel")
    _chk(parts_sorted, "parts_sorted", torch.int64); _split_map(d2, "d2", labels); _split_map(up, "up", labels)
    if k > MOSAIC_MAX_IDS:
        raise _lib.UllsamError("split_relabel: num must lie in 0..2^31 - 2")
    dev = labels.device
    n = parts_sorted.numel()
    out = torch.empty((h, w), dtype=torch.int32, device=dev)
    newid = torch.empty((h, w), dtype=torch.int32, device=dev)
    parent = torch.empty((n,), dtype=torch.int32, device=dev)
    peak_r2 = torch.empty((n,), dtype=torch.int32, device=dev)
    peak_xy = torch.empty((n, 2), dtype=torch.int32, device=dev)
    parts_of = torch.empty((k,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SPLIT_FLAGS, dev)
    _lib.call("ullsam_split_relabel", _p(parts_sorted) if n else None, n, labels.data_ptr(), d2.data_ptr(), up.data_ptr(), h, w, k, newid.data_ptr(),
              out.data_ptr(), parent.data_ptr(), peak_r2.data_ptr(), peak_xy.data_ptr(), _p(parts_of) if k else None, flags.data_ptr(), _stream())
    return out, parent, peak_r2, peak_xy, parts_of, flags


# ---- the same split of a label volume (csrc/split3d.hip; utils.split3d drives these, with split_flatten / split_round / split_collect) ----------
SPLIT3D_MAX_VOXELS = 32767 * 32767    # the bound of the flat split entry points; every neighbour index stays inside int32


def _split3d_volume(volume: torch.Tensor, num, what: str):
    z, h, w, k = _distance3d_volume(volume, num, what)
    if z * h * w > SPLIT3D_MAX_VOXELS:
        raise _lib.UllsamError(f"{what}: a volume of {z} x {h} x {w} = {z * h * w} voxels (at most 32767^2 = {SPLIT3D_MAX_VOXELS})")
    return z, h, w, k


def split3d_ascent(volume: torch.Tensor, d2: torch.Tensor, num: Optional[int] = None, route: str = "auto", flags: Optional[torch.Tensor] = None):
    """volume, d2 int32 [Z, H, W] (d2 = distance3d_x's "inner" map) -> (up int32 [Z, H, W], flags int32 [8]): up[p] = the linear index of the voxel
    of greatest (d2, -index) among p and its 26 neighbours with p's label; p itself on the background (ullsam_hip.h split3d_ascent).  route "auto"
    / "lds" / "global": where the 3 x 3 x 3 neighbourhood is read from; the output does not depend on it."""
    z, h, w, k = _split3d_volume(volume, num, "split3d_ascent")
    _split_map(d2, "d2", volume)
    flags = _flags_i32(flags, SPLIT_FLAGS, volume.device)
    up = torch.empty((z, h, w), dtype=torch.int32, device=volume.device)
    _lib.call("ullsam_split3d_ascent", volume.data_ptr(), d2.data_ptr(), z, h, w, k, SPLIT_ROUTES[route], up.data_ptr(), flags.data_ptr(), _stream())
    return up, flags


def split3d_passes(volume: torch.Tensor, d2: torch.Tensor, up: torch.Tensor, max_pairs: int, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """up flattened -> (keys int64 [slots] -- smaller root << 32 | larger root, 0 = empty --, vals int32 [slots] = the pass: the largest min(d2, d2)
    over the 26-adjacent voxel pairs of one label across the two basins, flags): split_passes' table; the caller reads flags[1], flags[2]."""
    z, h, w, k = _split3d_volume(volume, num, "split3d_passes")
    _split_map(d2, "d2", volume); _split_map(up, "up", volume)
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise _lib.UllsamError(f"split3d_passes: max_pairs must lie in 1..2^30, got {max_pairs}")
    dev = volume.device
    cap = mosaic_table_slots(max_pairs)
    keys = torch.empty((cap,), dtype=torch.int64, device=dev)
    vals = torch.empty((cap,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SPLIT_FLAGS, dev)
    _lib.call("ullsam_split3d_passes", volume.data_ptr(), d2.data_ptr(), up.data_ptr(), z, h, w, k, keys.data_ptr(), vals.data_ptr(), cap, max_pairs,
              flags.data_ptr(), _stream())
    return keys, vals, flags


def split3d_relabel(parts_sorted: torch.Tensor, volume: torch.Tensor, d2: torch.Tensor, up: torch.Tensor, num: int, flags: Optional[torch.Tensor] = None):
    """parts_sorted int64 [K'] (split_collect's list, sorted), up flattened -> (out int32 [Z, H, W], parent int32 [K'], peak_r2 int32 [K'], peak_xyz
    int32 [K', 3], parts_of int32 [num], flags): part i gets id i + 1 (ullsam_hip.h split3d_relabel)."""
    z, h, w, k = _split3d_volume(volume, num, "split3d_relabel")
    _chk(parts_sorted, "parts_sorted", torch.int64); _split_map(d2, "d2", volume); _split_map(up, "up", volume)
    if k > MOSAIC_MAX_IDS:
        raise _lib.UllsamError("split3d_relabel: num must lie in 0..2^31 - 2")
    dev = volume.device
    n = parts_sorted.numel()
    out = torch.empty((z, h, w), dtype=torch.int32, device=dev)
    newid = torch.empty((z, h, w), dtype=torch.int32, device=dev)
    parent = torch.empty((n,), dtype=torch.int32, device=dev)
    peak_r2 = torch.empty((n,), dtype=torch.int32, device=dev)
    peak_xyz = torch.empty((n, 3), dtype=torch.int32, device=dev)
    parts_of = torch.empty((k,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SPLIT_FLAGS, dev)
    _lib.call("ullsam_split3d_relabel", _p(parts_sorted) if n else None, n, volume.data_ptr(), d2.data_ptr(), up.data_ptr(), z, h, w, k, newid.data_ptr(),
              out.data_ptr(), parent.data_ptr(), peak_r2.data_ptr(), peak_xyz.data_ptr(), _p(parts_of) if k else None, flags.data_ptr(), _stream())
    return out, parent, peak_r2, peak_xyz, parts_of, flags


# ---- skeletons of a label image (csrc/skeleton.hip; utils.skeleton drives these) ---------------------------------------------------------------
SKEL_FLAGS = 4             # bad id, a deletion at or past the limit, (two free)
SKEL_TILE_STEPS = 8        # the sub-iterations of one skel_tile launch = the depth of its halo (skeleton.hip SK_S)
SKEL_TILE = (32, 64)       # its core, rows x columns (skeleton.hip SK_CH, SK_CW)
SKEL_BLOCK = 32            # the sub-iterations the driver launches between two read-backs of the counters
SKEL_FIELDS = ("pixels", "end_points", "junctions", "isolated", "links_orth", "links_diag", "degree_sum")


def _skel_pair(src: torch.Tensor, dst: Optional[torch.Tensor], index: int, limit: int, counts: Optional[torch.Tensor], n: int, what: str):
    h, w, _ = _distance_frame(src, None, what)
    dst = _out_i32(dst, (h, w), src.device, "dst")
    if dst.data_ptr() == src.data_ptr():
        raise _lib.UllsamError(f"{what}: src and dst must be two images")
    index, limit = int(index), int(limit)
    if not (0 <= index <= DISTANCE_INF - n and 0 <= limit <= DISTANCE_INF):
        raise _lib.UllsamError(f"{what}: index = {index} and limit = {limit} must lie in 0..2^31 - 1")
    counts = torch.zeros((n,), dtype=torch.int32, device=src.device) if counts is None else _out_i32(counts, (n,), src.device, "counts")
    return h, w, dst, index, limit, counts


def skel_step(src: torch.Tensor, dst: Optional[torch.Tensor], index: int, limit: int = DISTANCE_INF, counts: Optional[torch.Tensor] = None,
              flags: Optional[torch.Tensor] = None):
    """src int32 [H, W] -> (dst int32 [H, W], counts int32 [1], flags int32 [4]): one sub-iteration of the thinning (ullsam_hip.h skel_step), number
    `index` (its parity picks the table); counts[0] += the pixels it deleted; flags[1] is raised when it deleted one and index >= limit."""
    h, w, dst, index, limit, counts = _skel_pair(src, dst, index, limit, counts, 1, "skel_step")
    flags = _flags_i32(flags, SKEL_FLAGS, src.device)
    _lib.call("ullsam_skel_step", src.data_ptr(), dst.data_ptr(), h, w, index, limit, counts.data_ptr(), flags.data_ptr(), _stream())
    return dst, counts, flags


def skel_tile(src: torch.Tensor, dst: Optional[torch.Tensor], index: int, limit: int = DISTANCE_INF, counts: Optional[torch.Tensor] = None,
              flags: Optional[torch.Tensor] = None):
    """src int32 [H, W] -> (dst int32 [H, W], counts int32 [SKEL_TILE_STEPS], flags int32 [4]): the sub-iterations index .. index +
    SKEL_TILE_STEPS - 1 in one launch on tiles staged in LDS (ullsam_hip.h skel_tile); counts[j] += the pixels sub-iteration index + j deleted."""
    h, w, dst, index, limit, counts = _skel_pair(src, dst, index, limit, counts, SKEL_TILE_STEPS, "skel_tile")
    flags = _flags_i32(flags, SKEL_FLAGS, src.device)
    _lib.call("ullsam_skel_tile", src.data_ptr(), dst.data_ptr(), h, w, index, limit, counts.data_ptr(), flags.data_ptr(), _stream())
    return dst, counts, flags


def skel_measure(skeleton: torch.Tensor, num: Optional[int], d2: Optional[torch.Tensor] = None, nodes: bool = False, flags: Optional[torch.Tensor] = None):
    """skeleton int32 [H, W] -> (table or None, nodes uint8 [H, W] or None, flags int32 [4]) (ullsam_hip.h skel_measure).  num = K: the table is a
    dict of int64 [K] per SKEL_FIELDS, with d2 (int32 [H, W]) also d2_sum int64 [K], d2_min / d2_max int32 [K]; num None: no table, every positive
    id is live.  nodes: the node classes as well."""
    h, w, k = _distance_frame(skeleton, num, "skel_measure")
    dev = skeleton.device
    flags = _flags_i32(flags, SKEL_FLAGS, dev)
    table = d2_sum = d2_min = d2_max = None
    if num is not None:
        if k > DISTANCE_INF - 1:
            raise _lib.UllsamError("skel_measure: num must lie in 0..2^31 - 2")
        table = torch.zeros((len(SKEL_FIELDS), k), dtype=torch.int64, device=dev)
        if d2 is not None:
            _split_map(d2, "d2", skeleton)
            d2_sum = torch.zeros((k,), dtype=torch.int64, device=dev)
            d2_min = torch.full((k,), DISTANCE_INF, dtype=torch.int32, device=dev)
            d2_max = torch.full((k,), -1, dtype=torch.int32, device=dev)
    out = torch.empty((h, w), dtype=torch.uint8, device=dev) if nodes else None
    with_d2 = d2_sum is not None
    some = with_d2 and k > 0                              # (an empty tensor has no address)
    _lib.call("ullsam_skel_measure", skeleton.data_ptr(), _p(d2) if some else None, h, w, k, _p(table) if table is not None and k else None,
              _p(d2_sum) if some else None, _p(d2_min) if some else None, _p(d2_max) if some else None, _p(out), flags.data_ptr(), _stream())
    res = None
    if table is not None:
        res = {f: table[i] for i, f in enumerate(SKEL_FIELDS)}
        if with_d2:
            res.update(d2_sum=d2_sum, d2_min=d2_min, d2_max=d2_max)
    return res, out, flags


# ---- outlines of a label image: polygon loops (csrc/outline.hip; utils.outline drives these) --------------------------------------------------
OUTLINE_FLAGS = 8          # bad id / index, E, corners, leaders, list cursor, parent chain too long, (two free)
OUTLINE_MAX_PIXELS = 2 ** 29
OUTLINE_CHUNK = 2048       # values per workgroup of the scan (outline.hip OL_CHUNK)


def _outline_frame(labels: torch.Tensor, what: str):
    _chk(labels, "labels", torch.int32)
    assert labels.dim() == 2, tuple(labels.shape)
    h, w = labels.shape
    if not (h >= 1 and w >= 1 and h * w < OUTLINE_MAX_PIXELS):
        raise _lib.UllsamError(f"{what}: a frame of {h} x {w} (each side at least 1, fewer than 2^29 pixels)")
    return h, w


def _outline_vec(t: torch.Tensor, name: str, n: int, dtype=torch.int32):
    _chk(t, name, dtype)
    assert t.numel() == n, (name, tuple(t.shape), n)


def outline_sides(labels: torch.Tensor, num: Optional[int] = None, flags: Optional[torch.Tensor] = None):
    """labels int32 [H, W] -> (mask uint8 [H, W], off int32 [H * W], flags int32 [8]): bit s of mask = side s (top, right, bottom, left) of a labelled
    pixel faces a pixel that is not of its label; off = the exclusive scan of popcount(mask); flags[1] = E, the edges (ullsam_hip.h outline_sides)."""
    h, w = _outline_frame(labels, "outline_sides")
    k = _num_ids(num, "outline_sides")
    dev = labels.device
    mask = torch.empty((h, w), dtype=torch.uint8, device=dev)
    off = torch.empty((h * w,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, OUTLINE_FLAGS, dev)
    _lib.call("ullsam_outline_sides", labels.data_ptr(), h, w, k, mask.data_ptr(), off.data_ptr(), _scan_sums(h * w, OUTLINE_CHUNK, dev).data_ptr(), flags.data_ptr(),
              _stream())
    return mask, off, flags


def outline_scan(vals: torch.Tensor):
    """vals uint8 [n] -> (off int32 [n] = the exclusive scan of (vals != 0), total int32 [1])."""
    _chk(vals, "vals", torch.uint8)
    n, dev = vals.numel(), vals.device
    off = torch.empty((n,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.call("ullsam_outline_scan", _p(vals) if n else None, n, _p(off) if n else None, _scan_sums(n, OUTLINE_CHUNK, dev).data_ptr(), total.data_ptr(), _stream())
    return off, total


def outline_successors(labels: torch.Tensor, mask: torch.Tensor, off: torch.Tensor, edges: int, connectivity: int = 8, flags: Optional[torch.Tensor] = None):
    """outline_sides' maps and E = edges -> (eid int32 [E] = 4 * p + s in ascending order, succ int32 [E] = the compact index of every edge's successor,
    pdir uint8 [E] = the side of every edge's predecessor, flags) (ullsam_hip.h outline_successors)."""
    h, w = _outline_frame(labels, "outline_successors")
    _outline_vec(mask, "mask", h * w, torch.uint8); _outline_vec(off, "off", h * w)
    e = int(edges)
    if connectivity not in (4, 8) or not 0 <= e <= 4 * h * w:
        raise _lib.UllsamError(f"outline_successors: connectivity = {connectivity} must be 4 or 8 and edges = {edges} lie in 0..4 H W")
    dev = labels.device
    eid = torch.empty((e,), dtype=torch.int32, device=dev)
    succ = torch.empty((e,), dtype=torch.int32, device=dev)
    pdir = torch.empty((e,), dtype=torch.uint8, device=dev)
    flags = _flags_i32(flags, OUTLINE_FLAGS, dev)
    _lib.call("ullsam_outline_successors", labels.data_ptr(), h, w, mask.data_ptr(), off.data_ptr(), e, int(connectivity), _p(eid) if e else None,
              _p(succ) if e else None, _p(pdir) if e else None, flags.data_ptr(), _stream())
    return eid, succ, pdir, flags


def outline_rank(succ: torch.Tensor, eid: torch.Tensor, pdir: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """succ, a permutation of 0..E - 1 -> (leader int32 [E] = the smallest index of every edge's cycle, rank int32 [E] = the steps from it, flags):
    ceil(log2 E) rounds of pointer doubling in ping-pong buffers (ullsam_hip.h outline_rank).  flags[3] += the leaders, flags[2] += the corners
    (the edges with pdir != eid & 3)."""
    _chk(succ, "succ", torch.int32)
    e, dev = succ.numel(), succ.device
    _outline_vec(eid, "eid", e); _outline_vec(pdir, "pdir", e, torch.uint8)
    rounds = max(e - 1, 0).bit_length()
    ws = torch.empty((2, e, 4), dtype=torch.int32, device=dev)
    leader = torch.empty((e,), dtype=torch.int32, device=dev)
    rank = torch.empty((e,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, OUTLINE_FLAGS, dev)
    _lib.call("ullsam_outline_rank", _p(succ) if e else None, _p(eid) if e else None, _p(pdir) if e else None, e, rounds, _p(ws) if e else None,
              _p(leader) if e else None, _p(rank) if e else None, flags.data_ptr(), _stream())
    return leader, rank, flags


def outline_collect(labels: torch.Tensor, eid: torch.Tensor, leader: torch.Tensor, room: int, flags: Optional[torch.Tensor] = None):
    """-> (list int64 [room], flags): label << 32 | compact index of every leader (leader[e] = e), in no particular order, from flags[4] on; the first
    flags[4] entries are written, sorting them gives the order of the loops."""
    _chk(labels, "labels", torch.int32); _chk(eid, "eid", torch.int32)
    e = eid.numel()
    _outline_vec(leader, "leader", e)
    lst = torch.zeros((int(room),), dtype=torch.int64, device=labels.device)
    flags = _flags_i32(flags, OUTLINE_FLAGS, labels.device)
    _lib.call("ullsam_outline_collect", labels.data_ptr(), labels.numel(), _p(eid) if e else None, _p(leader) if e else None, e,
              _p(lst) if lst.numel() else None, lst.numel(), flags.data_ptr(), _stream())
    return lst, flags


def outline_loops(eid: torch.Tensor, leader: torch.Tensor, loop_of: torch.Tensor, loops: int, width: int, flags: Optional[torch.Tensor] = None):
    """loop_of int32 [E]: at every leader, the index of its loop -> (edges int32 [L], area2 int64 [L], flags): the edge count and the shoelace sum of
    every loop (ullsam_hip.h outline_loops)."""
    _chk(eid, "eid", torch.int32)
    e, n, dev = eid.numel(), int(loops), eid.device
    _outline_vec(leader, "leader", e); _outline_vec(loop_of, "loop_of", e)
    edges = torch.zeros((n,), dtype=torch.int32, device=dev)
    area2 = torch.zeros((n,), dtype=torch.int64, device=dev)
    flags = _flags_i32(flags, OUTLINE_FLAGS, dev)
    if e and n:
        _lib.call("ullsam_outline_loops", eid.data_ptr(), leader.data_ptr(), loop_of.data_ptr(), e, n, int(width), edges.data_ptr(), area2.data_ptr(),
                  flags.data_ptr(), _stream())
    return edges, area2, flags


def outline_order(eid: torch.Tensor, pdir: torch.Tensor, leader: torch.Tensor, rank: torch.Tensor, loop_of: torch.Tensor, estart: torch.Tensor,
                  flags: Optional[torch.Tensor] = None):
    """estart int32 [L] = the exclusive scan of the loops' edge counts -> (reid int32 [E], corner uint8 [E], flags): edge e's id and whether it is a
    corner, at slot estart[its loop] + rank[e] -- the edges loop after loop, each loop in travel order from its leader."""
    _chk(eid, "eid", torch.int32); _chk(estart, "estart", torch.int32)
    e, dev = eid.numel(), eid.device
    _outline_vec(pdir, "pdir", e, torch.uint8); _outline_vec(leader, "leader", e); _outline_vec(rank, "rank", e); _outline_vec(loop_of, "loop_of", e)
    reid = torch.zeros((e,), dtype=torch.int32, device=dev)
    corner = torch.zeros((e,), dtype=torch.uint8, device=dev)
    flags = _flags_i32(flags, OUTLINE_FLAGS, dev)
    if e:
        _lib.call("ullsam_outline_order", eid.data_ptr(), pdir.data_ptr(), leader.data_ptr(), rank.data_ptr(), loop_of.data_ptr(), _p(estart) if estart.numel() else None,
                  e, estart.numel(), reid.data_ptr(), corner.data_ptr(), flags.data_ptr(), _stream())
    return reid, corner, flags


def outline_vertices(reid: torch.Tensor, corner: torch.Tensor, coff: torch.Tensor, count: int, width: int) -> torch.Tensor:
    """vertices int32 [count, 2]: the tail (x, y) of every corner edge of outline_order's copy, at coff = outline_scan(corner)."""
    _chk(reid, "reid", torch.int32)
    e, n = reid.numel(), int(count)
    _outline_vec(corner, "corner", e, torch.uint8); _outline_vec(coff, "coff", e)
    vertices = torch.zeros((n, 2), dtype=torch.int32, device=reid.device)
    if e and n:
        _lib.call("ullsam_outline_vertices", reid.data_ptr(), corner.data_ptr(), coff.data_ptr(), e, int(width), n, vertices.data_ptr(), _stream())
    return vertices


def outline_parents(labels: torch.Tensor, mask: torch.Tensor, off: torch.Tensor, eid: torch.Tensor, leader: torch.Tensor, loop_of: torch.Tensor,
                    lead: torch.Tensor, area2: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """lead int32 [L] = the compact index of every loop's leader, area2 int64 [L] -> (parent int32 [L], flags): an outer loop is its own parent; a hole
    walks left from its leader's pixel and chases (ullsam_hip.h outline_parents)."""
    h, w = _outline_frame(labels, "outline_parents")
    _outline_vec(mask, "mask", h * w, torch.uint8); _outline_vec(off, "off", h * w)
    _chk(eid, "eid", torch.int32); _chk(lead, "lead", torch.int32)
    e, n, dev = eid.numel(), lead.numel(), labels.device
    _outline_vec(leader, "leader", e); _outline_vec(loop_of, "loop_of", e); _outline_vec(area2, "area2", n, torch.int64)
    parent = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, OUTLINE_FLAGS, dev)
    if n:
        _lib.call("ullsam_outline_parents", labels.data_ptr(), h, w, mask.data_ptr(), off.data_ptr(), eid.data_ptr(), leader.data_ptr(), loop_of.data_ptr(),
                  lead.data_ptr(), area2.data_ptr(), e, n, parent.data_ptr(), flags.data_ptr(), _stream())
    return parent, flags


# ---- simplified outlines: Douglas-Peucker on the loops, shared borders watertight (csrc/simplify.hip; utils.simplify drives these) ------------
SIMPLIFY_FLAGS = 4         # an index left its table, (three free)
SIMPLIFY_MAX_SIDE = 32767
SIMPLIFY_MAX_T = 255 * 256


def _simplify_frame(h: int, w: int, what: str):
    h, w = int(h), int(w)
    if not (1 <= h <= SIMPLIFY_MAX_SIDE and 1 <= w <= SIMPLIFY_MAX_SIDE and h * w < OUTLINE_MAX_PIXELS):
        raise _lib.UllsamError(f"{what}: a frame of {h} x {w} (each side in 1..32767, fewer than 2^29 pixels)")
    return h, w


def simplify_flags(labels: torch.Tensor, reid: torch.Tensor, corner: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """labels int32 [H, W] and outline_order's copy -> (cand uint8 [E], flags): bit 0 = the tail of slot i is a candidate (a corner or a fixed point),
    bit 1 = it is a fixed point (ullsam_hip.h simplify_flags)."""
    _chk(labels, "labels", torch.int32); _chk(reid, "reid", torch.int32)
    assert labels.dim() == 2, tuple(labels.shape)
    h, w = _simplify_frame(*labels.shape, "simplify_flags")
    e, dev = reid.numel(), labels.device
    _outline_vec(corner, "corner", e, torch.uint8)
    cand = torch.zeros((e,), dtype=torch.uint8, device=dev)
    flags = _flags_i32(flags, SIMPLIFY_FLAGS, dev)
    if e:
        _lib.call("ullsam_simplify_flags", labels.data_ptr(), h, w, reid.data_ptr(), corner.data_ptr(), e, cand.data_ptr(), flags.data_ptr(), _stream())
    return cand, flags


def simplify_candidates(reid: torch.Tensor, cand: torch.Tensor, coff: torch.Tensor, estart: torch.Tensor, count: int, h: int, w: int,
                        flags: Optional[torch.Tensor] = None):
    """coff = outline_scan(cand), C = count -> (cxy int32 [C] = y << 16 | x, cloop int32 [C], kept uint8 [C] = the fixed ones, nfixed int32 [L], flags):
    the candidates in order, loop after loop, each in travel order (ullsam_hip.h simplify_candidates)."""
    _chk(reid, "reid", torch.int32); _chk(estart, "estart", torch.int32)
    h, w = _simplify_frame(h, w, "simplify_candidates")
    e, n, c, dev = reid.numel(), estart.numel(), int(count), reid.device
    _outline_vec(cand, "cand", e, torch.uint8); _outline_vec(coff, "coff", e)
    if not 0 <= n <= c <= e:
        raise _lib.UllsamError(f"simplify_candidates: {n} loops, {c} candidates, {e} edges (need L <= C <= E)")
    cxy = torch.zeros((c,), dtype=torch.int32, device=dev)
    cloop = torch.full((c,), -1, dtype=torch.int32, device=dev)
    kept = torch.zeros((c,), dtype=torch.uint8, device=dev)
    nfixed = torch.zeros((n,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SIMPLIFY_FLAGS, dev)
    if c and n:
        _lib.call("ullsam_simplify_candidates", reid.data_ptr(), cand.data_ptr(), coff.data_ptr(), estart.data_ptr(), e, n, c, h, w, cxy.data_ptr(),
                  cloop.data_ptr(), kept.data_ptr(), nfixed.data_ptr(), flags.data_ptr(), _stream())
    return cxy, cloop, kept, nfixed, flags


def _simplify_table(cxy: torch.Tensor, cloop: torch.Tensor, kept: torch.Tensor, loops: int, what: str):
    _chk(cxy, "cxy", torch.int32)
    c, n = cxy.numel(), int(loops)
    _outline_vec(cloop, "cloop", c); _outline_vec(kept, "kept", c, torch.uint8)
    if not 0 <= n <= c:
        raise _lib.UllsamError(f"{what}: {n} loops of {c} candidates (need L <= C)")
    return c, n


def simplify_anchors(cxy: torch.Tensor, cloop: torch.Tensor, nfixed: torch.Tensor, kept: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """Marks, IN kept, the two anchors of every loop without a fixed point (ullsam_hip.h simplify_anchors) -> (kept, flags)."""
    c, n = _simplify_table(cxy, cloop, kept, nfixed.numel(), "simplify_anchors")
    _chk(nfixed, "nfixed", torch.int32)
    flags = _flags_i32(flags, SIMPLIFY_FLAGS, cxy.device)
    if c and n:
        ws = torch.empty((2, n), dtype=torch.int64, device=cxy.device)
        _lib.call("ullsam_simplify_anchors", cxy.data_ptr(), cloop.data_ptr(), nfixed.data_ptr(), c, n, ws.data_ptr(), kept.data_ptr(), flags.data_ptr(), _stream())
    return kept, flags


def simplify_segments(kept: torch.Tensor, cloop: torch.Tensor, cstart: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """cstart int32 [L + 1] -> (pa, pb int32 [C], flags): the kept candidates before and after every candidate that is not kept, cyclic in its loop;
    -1 for a kept one (ullsam_hip.h simplify_segments)."""
    _chk(kept, "kept", torch.uint8); _chk(cstart, "cstart", torch.int32)
    c, n, dev = kept.numel(), cstart.numel() - 1, kept.device
    _outline_vec(cloop, "cloop", c)
    if not 0 <= n <= c:
        raise _lib.UllsamError(f"simplify_segments: {n} loops of {c} candidates (need L <= C)")
    pa = torch.full((c,), -1, dtype=torch.int32, device=dev)
    pb = torch.full((c,), -1, dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SIMPLIFY_FLAGS, dev)
    if c:
        koff, total = outline_scan(kept)
        klist = torch.empty((c,), dtype=torch.int32, device=dev)
        _lib.call("ullsam_simplify_segments", kept.data_ptr(), koff.data_ptr(), total.data_ptr(), cloop.data_ptr(), cstart.data_ptr(), c, n, klist.data_ptr(),
                  pa.data_ptr(), pb.data_ptr(), flags.data_ptr(), _stream())
    return pa, pb, flags


def simplify_rounds(cxy: torch.Tensor, cloop: torch.Tensor, cstart: torch.Tensor, t: int, rounds: int, pa: torch.Tensor, pb: torch.Tensor,
                    kept: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """`rounds` rounds of the rule at tolerance t / 256 pixel, IN pa, pb and kept -> (counts int32 [rounds] = the candidates every round kept, flags)
    (ullsam_hip.h simplify_rounds)."""
    _chk(cstart, "cstart", torch.int32)
    c, n = _simplify_table(cxy, cloop, kept, cstart.numel() - 1, "simplify_rounds")
    _outline_vec(pa, "pa", c); _outline_vec(pb, "pb", c)
    t, rounds = int(t), int(rounds)
    if not (0 <= t <= SIMPLIFY_MAX_T and 1 <= rounds <= 1024):
        raise _lib.UllsamError(f"simplify_rounds: t = {t} must lie in 0..{SIMPLIFY_MAX_T} and rounds = {rounds} in 1..1024")
    dev = cxy.device
    counts = torch.zeros((rounds,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, SIMPLIFY_FLAGS, dev)
    if c:
        ws = torch.empty((3, c), dtype=torch.int64, device=dev)
        _lib.call("ullsam_simplify_rounds", cxy.data_ptr(), cloop.data_ptr(), cstart.data_ptr(), c, n, t * t, rounds, ws.data_ptr(), pa.data_ptr(), pb.data_ptr(),
                  kept.data_ptr(), counts.data_ptr(), flags.data_ptr(), _stream())
    return counts, flags


def simplify_rings(cxy: torch.Tensor, cloop: torch.Tensor, kept: torch.Tensor, voff: torch.Tensor, total: torch.Tensor, cstart: torch.Tensor, count: int,
                   flags: Optional[torch.Tensor] = None):
    """voff, total = outline_scan(kept), N = count = total -> (vertices int32 [N, 2], nvert int32 [L], area2 int64 [L], flags): the kept candidates in
    order, and the vertex count and shoelace sum of every loop's ring (ullsam_hip.h simplify_rings)."""
    _chk(cstart, "cstart", torch.int32); _chk(total, "total", torch.int32)
    c, n = _simplify_table(cxy, cloop, kept, cstart.numel() - 1, "simplify_rings")
    _outline_vec(voff, "voff", c)
    nv, dev = int(count), cxy.device
    if not 0 <= nv <= c or total.numel() != 1:
        raise _lib.UllsamError(f"simplify_rings: count = {count} must lie in 0..C = {c}, total hold one value")
    vertices = torch.zeros((nv, 2), dtype=torch.int32, device=dev)
    nvert = torch.zeros((n,), dtype=torch.int32, device=dev)
    area2 = torch.zeros((n,), dtype=torch.int64, device=dev)
    flags = _flags_i32(flags, SIMPLIFY_FLAGS, dev)
    if c and n and nv:
        klist = torch.empty((c,), dtype=torch.int32, device=dev)
        _lib.call("ullsam_simplify_rings", cxy.data_ptr(), cloop.data_ptr(), kept.data_ptr(), voff.data_ptr(), total.data_ptr(), cstart.data_ptr(), c, n, nv,
                  klist.data_ptr(), vertices.data_ptr(), nvert.data_ptr(), area2.data_ptr(), flags.data_ptr(), _stream())
    return vertices, nvert, area2, flags


# ---- polygons to a label image: exact scanline rasterisation (csrc/raster.hip; utils.raster drives these) -------------------------------------
RASTER_FLAGS = 4           # status bits (1 bad ring_label, 2 coordinate beyond the range, 4 a total above 2^31 - 1, 8 an index left its table), C, (two free)
RASTER_MAX_SIDE = 32767
RASTER_MAX_IDS = 65535
RASTER_CHUNK = 2048        # values per workgroup of the scan (raster.hip RS_CHUNK)
RASTER_FORMS = {"waves": 0, "pixels": 1}


def _raster_frame(h: int, w: int, num: int, what: str):
    h, w, k = int(h), int(w), int(num)
    if not (1 <= h <= RASTER_MAX_SIDE and 1 <= w <= RASTER_MAX_SIDE and 0 <= k <= RASTER_MAX_IDS):
        raise _lib.UllsamError(f"{what}: a frame of {h} x {w} with {k} ids (each side in 1..32767, at most 65535 ids)")
    return h, w, k


def raster_scan(vals: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """vals int32 [n], each in 0..32767 -> (off int32 [n] = their exclusive scan, total int32 [1], flags); a total above 2^31 - 1 raises bit 4 of
    flags[0] (ullsam_hip.h raster_scan)."""
    _chk(vals, "vals", torch.int32)
    n, dev = vals.numel(), vals.device
    off = torch.empty((n,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, RASTER_FLAGS, dev)
    _lib.call("ullsam_raster_scan", _p(vals) if n else None, n, _p(off) if n else None, _scan_sums(n, RASTER_CHUNK, dev).data_ptr(), total.data_ptr(), flags.data_ptr(),
              _stream())
    return off, total, flags


def raster_edges(q: torch.Tensor, start: torch.Tensor, ring_label: torch.Tensor, h: int, w: int, num: int, flags: Optional[torch.Tensor] = None):
    """q int32 [N, 2] (1/256 pixel), start int32 [R + 1], ring_label int32 [R] -> (row0, cnt, nxt, elab, off int32 [N], flags): per edge the first and
    the number of the rows it crosses, its second vertex, its label, and the exclusive scan of cnt; flags[1] = C (ullsam_hip.h raster_edges)."""
    h, w, k = _raster_frame(h, w, num, "raster_edges")
    _chk(q, "q", torch.int32); _chk(start, "start", torch.int32); _chk(ring_label, "ring_label", torch.int32)
    assert q.dim() == 2 and q.shape[1] == 2, tuple(q.shape)
    n, r, dev = q.shape[0], ring_label.numel(), q.device
    assert start.numel() == r + 1 and (r >= 1 or n == 0), (tuple(start.shape), r, n)
    row0, cnt, nxt, elab, off = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(5))
    flags = _flags_i32(flags, RASTER_FLAGS, dev)
    if n:
        _lib.call("ullsam_raster_edges", q.data_ptr(), n, start.data_ptr(), r, ring_label.data_ptr(), h, w, k, row0.data_ptr(), cnt.data_ptr(), nxt.data_ptr(),
                  elab.data_ptr(), off.data_ptr(), _scan_sums(n, RASTER_CHUNK, dev).data_ptr(), flags.data_ptr(), _stream())
    return row0, cnt, nxt, elab, off, flags


def raster_keys(q: torch.Tensor, row0: torch.Tensor, cnt: torch.Tensor, nxt: torch.Tensor, elab: torch.Tensor, off: torch.Tensor, crossings: int, h: int,
                w: int, num: int, flags: Optional[torch.Tensor] = None):
    """raster_edges' tables and C = crossings -> (keys int64 [C] = label << 32 | row << 16 | xs of every crossing, in edge order, flags): one work
    item per crossing, its edge found by a search in off (ullsam_hip.h raster_keys)."""
    h, w, k = _raster_frame(h, w, num, "raster_keys")
    _chk(q, "q", torch.int32)
    n, c, dev = q.shape[0], int(crossings), q.device
    for t, name in ((row0, "row0"), (cnt, "cnt"), (nxt, "nxt"), (elab, "elab"), (off, "off")):
        _chk(t, name, torch.int32)
        assert t.numel() == n, (name, tuple(t.shape), n)
    if not 0 <= c <= DISTANCE_INF or (c and not n):
        raise _lib.UllsamError(f"raster_keys: crossings = {crossings} must lie in 0..2^31 - 1, and 0 without an edge")
    keys = torch.zeros((c,), dtype=torch.int64, device=dev)
    flags = _flags_i32(flags, RASTER_FLAGS, dev)
    if c:
        _lib.call("ullsam_raster_keys", q.data_ptr(), n, row0.data_ptr(), cnt.data_ptr(), nxt.data_ptr(), elab.data_ptr(), off.data_ptr(), c, h, w, k,
                  keys.data_ptr(), flags.data_ptr(), _stream())
    return keys, flags


def _raster_sorted(keys: torch.Tensor, what: str) -> int:
    _chk(keys, "keys", torch.int64)
    if keys.numel() % 2:
        raise _lib.UllsamError(f"{what}: {keys.numel()} keys (the crossings of closed rings come in pairs)")
    return keys.numel()


def raster_covered(keys: torch.Tensor, h: int, w: int, num: int, flags: Optional[torch.Tensor] = None):
    """keys int64 [C], SORTED -> (covered int32 [K] = the pixels of the frame inside every label, before overlaps, length int32 [C / 2] = the length of
    span j = keys[2 j], keys[2 j + 1], flags) (ullsam_hip.h raster_covered)."""
    h, w, k = _raster_frame(h, w, num, "raster_covered")
    c, dev = _raster_sorted(keys, "raster_covered"), keys.device
    covered = torch.zeros((k,), dtype=torch.int32, device=dev)
    length = torch.zeros((c // 2,), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, RASTER_FLAGS, dev)
    if c and k:
        _lib.call("ullsam_raster_covered", keys.data_ptr(), c, h, w, k, covered.data_ptr(), length.data_ptr(), flags.data_ptr(), _stream())
    return covered, length, flags


def raster_paint(keys: torch.Tensor, rank: torch.Tensor, h: int, w: int, form: str = "waves", length: Optional[torch.Tensor] = None,
                 flags: Optional[torch.Tensor] = None):
    """keys int64 [C], SORTED, rank int32 [K] (a permutation of 0..K - 1, larger = on top) -> (raw int32 [h, w] = 1 + the largest rank among the spans
    covering the pixel, 0 where none does, flags).  form "waves": one wave per span, its lanes striding the pixels; "pixels": one lane per pixel over a
    scan of `length` (raster_covered's), whose total stays on the device (ullsam_hip.h raster_paint)."""
    _chk(rank, "rank", torch.int32)
    h, w, k = _raster_frame(h, w, rank.numel(), "raster_paint")
    c, dev = _raster_sorted(keys, "raster_paint"), keys.device
    if form not in RASTER_FORMS:
        raise _lib.UllsamError(f'raster_paint: form must be "waves" or "pixels", got {form!r}')
    flags = _flags_i32(flags, RASTER_FLAGS, dev)
    if not (c and k):
        return torch.zeros((h, w), dtype=torch.int32, device=dev), flags
    poff = total = None
    if form == "pixels":
        if length is None:
            raise _lib.UllsamError('raster_paint: form "pixels" needs the span lengths')
        _chk(length, "length", torch.int32)
        assert length.numel() == c // 2, (tuple(length.shape), c)
        poff, total, _ = raster_scan(length, flags)
    raw = torch.empty((h, w), dtype=torch.int32, device=dev)
    _lib.call("ullsam_raster_paint", keys.data_ptr(), c, rank.data_ptr(), h, w, k, RASTER_FORMS[form], _p(poff), _p(total), raw.data_ptr(), flags.data_ptr(),
              _stream())
    return raw, flags


def raster_finish(raw: torch.Tensor, label_of: torch.Tensor, flags: Optional[torch.Tensor] = None):
    """raw int32 [H, W] (values 0..K), label_of int32 [K + 1] (label_of[0] = 0) -> (labels int32 [H, W] = label_of[raw], area int32 [K], box int32
    [K, 4] inclusive XYXY, (INT_MAX, INT_MAX, -1, -1) for a label without a pixel, flags): row-major, one pass (ullsam_hip.h raster_finish)."""
    _chk(raw, "raw", torch.int32); _chk(label_of, "label_of", torch.int32)
    assert raw.dim() == 2 and label_of.numel() >= 1, (tuple(raw.shape), tuple(label_of.shape))
    h, w, k = _raster_frame(raw.shape[0], raw.shape[1], label_of.numel() - 1, "raster_finish")
    dev = raw.device
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    area = torch.empty((k,), dtype=torch.int32, device=dev)
    box = torch.empty((k, 4), dtype=torch.int32, device=dev)
    flags = _flags_i32(flags, RASTER_FLAGS, dev)
    _lib.call("ullsam_raster_finish", raw.data_ptr(), h, w, label_of.data_ptr(), k, labels.data_ptr(), _p(area) if k else None, _p(box) if k else None,
              flags.data_ptr(), _stream())
    return labels, area, box, flags


# ---- per-instance measurements and contacts from a label image (csrc/measure.hip; utils.measure drives these) ---------------------------------
MEASURE_MAX_SIDE = 46340  # x * x < 2^31 and H * W < 2^31: every sum of the tables stays below 2^62
MEASURE_MAX_CHANNELS = 4
MEASURE_LDS_SLOTS = 128   # the per-workgroup LDS table of the default route, and the largest (0: every run straight to the global tables)
MEASURE_FLAGS = 4         # bad id, pair table overflow, distinct pairs, rows written


def _measure_frame(labels: torch.Tensor, num: int, what: str):
    _chk(labels, "labels", torch.int32)
    if labels.dim() != 2:
        raise ValueError(f"{what}: labels must be [H, W], got {tuple(labels.shape)}")
    h, w = labels.shape
    if not (1 <= h <= MEASURE_MAX_SIDE and 1 <= w <= MEASURE_MAX_SIDE):
        raise _lib.UllsamError(f"{what}: a frame of {h} x {w} (each side must lie in 1..{MEASURE_MAX_SIDE})")
    if not 0 <= int(num) <= MOSAIC_MAX_IDS:
        raise _lib.UllsamError(f"{what}: num = {num} must lie in 0..2^31 - 2")
    return h, w


def _out_view(out, name: str, shape, dtype, device) -> torch.Tensor:
    if out is None or name not in out:
        return torch.empty(shape, dtype=dtype, device=device)
    t = out[name]
    _chk(t, name, dtype)
    assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), tuple(shape))
    return t


def measure_instances(labels: torch.Tensor, num: int, intensity: Optional[torch.Tensor] = None, lds_slots: int = MEASURE_LDS_SLOTS,
                      out: Optional[dict] = None, flags: Optional[torch.Tensor] = None):
    """labels int32 [H, W] with ids 0..num, intensity None or uint8 / uint16 [H, W] / [H, W, C <= 4] -> (dict of the tables of ullsam_hip.h: area int64
    [num], box int32 [num, 4], moments int64 [num, 5], perimeter int64 [num, 3] and, with an image, isum / isum2 int64 [num, C], imin / imax int32
    [num, C]; flags int32 [4]: the caller reads flags[0]).  lds_slots: a power of two <= 128 (the runs of equal labels are summed in a per-workgroup LDS
    table first: the faster route as measured, tools/measure_bench.py) or 0 (every run straight to the global tables); same results.  out: preallocated tables by name."""
    h, w = _measure_frame(labels, num, "measure_instances")
    k, dev = int(num), labels.device
    c, nbytes = 0, 0
    if intensity is not None:
        if intensity.dtype not in (torch.uint8, torch.uint16):
            raise _lib.UllsamError(f"measure_instances: the intensity image must be uint8 or uint16, got {intensity.dtype} (float sums depend on the order of arrival)")
        _chk(intensity, "intensity")
        if intensity.dim() not in (2, 3) or tuple(intensity.shape[:2]) != (h, w):
            raise ValueError(f"measure_instances: intensity {tuple(intensity.shape)} for labels {(h, w)}")
        c = 1 if intensity.dim() == 2 else int(intensity.shape[2])
        if not 1 <= c <= MEASURE_MAX_CHANNELS:
            raise _lib.UllsamError(f"measure_instances: {c} channels (1..{MEASURE_MAX_CHANNELS})")
        nbytes = intensity.element_size()
    lds_slots = int(lds_slots)
    if lds_slots < 0 or lds_slots > MEASURE_LDS_SLOTS or lds_slots & (lds_slots - 1):
        raise _lib.UllsamError(f"measure_instances: lds_slots = {lds_slots} must be 0 or a power of two <= {MEASURE_LDS_SLOTS}")
    i32, i64 = torch.int32, torch.int64
    t = {"area": _out_view(out, "area", (k,), i64, dev), "box": _out_view(out, "box", (k, 4), i32, dev),
         "moments": _out_view(out, "moments", (k, 5), i64, dev), "perimeter": _out_view(out, "perimeter", (k, 3), i64, dev)}
    if c:
        t.update(isum=_out_view(out, "isum", (k, c), i64, dev), isum2=_out_view(out, "isum2", (k, c), i64, dev),
                 imin=_out_view(out, "imin", (k, c), i32, dev), imax=_out_view(out, "imax", (k, c), i32, dev))
    flags = _out_i32(flags, (MEASURE_FLAGS,), dev, "flags")
    _lib.call("ullsam_measure_instances", labels.data_ptr(), h, w, k, _p(intensity), c, nbytes, lds_slots, t["area"].data_ptr(), t["box"].data_ptr(),
              t["moments"].data_ptr(), t["perimeter"].data_ptr(), _p(t.get("isum")), _p(t.get("isum2")), _p(t.get("imin")), _p(t.get("imax")),
              flags.data_ptr(), _stream())
    return t, flags


def label_contacts(labels: torch.Tensor, num: int, max_pairs: int = 1 << 20, flags: Optional[torch.Tensor] = None):
    """labels int32 [H, W] with ids 0..num -> (rows int64 [max_pairs, 2] = (a << 32 | b, n) of the pairs 0 < a < b that share n pixel sides, in no
    particular order; flags int32 [4]: bad id, overflow, distinct pairs, rows written -- the caller reads them and keeps the first flags[2] rows)."""
    h, w = _measure_frame(labels, num, "label_contacts")
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise _lib.UllsamError(f"label_contacts: max_pairs must lie in 1..2^30, got {max_pairs}")
    dev = labels.device
    cap = mosaic_table_slots(max_pairs)
    keys = torch.empty((cap,), dtype=torch.int64, device=dev)
    counts = torch.empty((cap,), dtype=torch.int64, device=dev)
    rows = torch.empty((max_pairs, 2), dtype=torch.int64, device=dev)
    flags = _out_i32(flags, (MEASURE_FLAGS,), dev, "flags")
    _lib.call("ullsam_label_contacts", labels.data_ptr(), h, w, int(num), keys.data_ptr(), counts.data_ptr(), cap, max_pairs, rows.data_ptr(),
              flags.data_ptr(), _stream())
    return rows, flags


# ---- per-object measurements and contacts from a label volume (csrc/measure3d.hip; utils.measure3d drives these) ------------------------------
MEASURE3D_MAX_SIDE = 32767            # x * x < 2^30
MEASURE3D_MAX_VOXELS = 2 ** 31 - 1    # every count < 2^31: coordinate sums below 2^61, sum v^2 below 65535^2 (2^31 - 1) < 2^63
MEASURE3D_TILE_R = 8                  # M3_TILE_R and M3_TILE_P of csrc/measure3d.hip: a workgroup's tile is 256 columns x 8 rows x 4 planes
MEASURE3D_TILE_P = 4
MEASURE3D_LDS_SLOTS = 128             # the default route: the LDS table, 2 - 3 x faster per call than 0 (tools/measure3d_bench.py, profiles/r25_measure3d.txt)


def _measure3d_volume(volume: torch.Tensor, num: int, what: str):
    z, h, w = _volume_zhw(volume, what)
    if not 0 <= int(num) <= MOSAIC_MAX_IDS:
        raise _lib.UllsamError(f"{what}: num = {num} must lie in 0..2^31 - 2")
    return z, h, w


def measure_objects3d(volume: torch.Tensor, num: int, intensity: Optional[torch.Tensor] = None, lds_slots: int = MEASURE3D_LDS_SLOTS,
                      out: Optional[dict] = None, flags: Optional[torch.Tensor] = None):
    """volume int32 [Z, H, W] with ids 0..num, intensity None or uint8 / uint16 [Z, H, W] / [Z, H, W, C <= 4] -> (dict of the tables of ullsam_hip.h:
    voxels int64 [num], box int32 [num, 6], moments int64 [num, 9], surface int64 [num, 7] and, with an image, isum / isum2 int64 [num, C], imin /
    imax int32 [num, C]; flags int32 [4]: the caller reads flags[0]).  lds_slots: a power of two <= 128 (the runs of equal labels are summed in a
    per-workgroup LDS table first: the faster route as measured, tools/measure3d_bench.py) or 0 (every run straight to the global tables); same
    results.  out: preallocated tables by name."""
    z, h, w = _measure3d_volume(volume, num, "measure_objects3d")
    k, dev = int(num), volume.device
    c, nbytes = 0, 0
    if intensity is not None:
        if intensity.dtype not in (torch.uint8, torch.uint16):
            raise _lib.UllsamError(f"measure_objects3d: the intensity image must be uint8 or uint16, got {intensity.dtype} (float sums depend on the order of arrival)")
        _chk(intensity, "intensity")
        if intensity.dim() not in (3, 4) or tuple(intensity.shape[:3]) != (z, h, w):
            raise ValueError(f"measure_objects3d: intensity {tuple(intensity.shape)} for a volume {(z, h, w)}")
        c = 1 if intensity.dim() == 3 else int(intensity.shape[3])
        if not 1 <= c <= MEASURE_MAX_CHANNELS:
            raise _lib.UllsamError(f"measure_objects3d: {c} channels (1..{MEASURE_MAX_CHANNELS})")
        nbytes = intensity.element_size()
    lds_slots = int(lds_slots)
    if lds_slots < 0 or lds_slots > MEASURE_LDS_SLOTS or lds_slots & (lds_slots - 1):
        raise _lib.UllsamError(f"measure_objects3d: lds_slots = {lds_slots} must be 0 or a power of two <= {MEASURE_LDS_SLOTS}")
    i32, i64 = torch.int32, torch.int64
    t = {"voxels": _out_view(out, "voxels", (k,), i64, dev), "box": _out_view(out, "box", (k, 6), i32, dev),
         "moments": _out_view(out, "moments", (k, 9), i64, dev), "surface": _out_view(out, "surface", (k, 7), i64, dev)}
    if c:
        t.update(isum=_out_view(out, "isum", (k, c), i64, dev), isum2=_out_view(out, "isum2", (k, c), i64, dev),
                 imin=_out_view(out, "imin", (k, c), i32, dev), imax=_out_view(out, "imax", (k, c), i32, dev))
    flags = _out_i32(flags, (MEASURE_FLAGS,), dev, "flags")
    _lib.call("ullsam_measure_objects3d", volume.data_ptr(), z, h, w, k, _p(intensity), c, nbytes, lds_slots, t["voxels"].data_ptr(), t["box"].data_ptr(),
              t["moments"].data_ptr(), t["surface"].data_ptr(), _p(t.get("isum")), _p(t.get("isum2")), _p(t.get("imin")), _p(t.get("imax")),
              flags.data_ptr(), _stream())
    return t, flags


def object_contacts3d(volume: torch.Tensor, num: int, max_pairs: int = 1 << 20, flags: Optional[torch.Tensor] = None):
    """volume int32 [Z, H, W] with ids 0..num -> (rows int64 [max_pairs, 4] = (a << 32 | b, nz, ny, nx) of the pairs 0 < a < b and the voxel faces they
    share per axis, in no particular order; flags int32 [4]: bad id, overflow, distinct pairs, rows written -- the caller reads them and keeps the
    first flags[2] rows)."""
    z, h, w = _measure3d_volume(volume, num, "object_contacts3d")
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= 2 ** 30:
        raise _lib.UllsamError(f"object_contacts3d: max_pairs must lie in 1..2^30, got {max_pairs}")
    dev = volume.device
    cap = mosaic_table_slots(max_pairs)
    keys = torch.empty((cap,), dtype=torch.int64, device=dev)
    counts = torch.empty((cap, 3), dtype=torch.int64, device=dev)
    rows = torch.empty((max_pairs, 4), dtype=torch.int64, device=dev)
    flags = _out_i32(flags, (MEASURE_FLAGS,), dev, "flags")
    _lib.call("ullsam_object_contacts3d", volume.data_ptr(), z, h, w, int(num), keys.data_ptr(), counts.data_ptr(), cap, max_pairs, rows.data_ptr(),
              flags.data_ptr(), _stream())
    return rows, flags


# ---- surface meshes and Euler numbers of a label volume (csrc/mesh3d.hip; utils.mesh3d drives these) -------------------------------------------
MESH3D_TILE_Y = 4                     # MS_TILE_Y and MS_TILE_Z of csrc/mesh3d.hip: a workgroup's tile is 64 columns x 4 rows x 4 planes
MESH3D_TILE_Z = 4
MESH3D_TILE_X = 64
MESH3D_MAX_LABEL = 2 ** 29 - 1        # a key is id | label << 34 and stays below 2^63
MESH3D_KEY_SHIFT = 34
INT32_MAX_COUNT = 2 ** 31 - 1         # faces and vertices are indexed in int32
MESH3D_BLOCK_KEYS = 2048              # sorted keys per workgroup of the heads / vertices kernels


def _mesh3d_volume(volume: torch.Tensor, num: int, what: str, max_label: int):
    z, h, w = _volume_zhw(volume, what)
    if not 0 <= int(num) <= max_label:
        raise _lib.UllsamError(f"{what}: num = {num} must lie in 0..{max_label}")
    return z, h, w


def _mesh3d_keys(t: torch.Tensor, name: str) -> int:
    _chk(t, name, torch.int64)
    if t.dim() != 1 or t.numel() > 4 * INT32_MAX_COUNT:
        raise ValueError(f"{name} must be int64 [n] with n <= 4 (2^31 - 1), got {tuple(t.shape)}")
    return t.numel()


def _mesh3d_plane(h: int, w: int, what: str):
    h, w = int(h), int(w)
    if not (1 <= h <= MEASURE3D_MAX_SIDE and 1 <= w <= MEASURE3D_MAX_SIDE):
        raise _lib.UllsamError(f"{what}: H = {h} and W = {w} must lie in 1..{MEASURE3D_MAX_SIDE}")
    return h, w


def mesh3d_tiles(z: int, h: int, w: int) -> int:
    return -(-w // MESH3D_TILE_X) * -(-h // MESH3D_TILE_Y) * -(-z // MESH3D_TILE_Z)


def mesh3d_masks(volume: torch.Tensor, num: int, only: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None):
    """volume int32 [Z, H, W] with ids 0..num <= 2^29 - 1, only None or uint8 [num + 1] (faces are made for the ids with only[id] != 0) -> (masks uint8
    [Z, H, W]: bit d of a voxel = it has a face towards d (0 = -z, 1 = +z, 2 = -y, 3 = +y, 4 = -x, 5 = +x); tile_offsets int64 [T + 1]: the exclusive
    sums of the faces per 64 x 4 x 4 tile, [T] = F; flags int32 [4]: the caller reads flags[0])."""
    z, h, w = _mesh3d_volume(volume, num, "mesh3d_masks", MESH3D_MAX_LABEL)
    if only is not None:
        _chk(only, "only", torch.uint8)
        if tuple(only.shape) != (int(num) + 1,):
            raise ValueError(f"mesh3d_masks: only must be uint8 [num + 1] = [{int(num) + 1}], got {tuple(only.shape)}")
    dev, t = volume.device, mesh3d_tiles(z, h, w)
    masks = torch.empty((z, h, w), dtype=torch.uint8, device=dev)
    counts = torch.empty((t,), dtype=torch.int32, device=dev)
    offsets = torch.empty((t + 1,), dtype=torch.int64, device=dev)
    flags = _out_i32(flags, (MEASURE_FLAGS,), dev, "flags")
    _lib.call("ullsam_mesh3d_masks", volume.data_ptr(), z, h, w, int(num), _p(only), masks.data_ptr(), counts.data_ptr(), offsets.data_ptr(),
              flags.data_ptr(), _stream())
    return masks, offsets, flags


def mesh3d_faces(volume: torch.Tensor, masks: torch.Tensor, tile_offsets: torch.Tensor, faces: int) -> torch.Tensor:
    """masks, tile_offsets of mesh3d_masks and faces = F = tile_offsets[-1] -> fkeys int64 [F] = 6 p + d | label << 34 of every face, a tile's at
    its offset (not sorted)."""
    z, h, w = _mesh3d_volume(volume, 0, "mesh3d_faces", MESH3D_MAX_LABEL)
    _chk(masks, "masks", torch.uint8); _chk(tile_offsets, "tile_offsets", torch.int64)
    if tuple(masks.shape) != (z, h, w) or tuple(tile_offsets.shape) != (mesh3d_tiles(z, h, w) + 1,):
        raise ValueError(f"mesh3d_faces: masks {tuple(masks.shape)} / tile_offsets {tuple(tile_offsets.shape)} for a volume {(z, h, w)}")
    f = int(faces)
    if not 0 <= f <= INT32_MAX_COUNT:
        raise _lib.UllsamError(f"mesh3d_faces: {f} faces (at most 2^31 - 1)")
    fkeys = torch.empty((f,), dtype=torch.int64, device=volume.device)
    _lib.call("ullsam_mesh3d_faces", volume.data_ptr(), masks.data_ptr(), z, h, w, tile_offsets.data_ptr(), fkeys.data_ptr(), f, _stream())
    return fkeys


def mesh3d_corners(fkeys: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """fkeys int64 [F] -> ckeys int64 [4 F]: corner id | label << 34 of the four corners of every face, counter-clockwise seen from outside."""
    f = _mesh3d_keys(fkeys, "fkeys")
    h, w = _mesh3d_plane(h, w, "mesh3d_corners")
    if f > INT32_MAX_COUNT:
        raise _lib.UllsamError(f"mesh3d_corners: {f} faces (at most 2^31 - 1)")
    ckeys = torch.empty((4 * f,), dtype=torch.int64, device=fkeys.device)
    _lib.call("ullsam_mesh3d_corners", fkeys.data_ptr(), f, h, w, ckeys.data_ptr(), _stream())
    return ckeys


def mesh3d_heads(sorted_keys: torch.Tensor) -> torch.Tensor:
    """sorted int64 [n] -> block_offsets int64 [B + 1], B = ceil(n / 2048): the exclusive sums of the number of keys per block that differ from their
    predecessor; [B] = the number of distinct keys."""
    n = _mesh3d_keys(sorted_keys, "sorted_keys")
    b = -(-n // MESH3D_BLOCK_KEYS)
    counts = torch.empty((max(b, 1),), dtype=torch.int32, device=sorted_keys.device)
    offsets = torch.empty((b + 1,), dtype=torch.int64, device=sorted_keys.device)
    _lib.call("ullsam_mesh3d_heads", sorted_keys.data_ptr(), n, counts.data_ptr(), offsets.data_ptr(), _stream())
    return offsets


def mesh3d_vertices(sorted_keys: torch.Tensor, block_offsets: torch.Tensor, count: int, h: int, w: int, vertices: Optional[torch.Tensor] = None):
    """sorted corner keys, mesh3d_heads' offsets and count = V = block_offsets[-1] -> (ukeys int64 [V] = the distinct keys in order, vertices int32
    [V, 3] = their lattice corners (x, y, z))."""
    n = _mesh3d_keys(sorted_keys, "sorted_keys")
    h, w = _mesh3d_plane(h, w, "mesh3d_vertices")
    _chk(block_offsets, "block_offsets", torch.int64)
    if tuple(block_offsets.shape) != (-(-n // MESH3D_BLOCK_KEYS) + 1,):
        raise ValueError(f"mesh3d_vertices: block_offsets {tuple(block_offsets.shape)} for {n} keys")
    v = int(count)
    if not 0 <= v <= min(n, INT32_MAX_COUNT):
        raise _lib.UllsamError(f"mesh3d_vertices: {v} vertices of {n} keys (at most 2^31 - 1)")
    ukeys = torch.empty((v,), dtype=torch.int64, device=sorted_keys.device)
    vertices = _out_i32(vertices, (v, 3), sorted_keys.device, "vertices")
    _lib.call("ullsam_mesh3d_vertices", sorted_keys.data_ptr(), n, block_offsets.data_ptr(), h, w, ukeys.data_ptr(), vertices.data_ptr(), v, _stream())
    return ukeys, vertices


def mesh3d_quads(fkeys: torch.Tensor, ukeys: torch.Tensor, h: int, w: int, quads: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fkeys int64 [F], ukeys int64 [V] sorted and distinct -> quads int32 [F, 4]: the index in ukeys of each corner key of each face."""
    f, v = _mesh3d_keys(fkeys, "fkeys"), _mesh3d_keys(ukeys, "ukeys")
    h, w = _mesh3d_plane(h, w, "mesh3d_quads")
    if f > INT32_MAX_COUNT or v > INT32_MAX_COUNT:
        raise _lib.UllsamError(f"mesh3d_quads: {f} faces and {v} vertices (at most 2^31 - 1 each)")
    quads = _out_i32(quads, (f, 4), fkeys.device, "quads")
    _lib.call("ullsam_mesh3d_quads", fkeys.data_ptr(), f, ukeys.data_ptr(), v, h, w, quads.data_ptr(), _stream())
    return quads


def mesh3d_starts(sorted_keys: torch.Tensor, num: int, start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sorted int64 [n] -> start int64 [num + 1]: start[k] = the number of keys whose label (key >> 34) is <= k."""
    n, k = _mesh3d_keys(sorted_keys, "sorted_keys"), int(num)
    if not 0 <= k <= MESH3D_MAX_LABEL:
        raise _lib.UllsamError(f"mesh3d_starts: num = {k} must lie in 0..2^29 - 1")
    if start is None:
        start = torch.empty((k + 1,), dtype=torch.int64, device=sorted_keys.device)
    _chk(start, "start", torch.int64)
    assert tuple(start.shape) == (k + 1,), (tuple(start.shape), k + 1)
    _lib.call("ullsam_mesh3d_starts", sorted_keys.data_ptr(), n, k, start.data_ptr(), _stream())
    return start


def mesh3d_topology(volume: torch.Tensor, num: int, out: Optional[dict] = None, flags: Optional[torch.Tensor] = None):
    """volume int32 [Z, H, W] with ids 0..num -> (euler int64 [num], pinch_edges int64 [num], flags int32 [4]: the caller reads flags[0]); the
    definitions of ullsam_hip.h.  out: preallocated tables by name."""
    z, h, w = _mesh3d_volume(volume, num, "mesh3d_topology", MOSAIC_MAX_IDS)
    k, dev = int(num), volume.device
    euler = _out_view(out, "euler", (k,), torch.int64, dev)
    pinch = _out_view(out, "pinch_edges", (k,), torch.int64, dev)
    flags = _out_i32(flags, (MEASURE_FLAGS,), dev, "flags")
    _lib.call("ullsam_mesh3d_topology", volume.data_ptr(), z, h, w, k, euler.data_ptr(), pinch.data_ptr(), flags.data_ptr(), _stream())
    return euler, pinch, flags


# ---- the interactive loop's display tail (csrc/interactive.hip) ---------------------------------------------------------------------
CLICK_MAX_P = 512


def click_finish(low: torch.Tensor, frame: int, hw, side: Optional[int] = None, top: int = 0, left: int = 0, thr: float = 0.0,
                 image: Optional[torch.Tensor] = None, canvas: Optional[torch.Tensor] = None, first_id: int = 1, paint: bool = False,
                 highlight: bool = False, lut_inst: Optional[torch.Tensor] = None, lut_cur: Optional[torch.Tensor] = None,
                 want_mask: bool = True, want_overlay: bool = False, want_stats: bool = True, mask: Optional[torch.Tensor] = None,
                 overlay: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None):
    """One launch from the logits low fp32 [P, LH, LW] of P masks to what the display shows (include/ullsam_hip.h ullsam_click_finish): the
    display image is [H, W] = hw at (top, left) of the padded square of side `side` (default max(H, W)) that the frame x frame model input was
    resized from.  Returns (mask uint8 [P, H, W], overlay uint8 [H, W, 3], stats int32 [P, 5] = area, x0, y0, x1, y1), None for what was not
    asked for; mask= / overlay= / stats= are buffers to fill.  paint writes first_id + p into canvas int32 [H, W] in place (last p on top);
    the overlay blends image uint8 [H, W, 3] through lut_inst uint8 [K, 3, 256] by canvas id and, with highlight, through lut_cur uint8 [3, 256]
    where the last mask is set."""
    _chk(low, "low", torch.float32)
    assert low.dim() == 3, low.shape
    P, LH, LW = low.shape
    H, W = (int(v) for v in hw)
    side = max(H, W) if side is None else int(side)
    dev = low.device

    def buf(t, want, shape, dtype, name):
        if t is not None:
            _chk(t, name, dtype)
            assert tuple(t.shape) == shape, (name, tuple(t.shape), shape)
            return t
        return torch.empty(shape, dtype=dtype, device=dev) if want else None

    mask = buf(mask, want_mask, (P, H, W), torch.uint8, "mask")
    overlay = buf(overlay, want_overlay, (H, W, 3), torch.uint8, "overlay")
    stats = buf(stats, want_stats, (P, 5), torch.int32, "stats")
    K = 0
    if overlay is not None:
        if image is None or lut_inst is None or lut_cur is None:
            raise _lib.UllsamError("click_finish: an overlay needs image, lut_inst and lut_cur")
        _chk(image, "image", torch.uint8); _chk(lut_inst, "lut_inst", torch.uint8); _chk(lut_cur, "lut_cur", torch.uint8)
        assert tuple(image.shape) == (H, W, 3) and lut_inst.dim() == 3 and tuple(lut_inst.shape[1:]) == (3, 256) and tuple(lut_cur.shape) == (3, 256)
        K = int(lut_inst.shape[0])
    if canvas is not None:
        _chk(canvas, "canvas", torch.int32)
        assert tuple(canvas.shape) == (H, W), (canvas.shape, (H, W))
    scratch = torch.empty((5 * P + 1,), dtype=torch.int32, device=dev) if stats is not None else None
    _lib.call("ullsam_click_finish", low.data_ptr(), P, LH, LW, int(frame), H, W, side, int(top), int(left), float(thr),
              _p(image) if overlay is not None else None, _p(canvas), int(first_id), (1 if paint else 0) | (2 if highlight else 0),
              _p(lut_inst) if overlay is not None else None, K, _p(lut_cur) if overlay is not None else None, _p(mask), _p(overlay),
              _p(stats), _p(scratch), _stream())
    return mask, overlay, stats


# ---- prompts from an instance label image (csrc/prompts.hip) ----------------------------------------------------------------------
PROMPT_MAX_ID = 65535
PROMPT_MAX_RADIUS = 64
PROMPT_MAX_POINTS = 16


def label_d1(labels: torch.Tensor, radius: int, status: Optional[torch.Tensor] = None):
    """labels int32 [h, w] -> (d1 uint8 [h, w] = min(radius + 1, city-block distance to the nearest pixel with another label, the outside of the
    frame counting as another label); status int32 [1], set to 1 when a label lies outside 0..65535 -- the caller zeroes and reads it)."""
    _chk(labels, "labels", torch.int32)
    assert labels.dim() == 2
    h, w = labels.shape
    if not 0 <= int(radius) <= PROMPT_MAX_RADIUS:
        raise _lib.UllsamError(f"label_d1: radius {radius} is outside 0..{PROMPT_MAX_RADIUS}")
    scratch = torch.empty((h, w), dtype=torch.uint8, device=labels.device)
    d1 = torch.empty((h, w), dtype=torch.uint8, device=labels.device)
    if status is None:
        status = torch.zeros((1,), dtype=torch.int32, device=labels.device)
    else:
        _chk(status, "status", torch.int32)
    _lib.call("ullsam_label_d1", labels.data_ptr(), h, w, int(radius), scratch.data_ptr(), d1.data_ptr(), status.data_ptr(), _stream())
    return d1, status


def prompt_choose(areas: torch.Tensor, max_instances: int, seed: int, info: Optional[torch.Tensor] = None):
    """areas int32 [65536] (label_stats with n = 65535) -> (sel int32 [max_instances]: the present ids in increasing order, or max_instances of them
    by the draw rule when more are present; info int32 [2 + 4 * max_instances] with info[0] = how many were chosen)."""
    _chk(areas, "areas", torch.int32)
    assert areas.numel() == PROMPT_MAX_ID + 1
    m = int(max_instances)
    if not 1 <= m <= PROMPT_MAX_ID:
        raise _lib.UllsamError(f"prompt_choose: max_instances {m} is outside 1..{PROMPT_MAX_ID}")
    dev = areas.device
    present = torch.empty((PROMPT_MAX_ID,), dtype=torch.int32, device=dev)
    sorted_ = torch.empty((m,), dtype=torch.int32, device=dev)
    sel = torch.zeros((m,), dtype=torch.int32, device=dev)
    if info is None:
        info = torch.zeros((2 + 4 * m,), dtype=torch.int32, device=dev)
    else:
        _chk(info, "info", torch.int32)
        assert info.numel() >= 2 + 4 * m
    _lib.call("ullsam_prompt_choose", areas.data_ptr(), m, int(seed) % (1 << 64), present.data_ptr(), sorted_.data_ptr(), sel.data_ptr(),
              info.data_ptr(), _stream())
    return sel, info


def prompt_sets(labels: torch.Tensor, d1: torch.Tensor, areas: torch.Tensor, boxes_t: torch.Tensor, sel: torch.Tensor, info: torch.Tensor,
                radius: int, ring, debug: bool = False):
    """The interior and ring candidate sets of the slots s < info[0] (ids sel[s]) as bit rows -> (bits int64 [2, slots, h, ceil(w / 64)], rowcnt int32
    [2, slots, h], sums int64 [slots, 2] = (sum x, sum y) over the instance, dbg: None or (inner, ring) uint8 [slots, h, w]).  areas / boxes_t:
    label_stats(labels, 65535) -- the label image read as a transposed map, so a box there is (y0, x0, y1, x1).  The outputs are sized by the slots,
    used or not (h * ceil(w / 64) * 16 + h * 8 bytes each): utils.prompts bounds them before it calls."""
    for t, name, dt in ((labels, "labels", torch.int32), (d1, "d1", torch.uint8), (areas, "areas", torch.int32), (boxes_t, "boxes_t", torch.int32),
                        (sel, "sel", torch.int32), (info, "info", torch.int32)):
        _chk(t, name, dt)
    h, w = labels.shape
    slots = sel.numel()
    lo, hi = (int(v) for v in ring)
    assert d1.shape == labels.shape and areas.numel() == PROMPT_MAX_ID + 1 and boxes_t.numel() == 4 * (PROMPT_MAX_ID + 1) and info.numel() >= 2 + 4 * slots
    if not (0 <= int(radius) <= PROMPT_MAX_RADIUS and 0 <= lo <= hi <= PROMPT_MAX_RADIUS and 1 <= slots <= PROMPT_MAX_ID):
        raise _lib.UllsamError(f"prompt_sets: need 0 <= radius <= {PROMPT_MAX_RADIUS}, 0 <= ring[0] <= ring[1] <= {PROMPT_MAX_RADIUS} and 1..{PROMPT_MAX_ID} slots")
    dev = labels.device
    bits = torch.empty((2, slots, h, (w + 63) // 64), dtype=torch.int64, device=dev)
    rowcnt = torch.empty((2, slots, h), dtype=torch.int32, device=dev)
    sums = torch.empty((slots, 2), dtype=torch.int64, device=dev)
    dbg = (torch.empty((slots, h, w), dtype=torch.uint8, device=dev), torch.empty((slots, h, w), dtype=torch.uint8, device=dev)) if debug else None
    _lib.call("ullsam_prompt_sets", labels.data_ptr(), d1.data_ptr(), h, w, areas.data_ptr(), boxes_t.data_ptr(), sel.data_ptr(), info.data_ptr(), slots,
              int(radius), lo, hi, bits.data_ptr(), rowcnt.data_ptr(), sums.data_ptr(), _p(dbg[0]) if dbg else None, _p(dbg[1]) if dbg else None, _stream())
    return bits, rowcnt, sums, dbg


def prompt_points(hw, areas: torch.Tensor, boxes_t: torch.Tensor, sel: torch.Tensor, info: torch.Tensor, bits: torch.Tensor, rowcnt: torch.Tensor,
                  sums: torch.Tensor, hi: int, num_pos: int, num_neg: int, seed: int):
    """The points of every slot from its candidate sets (prompt_sets) by the draw rule -> (coords float32 [slots, num_pos + num_neg, 2] as (x, y),
    boxes float32 [slots, 4] XYXY inclusive, counts int32 [slots, 2] = (|inner|, |ring|)); info[2 + 4 s ..] = (id, area, |inner|, |ring|).  The
    negatives of a slot with |ring| < num_neg stay zero: the caller applies the fallbacks."""
    for t, name, dt in ((areas, "areas", torch.int32), (boxes_t, "boxes_t", torch.int32), (sel, "sel", torch.int32), (info, "info", torch.int32),
                        (bits, "bits", torch.int64), (rowcnt, "rowcnt", torch.int32), (sums, "sums", torch.int64)):
        _chk(t, name, dt)
    h, w = (int(v) for v in hw)
    slots = sel.numel()
    assert bits.shape == (2, slots, h, (w + 63) // 64) and rowcnt.shape == (2, slots, h) and sums.shape == (slots, 2) and info.numel() >= 2 + 4 * slots
    if not (0 <= int(num_pos) <= PROMPT_MAX_POINTS and 0 <= int(num_neg) <= PROMPT_MAX_POINTS and 0 <= int(hi) <= PROMPT_MAX_RADIUS):
        raise _lib.UllsamError(f"prompt_points: need num_pos, num_neg <= {PROMPT_MAX_POINTS} and ring[1] <= {PROMPT_MAX_RADIUS}")
    dev = sel.device
    coords = torch.zeros((slots, int(num_pos) + int(num_neg), 2), dtype=torch.float32, device=dev)
    boxes = torch.zeros((slots, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros((slots, 2), dtype=torch.int32, device=dev)
    _lib.call("ullsam_prompt_points", h, w, areas.data_ptr(), boxes_t.data_ptr(), sel.data_ptr(), info.data_ptr(), slots, int(hi), int(num_pos),
              int(num_neg), int(seed) % (1 << 64), bits.data_ptr(), rowcnt.data_ptr(), sums.data_ptr(), coords.data_ptr(), boxes.data_ptr(),
              counts.data_ptr(), _stream())
    return coords, boxes, counts


def instance_masks(labels: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """labels int32 [h, w], ids int32 [n] -> float32 [n, h, w] = (labels == ids[i])."""
    _chk(labels, "labels", torch.int32); _chk(ids, "ids", torch.int32)
    h, w = labels.shape
    n = ids.numel()
    assert n <= PROMPT_MAX_ID
    out = torch.empty((n, h, w), dtype=torch.float32, device=labels.device)
    _lib.call("ullsam_instance_masks", labels.data_ptr(), ids.data_ptr(), n, h * w, out.data_ptr(), _stream())
    return out


# ---- image preprocessing (csrc/imageprep.hip) --------------------------------------------------------------------------------------
AA_FILTERS = ("bilinear", "bicubic")
AA_BITS = 22
_AA_HOST = {}
_AA_DEV = {}


def _aa_filter(name: str, x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def aa_tables(in_size: int, out_size: int, filter: str = "bilinear"):
    """The bounds and coefficients of one axis of Pillow's 8-bit antialiased resize (Resample.c precompute_coeffs + normalize_coeffs_8bpc), in
    float64 on the host -> (bounds int32 [out, 2] = (first tap, tap count), coef int32 [out, ksize], taps past the count zero).  Cached per
    (in, out, filter).  in == out is the pass Pillow skips: the identity table (one tap of 2**22), which copies."""
    if filter not in AA_FILTERS:
        raise ValueError(f"filter must be one of {AA_FILTERS}, got {filter!r}")
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"aa_tables: sizes must be positive, got {in_size} -> {out_size}")
    key = (in_size, out_size, filter)
    hit = _AA_HOST.get(key)
    if hit is not None:
        return hit
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32)
        coef = np.full((out_size, 1), 1 << AA_BITS, np.int32)
    else:
        scale = in_size / out_size
        fs = max(scale, 1.0)
        support = (1.0 if filter == "bilinear" else 2.0) * fs
        ksize = int(np.ceil(support)) * 2 + 1
        ss = 1.0 / fs                                            # (Pillow multiplies by the reciprocal; a division differs in the last bit)
        center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
        xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
        n = xmax - xmin
        t = np.arange(ksize)
        w = _aa_filter(filter, (t[None, :] + xmin[:, None] - center[:, None] + 0.5) * ss)
        w[t[None, :] >= n[:, None]] = 0.0
        ww = np.zeros(out_size, np.float64)
        for j in range(ksize):                                   # the sum in index order, as the C loop forms it
            ww = ww + w[:, j]
        w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
        coef = np.where(w < 0, np.trunc(-0.5 + w * (1 << AA_BITS)), np.trunc(0.5 + w * (1 << AA_BITS))).astype(np.int32)
        bounds = np.stack([xmin, n], 1).astype(np.int32)
    if len(_AA_HOST) >= 64:
        _AA_HOST.clear()
    _AA_HOST[key] = (bounds, coef)
    return bounds, coef


def _aa_tables_dev(in_size: int, out_size: int, filter: str, tap_major: bool, device):
    """aa_tables on the device, uploaded once per (in, out, filter, layout, device): (bounds, coef, ksize); tap_major -> coef [ksize, out]."""
    key = (int(in_size), int(out_size), filter, bool(tap_major), str(device))
    hit = _AA_DEV.get(key)
    if hit is None:
        bounds, coef = aa_tables(in_size, out_size, filter)
        c = np.ascontiguousarray(coef.T if tap_major else coef)
        if len(_AA_DEV) >= 64:
            _AA_DEV.clear()
        hit = _AA_DEV[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(c).to(device), int(coef.shape[1]))
    return hit


def aa_row_span(in_size: int, out_size: int, filter: str = "bilinear"):
    """(first, count): the source rows the vertical pass reads -- all the horizontal pass has to compute."""
    bounds, _ = aa_tables(in_size, out_size, filter)
    first = int(bounds[:, 0].min())
    return first, int((bounds[:, 0] + bounds[:, 1]).max()) - first


def resize_u8_aa(src: torch.Tensor, out_hw, filter: str = "bilinear", window=None, lut: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, want_u8: bool = True):
    """Pillow's antialiased 8-bit resize (Image.resize, BILINEAR / BICUBIC), bit-exact.  src uint8 [H, W, C] or [H, W] with any non-negative
    strides (a planar [C, H, W] image is passed as chw.permute(1, 2, 0); a crop as a slice), C in {1, 3, 4}.
    window = (top, left, VH, VW): the image sits at (top, left) of a zero image of VH x VW, and that is what is resized (pad_to_square without the copy).
    -> (u8, f32): u8 uint8 [OH, OW, C] when want_u8; f32 when `lut` (float32 [3, 256]) is given: float32 [3, S_h >= OH, S_w >= OW] = `out` (a slot of a
    batch tensor; last stride 1) or a new [3, OH, OW], whose top-left OH x OW of plane c holds lut[c][value] -- the rest of `out` is left untouched."""
    if not src.is_cuda:
        raise _lib.UllsamError("src must live on the GPU (ullsam_amd has no CPU path)")
    if src.device.index != torch.cuda.current_device():
        raise _lib.UllsamError(f"src lives on {src.device} but the current device is cuda:{torch.cuda.current_device()}")
    if src.dtype != torch.uint8:
        raise TypeError(f"src must be torch.uint8, got {src.dtype}")
    if src.dim() == 2:
        src = src[:, :, None]
    if src.dim() != 3 or src.shape[2] not in (1, 3, 4) or src.shape[0] == 0 or src.shape[1] == 0 or min(src.stride()) < 0:
        raise ValueError(f"src must be a non-empty [H, W, C] image with C in (1, 3, 4) and non-negative strides, got shape {tuple(src.shape)}")
    IH, IW, C = (int(v) for v in src.shape)
    OH, OW = (int(v) for v in out_hw)
    top, left, VH, VW = (0, 0, IH, IW) if window is None else (int(v) for v in window)
    if not (OH > 0 and OW > 0 and top >= 0 and left >= 0 and top + IH <= VH and left + IW <= VW):
        raise _lib.UllsamError(f"resize_u8_aa: the image {(IH, IW)} at {(top, left)} does not lie inside the window {(VH, VW)}, or the output size {(OH, OW)} is empty")
    if lut is None and not want_u8:
        raise ValueError("resize_u8_aa: nothing to compute (want_u8=False and no lut)")
    dev = src.device
    bh, ch, kh = _aa_tables_dev(VW, OW, filter, True, dev)
    bv, cv, kv = _aa_tables_dev(VH, OH, filter, False, dev)
    row0, rows = aa_row_span(VH, OH, filter)
    f32 = None
    if lut is not None:
        _chk(lut, "lut", torch.float32)
        if tuple(lut.shape) != (3, 256):
            raise ValueError(f"lut must be [3, 256], got {tuple(lut.shape)}")
        if out is None:
            f32 = torch.empty((3, OH, OW), dtype=torch.float32, device=dev)
        else:
            if not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == 3 and out.shape[1] >= OH
                    and out.shape[2] >= OW and out.stride(2) == 1 and out.stride(1) >= out.shape[2] and out.stride(0) >= 0):
                raise ValueError(f"out must be a float32 [3, >= {OH}, >= {OW}] tensor on {dev} with unit last stride, got {tuple(out.shape)} {out.dtype}")
            f32 = out
    elif out is not None:
        raise ValueError("resize_u8_aa: `out` is the float output and needs `lut`")
    u8 = torch.empty((OH, OW, C), dtype=torch.uint8, device=dev) if want_u8 else None
    tmp = torch.empty((rows, OW, C), dtype=torch.uint8, device=dev)
    _lib.call("ullsam_resize_u8_aa_h", src.data_ptr(), src.stride(0), src.stride(1), src.stride(2), IH, IW, C, top, left, VH, VW, row0, rows,
              bh.data_ptr(), ch.data_ptr(), kh, OW, tmp.data_ptr(), _stream())
    _lib.call("ullsam_resize_u8_aa_v", tmp.data_ptr(), row0, rows, OW, C, bv.data_ptr(), cv.data_ptr(), kv, OH, _p(u8), _p(lut), _p(f32),
              f32.stride(0) if f32 is not None else 0, f32.stride(1) if f32 is not None else 0, _stream())
    return u8, f32


def normalize_to_u8(x: torch.Tensor) -> torch.Tensor:
    """((x - x.min()) / (x.max() - x.min() + 1e-8) * 255).astype(np.uint8) (app.py:190-191) with numpy's types: a uint16 tensor takes the difference
    in uint16 and the quotient and product in float64; a float32 tensor does every step in float32.  -> uint8, same shape.  NaN inputs are out
    of scope (numpy's min / max propagate them; the integer keys here do not)."""
    kind = {torch.uint16: "u16", torch.float32: "f32"}.get(x.dtype)
    if kind is None:
        raise TypeError(f"normalize_to_u8 takes uint16 or float32, got {x.dtype}")
    _chk(x, "x")
    if x.numel() == 0:
        raise ValueError("normalize_to_u8: empty input")
    mm = torch.empty((2,), dtype=torch.int32, device=x.device)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.call(f"ullsam_minmax_{kind}", x.data_ptr(), x.numel(), mm.data_ptr(), _stream())
    _lib.call(f"ullsam_normalize_to_u8_{kind}", x.data_ptr(), x.numel(), mm.data_ptr(), out.data_ptr(), _stream())
    return out
