"""Activations as K-panels (packing.pack_activation_panels; csrc/gemm.hip gemm_ring8_kernel / launch_ring, csrc/gemm_ring8p.h, csrc/norm.hip): a ring GEMM that reads
its A as panels, or writes its 2-byte C as panels, and a norm that writes panels, against the same launches row-major.  Only addresses change -- same lanes, same bytes,
same LDS image, same MFMA order, same arithmetic -- so every comparison is EQUALITY in bits; each base result is also held against the fp32 matmul with the tolerances
of tests/test_ring_panels_gpu.py, whose case table (the smallest shapes that reach each kernel) is reused."""
import ctypes

import pytest
import torch

from oracle import ullsam_oracle as O
from tests import gemm_ref as R
from tests.test_ring_panels_gpu import CASES, _operands

pytestmark = pytest.mark.gpu
DEV = "cuda"
PERSIST_DEFAULT, PANELS_DEFAULT, ACT_PANELS_DEFAULT = 2, 1, 1   # csrc/gemm.hip g_persist, g_ring_panels, g_act_panels
NAN_BITS = 0x7FC1                                               # a bf16 NaN pattern (as int16: 32705)


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as _ops
    return _ops


def _lib_():
    from ullsam_amd import _lib
    return _lib.load()


def _query(M, N, K, act=0, out_f32=False, bias=False, res=False, rope=False):
    ra, wc = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib_().ullsam_gemm_act_panels_query(R.DT_BF16, M, N, K, 4 if rope else act, int(out_f32), int(bias), int(res), 1, 128 << 20, ctypes.addressof(ra), ctypes.addressof(wc)) == 0
    return bool(ra.value), bool(wc.value)


def _poisoned(x):
    """x as panels with the padding rows (M .. the next multiple of 16) filled with NaN bit patterns."""
    from ullsam_amd.packing import pack_activation_panels
    M, K = x.shape
    p = pack_activation_panels(x)
    Mp = p.shape[0]
    if Mp != M:
        v = p.view(Mp // 16, K // 32, 16, 32)
        v[-1, :, M % 16:, :] = torch.tensor(NAN_BITS, dtype=torch.int16, device=x.device).view(torch.bfloat16)
    return p


def _run(ops, mode, a, w, bias, x0, wpan, ap, cp):
    """-> (output [M, N'] row-major fp32-or-bf16, reference from the fp32 matmul, tolerance).  wpan: weight panels too; ap / cp: A read / C written as panels."""
    from ullsam_amd.packing import pack_ring_panels, pack_w13, unpack_activation_panels
    F = torch.nn.functional
    M, N = a.shape[0], w.shape[0]
    ref = a.float() @ w.float().T
    A = _poisoned(a) if ap else a
    kw = dict(a_panels=ap, m=M)
    un = lambda y: unpack_activation_panels(y, M) if cp else y
    wp = lambda t: pack_ring_panels(t) if wpan else None
    if mode == "plain":
        return un(ops.gemm(A, w, w_panels=wp(w), out_panels=cp, **kw)), ref, 3e-2
    if mode == "bias":
        return un(ops.gemm(A, w, bias, w_panels=wp(w), out_panels=cp, **kw)), ref + bias, 3e-2
    if mode == "bias_gelu":
        return un(ops.gemm(A, w, bias, act=ops.ACT_GELU, w_panels=wp(w), out_panels=cp, **kw)), F.gelu(ref + bias), 3e-2
    if mode == "res":
        x = x0.clone()
        ops.gemm(A, w, bias, residual=x, out_f32=True, out=x, w_panels=wp(w), **kw)
        return x, ref + bias + x0, 2e-3
    if mode == "res_mod":
        pe = x0[:M // 2].contiguous()
        return ops.gemm(A, w, bias, residual=pe, res_row_mod=M // 2, out_f32=True, w_panels=wp(w), **kw), ref + bias + pe.repeat(2, 1), 2e-3
    assert mode == "swiglu"
    I = N // 2
    w13 = pack_w13(w[:I].contiguous(), w[I:].contiguous())
    return un(ops.gemm(A, w13, act=ops.ACT_SWIGLU, w_panels=wp(w13), out_panels=cp, **kw)), F.silu(ref[:, :I]) * ref[:, I:], 3e-2


@pytest.mark.parametrize("persist", [2, 0])
@pytest.mark.parametrize("variant,M,N,K,mode", CASES)
def test_ring_gemm_on_activation_panels_equals_row_major(ops, variant, M, N, K, mode, persist):
    """Both ring kernels (ullsam_set_gemm_tuning(2, 0) = one tile per workgroup), every direct epilogue: A as panels, C as panels (the 2-byte epilogues: plain, bias, bias + GELU
    on the 320-wide tile, SwiGLU), both at once, with the weight as panels and row-major -- all equal the row-major launch in bits.  Ragged M (4324, 6000, 8000): the padding rows
    of A hold NaN patterns and no NaN may come out.  A zero matrix handed over as panels must zero the result with the switch on and is refused with it off."""
    from ullsam_amd import _lib
    from ullsam_amd.packing import pack_activation_panels
    lib = _lib_()
    a, w, bias, x0 = _operands(M, N, K, M + N + K + variant)
    two_byte = mode in ("plain", "bias", "bias_gelu", "swiglu")
    got = {}
    try:
        lib.ullsam_set_gemm_variant(variant)
        lib.ullsam_set_gemm_tuning(2, persist)
        can_a, can_c = _query(M, N, K, act={"bias_gelu": 1, "swiglu": 3}.get(mode, 0), out_f32=not two_byte, bias=mode not in ("plain", "swiglu"), res=not two_byte)
        assert can_a and can_c == two_byte, (can_a, can_c)
        base, want, tol = _run(ops, mode, a, w, bias, x0, False, False, False)
        for wpan in (False, True):
            got[("a", wpan)] = _run(ops, mode, a, w, bias, x0, wpan, True, False)[0]
            if two_byte:
                got[("c", wpan)] = _run(ops, mode, a, w, bias, x0, wpan, False, True)[0]
                got[("ac", wpan)] = _run(ops, mode, a, w, bias, x0, wpan, True, True)[0]
        if mode == "plain":
            zeros = pack_activation_panels(torch.zeros_like(a))
            read = ops.gemm(zeros, w, a_panels=True, m=M).float()
            lib.ullsam_set_gemm_tuning(5, 0)
            off = ops.gemm(a, w)
            with pytest.raises(_lib.UllsamError):     # the switch off: the parent's launches, and a panel buffer is never read as row-major
                ops.gemm(zeros, w, a_panels=True, m=M)
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_gemm_variant(0)
        lib.ullsam_set_gemm_tuning(2, PERSIST_DEFAULT)
        lib.ullsam_set_gemm_tuning(5, ACT_PANELS_DEFAULT)
    err = float((base.float() - want).abs().max())
    print(f"max abs err vs fp32 matmul {err:.3e} (bound {tol * max(1.0, float(want.abs().max()) / 4):.3e})")
    assert err < tol * max(1.0, float(want.abs().max()) / 4)
    for key, y in got.items():
        assert not bool(torch.isnan(y).any()), key
        assert torch.equal(y, base), (key, int((y != base).sum()))
    if mode == "plain":
        assert float(read.abs().max()) == 0.0
        assert torch.equal(off, base)


@pytest.mark.parametrize("persist", [2, 0])
@pytest.mark.parametrize("B,S,KVH,G,K,variant", [(2, 1500, 8, 4, 512, 9), (3, 1202, 8, 4, 1024, 6), (2, 1500, 8, 2, 512, 0)])
def test_rope_gemm_reading_activation_panels_equals_row_major(ops, B, S, KVH, G, K, variant, persist):
    """wqkv + head split + RoPE + KV-cache append in the epilogue reading x as panels (padding rows NaN where B S is ragged: 3 x 1202 = 3606): q, the appended K / V rows and the
    untouched cache rows equal in bits; q against the float64 definition."""
    import numpy as np
    from ullsam_amd.packing import pack_ring_panels
    lib = _lib_()
    hd = 128
    g = torch.Generator(device=DEV); g.manual_seed(B * S + K + G)
    x = torch.randn(B * S, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(KVH * (G + 2) * hd, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    pos = ((torch.arange(S, device=DEV, dtype=torch.int32)[None] + 3 * torch.arange(B, device=DEV, dtype=torch.int32)[:, None]) % (S + 5)).contiguous()
    cos, sin = O.rope_tables(hd, S + 8, 1e6)
    cos, sin = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV).float().contiguous() for t in (cos, sin))
    cap, p0 = S + 6, 2
    res = {}
    try:
        lib.ullsam_set_gemm_variant(variant)
        lib.ullsam_set_gemm_tuning(2, persist)
        assert _query(B * S, w.shape[0], K, rope=True) == (True, False)
        for name, xx, ap, wp in (("rows", x, False, None), ("panels", _poisoned(x), True, None), ("both", _poisoned(x), True, pack_ring_panels(w))):
            kc = torch.full((B, KVH, cap, hd), 0.25, dtype=torch.bfloat16, device=DEV); vc = torch.full_like(kc, -0.5)
            q = ops.gemm_qkv_rope(xx, w, None, kc, vc, pos, cos, sin, B, S, KVH, G, p0, w_panels=wp, a_panels=ap)
            res[name] = (q, kc, vc)
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_gemm_variant(0)
        lib.ullsam_set_gemm_tuning(2, PERSIST_DEFAULT)
    for name in ("panels", "both"):
        for u, v in zip(res["rows"], res[name]):
            assert not bool(torch.isnan(v).any())
            assert torch.equal(u, v), (name, int((u != v).sum()))
    qkv = (x.double() @ w.double().T).view(B * S, KVH, G + 2, hd)[:, :, :G]
    c, s_ = cos.double()[pos.reshape(-1).long()][:, None, None, :], sin.double()[pos.reshape(-1).long()][:, None, None, :]
    rot = torch.cat([-qkv[..., hd // 2:], qkv[..., :hd // 2]], -1)
    want = (qkv * c + rot * s_).reshape(B * S, KVH * G * hd)
    err = float((res["rows"][0].double() - want).abs().max())
    print(f"q max abs err vs float64 {err:.3e}")
    assert err < 3e-2 * max(1.0, float(want.abs().max()) / 4)


@pytest.mark.parametrize("rows", [100, 4324])
@pytest.mark.parametrize("D,rms,variant", [(4096, True, 0), (4096, True, 1), (1280, False, 0), (384, False, 0)])
def test_norm_writes_panels_with_the_row_major_bits(ops, rows, D, rms, variant):
    """RMSNorm at D = 4096 through norm_block_kernel (4324 rows: launch_norm gives it rows of >= 2048 elements from 1024 rows up) and through norm_kernel (100 rows, and
    4324 under ullsam_set_norm_variant(1)), LayerNorm at D = 1280 and 384 (norm_kernel): the panel output unpacked equals the row-major output in bits, and the row-major
    output is one bf16 rounding away from the float64 definition."""
    from ullsam_amd.packing import unpack_activation_panels
    lib = _lib_()
    g = torch.Generator(device=DEV); g.manual_seed(rows + D)
    x = torch.randn(rows, D, device=DEV, generator=g) * 3 + 0.5
    w = torch.randn(D, device=DEV, generator=g)
    b = None if rms else torch.randn(D, device=DEV, generator=g)
    try:
        lib.ullsam_set_norm_variant(variant)
        base = ops.norm(x, w, b, 1e-6, torch.bfloat16, rms=rms)
        pan = ops.norm(x, w, b, 1e-6, torch.bfloat16, rms=rms, out_panels=True)
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_norm_variant(0)
    assert pan.shape == ((rows + 15) // 16 * 16, D) and pan.data_ptr() % 1024 == 0
    assert torch.equal(unpack_activation_panels(pan, rows), base)
    xf = x.double()
    want = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-6) * w.double() if rms else torch.nn.functional.layer_norm(xf, (D,), w.double(), b.double(), 1e-6)
    assert float((base.double() - want).abs().max()) < 2 ** -8 * max(1.0, float(want.abs().max()))   # one bf16 rounding (2^-9 relative) of an fp32 result


@pytest.mark.parametrize("persist", [2, 0])
@pytest.mark.parametrize("kind,M,D,I", [("swiglu", 4324, 4096, 2048), ("gelu", 16384, 1280, 2560)])
def test_chain_norm_gemm_residual_gemm_on_panels_equals_row_major(ops, kind, M, D, I, persist):
    """norm -> GEMM (SwiGLU on 272x256 tiles / bias + GELU on 256x320 tiles) -> residual GEMM: every intermediate travels as panels, written by its producer; the fp32 residual
    stream at the end equals the row-major chain in bits."""
    from ullsam_amd.packing import pack_w13
    lib = _lib_()
    g = torch.Generator(device=DEV); g.manual_seed(M + D + I)
    x0 = torch.randn(M, D, device=DEV, generator=g)
    nw, nb = torch.randn(D, device=DEV, generator=g), torch.randn(D, device=DEV, generator=g)
    swiglu = kind == "swiglu"
    w1 = (torch.randn(2 * I if swiglu else I, D, device=DEV, generator=g) * D ** -0.5).bfloat16()
    if swiglu:
        w1 = pack_w13(w1[:I].contiguous(), w1[I:].contiguous())
    b1 = None if swiglu else torch.randn(I, device=DEV, generator=g)
    w2 = (torch.randn(D, I, device=DEV, generator=g) * I ** -0.5).bfloat16()
    b2 = torch.randn(D, device=DEV, generator=g)
    act = ops.ACT_SWIGLU if swiglu else ops.ACT_GELU
    out = {}
    try:
        lib.ullsam_set_gemm_tuning(2, persist)
        ap, cp = _query(M, w1.shape[0], D, act=act, bias=b1 is not None)
        hp, _ = _query(M, D, I, out_f32=True, bias=True, res=True)
        assert ap and cp and hp
        for name, on in (("rows", False), ("panels", True)):
            x = x0.clone()
            xn = ops.norm(x, nw, None if swiglu else nb, 1e-6, torch.bfloat16, rms=swiglu, out_panels=on)
            h = ops.gemm(xn, w1, b1, act=act, a_panels=on, out_panels=on, m=M)
            ops.gemm(h, w2, b2, residual=x, out_f32=True, out=x, a_panels=on, m=M)
            out[name] = x
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_gemm_tuning(2, PERSIST_DEFAULT)
    assert not bool(torch.isnan(out["panels"]).any())
    assert torch.equal(out["rows"], out["panels"]), int((out["rows"] != out["panels"]).sum())


def test_declined_launches_get_row_major_buffers_and_the_old_result(ops):
    """K = 48 k shapes (no 32-deep panels ... the layout needs K % 32 == 0; the GEMM itself K % 64) and M = 1081 on the 128x128 kernel: ops.activation_panels_plan says no,
    the producers write row-major and the result is the old one; a flag forced onto such a launch is refused."""
    from ullsam_amd import _lib
    with torch.no_grad():
        assert ops.activation_panels_plan(1081, 4096, 4096, torch.bfloat16) == (False, False)
        assert ops.activation_panels_plan(4324, 4096, 4096, torch.float32) == (False, False)
        assert ops.activation_panels_plan(4324, 4096, 4096, torch.bfloat16) == (True, True)
        with torch.enable_grad():
            assert ops.activation_panels_plan(4324, 4096, 4096, torch.bfloat16) == (False, False)
        try:
            ops.set_activation_panels(False)
            assert ops.activation_panels_plan(4324, 4096, 4096, torch.bfloat16) == (False, False)
        finally:
            ops.set_activation_panels(True)
        for M, N, K in ((1081, 512, 384), (4096, 4096, 48 * 4)):
            a, w, bias, _ = _operands(M, N, K, M + K)
            ap, cp = ops.activation_panels_plan(M, N, K, torch.bfloat16, bias=True)
            if M == 1081:
                assert (ap, cp) == (False, False)
                with pytest.raises(_lib.UllsamError):
                    ops.gemm(ops.empty_activation_panels(M, K, DEV), w, bias, a_panels=True, m=M)
            y = ops.gemm(a, w, bias, a_panels=False, out_panels=False, m=M)
            assert y.shape == (M, N) and torch.equal(y, ops.gemm(a, w, bias))
            err = float((y.float() - (a.float() @ w.float().T + bias)).abs().max())
            assert err < 3e-2 * max(1.0, float(y.float().abs().max()) / 4)
    torch.cuda.synchronize()


def test_model_blocks_with_the_switch_on_and_off_are_equal(ops):
    """One pair of ViT-H blocks (windowed + global, 4096 tokens) and one LLM layer (4 x 1081 rows, hidden 1024) -- shapes at which qkv / lin1 / wqkv / w13 reach the ring
    kernels and lin2 / w2 do not (their inputs stay row-major): the switch on and off give equal outputs, and with it on the plan really says yes for those launches."""
    from tests import util as U
    from tests.test_model_gpu import make_vit
    from ullsam_amd.modeling.configuration_internlm2 import InternLM2Config
    from ullsam_amd.modeling.modeling_internlm2 import InternLM2Model
    torch.manual_seed(3)
    with torch.no_grad():
        with torch.device(DEV):
            vit = make_vit(U.VIT_H_D2).to(torch.bfloat16).eval()
            cfg = InternLM2Config(vocab_size=64, hidden_size=1024, intermediate_size=3072, num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=2, bias=False,
                                  max_position_embeddings=32768, rope_theta=1000000.0, rms_norm_eps=1e-5)
            llm = InternLM2Model(cfg).to(torch.bfloat16).eval()
        img = torch.from_numpy(U.rand_image((1, 3, 1024, 1024), 5)).to(DEV)
        B, S = 4, 1081
        emb = torch.randn(B * S, 1024, device=DEV) * 0.5
        pos = torch.arange(S, device=DEV, dtype=torch.int32).repeat(B, 1).contiguous()
        assert ops.activation_panels_plan(4096, 3 * 1280, 1280, torch.bfloat16, bias=True)[0]
        assert ops.activation_panels_plan(4096, 5120, 1280, torch.bfloat16, act=ops.ACT_GELU, bias=True) == (True, True)
        assert ops.activation_panels_plan(B * S, 1536, 1024, torch.bfloat16, rope=True)[0]
        assert ops.activation_panels_plan(B * S, 6144, 1024, torch.bfloat16, act=ops.ACT_SWIGLU) == (True, True)
        res = {}
        try:
            for on in (True, False):
                ops.set_activation_panels(on)
                res[on] = (vit.forward_tokens(img), llm.run_layers(emb.clone(), B, S, pos, None, None))
            torch.cuda.synchronize()
        finally:
            ops.set_activation_panels(True)
    for u, v in zip(res[True], res[False]):
        assert not bool(torch.isnan(u.float()).any())
        assert torch.equal(u, v), int((u != v).sum())
