"""The ring GEMM kernels reading their weight as K-panels (packing.pack_ring_panels; csrc/gemm.hip gemm_ring8_kernel / launch_ring, csrc/gemm_ring8p.h) against the
same launches on the row-major weight: the panels change the addresses the weight requests read from and nothing else -- same LDS image, same MFMA order, same
epilogues -- so the outputs must be EQUAL bit for bit; each case is also held against the fp32 matmul with the tolerances of
tests/test_kernels_gpu.py::test_gemm_persistent_ring_equals_the_one_tile_kernel, whose case table (the smallest shapes that reach each kernel) is reused here."""
import numpy as np
import pytest
import torch

from oracle import ullsam_oracle as O
from tests import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PERSIST_DEFAULT, PANELS_DEFAULT = 2, 1   # csrc/gemm.hip g_persist, g_ring_panels


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as _ops
    return _ops


def _lib_():
    from ullsam_amd import _lib
    return _lib.load()


def _operands(M, N, K, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    a = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    bias = torch.randn(N, device=DEV, generator=g)
    x0 = torch.randn(M, N, device=DEV, generator=g)
    return a, w, bias, x0


def _run(ops, mode, a, w, bias, x0, wp):
    """-> (output fp32, reference from the fp32 matmul, tolerance) of one epilogue mode; wp = the weight as panels, or None for the row-major launch."""
    from ullsam_amd.packing import pack_ring_panels, pack_w13
    F = torch.nn.functional
    M, N = a.shape[0], w.shape[0]
    ref = a.float() @ w.float().T
    if mode == "plain":
        return ops.gemm(a, w, w_panels=wp).float(), ref, 3e-2
    if mode == "bias":
        return ops.gemm(a, w, bias, w_panels=wp).float(), ref + bias, 3e-2
    if mode == "bias_gelu":
        return ops.gemm(a, w, bias, act=ops.ACT_GELU, w_panels=wp).float(), F.gelu(ref + bias), 3e-2
    if mode == "res":
        x = x0.clone()
        ops.gemm(a, w, bias, residual=x, out_f32=True, out=x, w_panels=wp)
        return x, ref + bias + x0, 2e-3
    if mode == "res_mod":
        pe = x0[:M // 2].contiguous()
        return ops.gemm(a, w, bias, residual=pe, res_row_mod=M // 2, out_f32=True, w_panels=wp), ref + bias + pe.repeat(2, 1), 2e-3
    assert mode == "swiglu"
    I = N // 2
    w13 = pack_w13(w[:I].contiguous(), w[I:].contiguous())
    return ops.gemm(a, w13, act=ops.ACT_SWIGLU, w_panels=None if wp is None else pack_ring_panels(w13)).float(), F.silu(ref[:, :I]) * ref[:, I:], 3e-2


# variant 9 / 8 / 6 = 272x256 / 256x320 / 256x256 tiles; more than 256 tiles each (the persistent kernel takes them), ragged M, K from 128 * 3 (the shortest the ring accepts:
# the last trip's next-tile offsets are those of the first) -- then two launches of ONE round (at most 256 tiles: the one-tile kernel whatever the switch says)
CASES = [(9, 4324, 8192, 384, "swiglu"), (9, 8704, 4096, 512, "res"), (8, 8192, 3840, 384, "bias_gelu"), (8, 8000, 3840, 640, "res_mod"),
         (6, 8192, 4096, 384, "bias"), (6, 6000, 6144, 1024, "plain"),
         (9, 4324, 4096, 512, "res"), (8, 4096, 1280, 384, "res")]


@pytest.mark.parametrize("persist", [2, 0])
@pytest.mark.parametrize("variant,M,N,K,mode", CASES)
def test_ring_gemm_on_panels_equals_row_major(ops, variant, M, N, K, mode, persist):
    """Every direct epilogue on both ring kernels (ullsam_set_gemm_tuning(2, 0) = one tile per workgroup): panels == row-major in bits, both within the fp32 matmul's tolerance.
    A weight of zeros handed over as `panels` must change the result -- the launch really read the panels -- and must not with the switch off."""
    from ullsam_amd.packing import pack_ring_panels
    lib = _lib_()
    a, w, bias, x0 = _operands(M, N, K, M + N + K + variant)
    try:
        lib.ullsam_set_gemm_variant(variant)
        lib.ullsam_set_gemm_tuning(2, persist)
        base, want, tol = _run(ops, mode, a, w, bias, x0, None)
        got, _, _ = _run(ops, mode, a, w, bias, x0, pack_ring_panels(w))
        if mode == "plain":
            zeros = pack_ring_panels(torch.zeros_like(w))
            read = ops.gemm(a, w, w_panels=zeros).float()
            lib.ullsam_set_gemm_tuning(4, 0)
            off = ops.gemm(a, w, w_panels=zeros).float()
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_gemm_variant(0)
        lib.ullsam_set_gemm_tuning(2, PERSIST_DEFAULT)
        lib.ullsam_set_gemm_tuning(4, PANELS_DEFAULT)
    err = float((base - want).abs().max())
    print(f"max abs err vs fp32 matmul {err:.3e} (bound {tol * max(1.0, float(want.abs().max()) / 4):.3e})")
    assert err < tol * max(1.0, float(want.abs().max()) / 4)
    assert torch.equal(got, base), int((got != base).sum())
    if mode == "plain":
        assert float(read.abs().max()) == 0.0
        assert torch.equal(off, base)


@pytest.mark.parametrize("persist", [2, 0])
@pytest.mark.parametrize("B,S,KVH,G,K,variant", [(2, 1500, 8, 4, 512, 9), (3, 1200, 8, 4, 1024, 6), (2, 1500, 8, 2, 512, 0)])
def test_rope_gemm_on_panels_equals_row_major(ops, B, S, KVH, G, K, variant, persist):
    """wqkv + head split + RoPE + KV-cache append in the epilogue: q, the appended K / V rows and the untouched cache rows equal in bits; q against the float64 definition."""
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
        for name, wp in (("rows", None), ("panels", pack_ring_panels(w))):
            kc = torch.full((B, KVH, cap, hd), 0.25, dtype=torch.bfloat16, device=DEV); vc = torch.full_like(kc, -0.5)
            q = ops.gemm_qkv_rope(x, w, None, kc, vc, pos, cos, sin, B, S, KVH, G, p0, w_panels=wp)
            res[name] = (q, kc, vc)
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_gemm_variant(0)
        lib.ullsam_set_gemm_tuning(2, PERSIST_DEFAULT)
    for u, v in zip(res["rows"], res["panels"]):
        assert torch.equal(u, v), int((u != v).sum())
    # float64: qkv = x w^T, head slot (kv, g) of 128 columns; q slots rotated: out = t cos + rotate_half(t) sin
    qkv = (x.double() @ w.double().T).view(B * S, KVH, G + 2, hd)[:, :, :G]
    c, s_ = cos.double()[pos.reshape(-1).long()][:, None, None, :], sin.double()[pos.reshape(-1).long()][:, None, None, :]
    rot = torch.cat([-qkv[..., hd // 2:], qkv[..., :hd // 2]], -1)
    want = (qkv * c + rot * s_).reshape(B * S, KVH * G * hd)
    err = float((res["panels"][0].double() - want).abs().max())
    print(f"q max abs err vs float64 {err:.3e}")
    assert err < 3e-2 * max(1.0, float(want.abs().max()) / 4)


def test_launches_the_panels_do_not_fit_read_the_row_major_weight(ops):
    """launch_ring keeps the panels only for whole tiles of a contiguous weight; odd M and K < 384 leave the persistent kernel.  Every one equals the row-major launch
    (where the layout is not defined, even with zeros handed over as panels: they are not read)."""
    from ullsam_amd import _lib
    from ullsam_amd.packing import pack_ring_panels
    lib = _lib_()
    try:
        lib.ullsam_set_gemm_variant(6)
        # N % BN != 0: 4224 = 16.5 tiles of 256 columns
        a, w, bias, _ = _operands(4096, 4224, 384, 1)
        assert torch.equal(ops.gemm(a, w, bias, w_panels=pack_ring_panels(torch.zeros_like(w))), ops.gemm(a, w, bias))
        # a strided weight (ldw > K): through the entry point itself, ops.gemm only takes dense operands
        a, w, bias, _ = _operands(4096, 4096, 384, 2)
        M, N, K = 4096, 4096, 384
        wb, wptr = R.padded(w, K + 64)
        zeros = pack_ring_panels(torch.zeros_like(w))
        out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        ws = R.workspace(DEV)
        _lib.call("ullsam_gemm_panels", R.DT_BF16, a.data_ptr(), K, wptr, K + 64, zeros.data_ptr(), out.data_ptr(), N, 0, bias.data_ptr(), None, 0, 0, 0, M, N, K,
                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert torch.equal(out, ops.gemm(a, w, bias))
        # odd M (no direct epilogue: the one-tile kernel's staged one) and K < 384 (the persistent kernel declines): the layout is defined, the result the same
        for M, K in ((4097, 384), (8192, 256)):
            a, w, bias, _ = _operands(M, 4096, K, M + K)
            assert torch.equal(ops.gemm(a, w, bias, w_panels=pack_ring_panels(w)), ops.gemm(a, w, bias))
        torch.cuda.synchronize()
    finally:
        lib.ullsam_set_gemm_variant(0)
    with pytest.raises(_lib.UllsamError):   # fp32 has no panels
        a32 = torch.zeros(1024, 256, device=DEV)
        _lib.call("ullsam_gemm_panels", R.DT_F32, a32.data_ptr(), 256, a32.data_ptr(), 256, a32.data_ptr(), a32.data_ptr(), 1024, 1, None, None, 0, 0, 0, 1024, 1024, 256,
                  None, 0, torch.cuda.current_stream().cuda_stream)


def test_an_in_place_weight_update_repacks(ops):
    """Linear caches the panels per weight version: after an in-place update the output follows the NEW weight and equals the row-major launch; under autograd no copy is built."""
    from ullsam_amd.modeling.common import Linear
    lin = Linear(512, 4096).to(DEV).to(torch.bfloat16)
    g = torch.Generator(device=DEV); g.manual_seed(5)
    x = torch.randn(8192, 512, device=DEV, generator=g).bfloat16()
    assert lin.wp(torch.bfloat16, 8192) is None                       # grad mode + a trainable weight: the row-major path
    with torch.no_grad():
        assert lin.wp(torch.bfloat16, 4) is None                      # a decode step's rows never reach a ring kernel
        y1 = lin(x)
        p1 = lin.wp(torch.bfloat16, 8192)
        assert p1 is not None and p1 is lin.wp(torch.bfloat16, 8192)  # built once
        assert torch.equal(y1, ops.gemm(x, lin.weight.detach(), lin.b()))
        lin.weight.mul_(-2.0)
        y2 = lin(x)
        p2 = lin.wp(torch.bfloat16, 8192)
        assert p2 is not p1
        assert torch.equal(y2, ops.gemm(x, lin.weight.detach(), lin.b())) and not torch.equal(y2, y1)
    torch.cuda.synchronize()
