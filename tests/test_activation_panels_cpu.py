"""Activation K-panels on the host (packing.pack_activation_panels; csrc/gemm_ring8p.h has the layout): the index formula, the round trip with ragged row counts,
the refusals, the new exports' arity, and -- without a GPU, as tests/test_gemm_abi_cpu.py does it -- the query's answers and the refusal BEFORE any launch of a
call that carries a panel flag and whose dispatch does not reach a ring kernel."""
import ctypes
import os
import re

import pytest
import torch

from tests import gemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ullsam_gemm_act_panels", "ullsam_gemm_qkv_rope_act_panels", "ullsam_gemm_act_panels_query", "ullsam_norm_panels")
P = 1 << 20     # a 1 KiB aligned dummy address: never dereferenced, every check below comes before the first HIP call


@pytest.fixture(scope="module")
def lib():
    from ullsam_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("M,K", [(100, 64), (4324, 128), (16, 32), (33, 96)])
def test_index_formula_and_round_trip(M, K):
    from ullsam_amd.packing import pack_activation_panels, unpack_activation_panels
    x = (torch.arange(M * K, dtype=torch.float32) % 251 - 125).reshape(M, K).bfloat16()   # exact in bf16, every (row, k) told apart from its neighbours
    p = pack_activation_panels(x)
    Mp = (M + 15) // 16 * 16
    assert p.shape == (Mp, K) and p.dtype == torch.bfloat16 and p.data_ptr() % 1024 == 0
    flat = p.reshape(-1).float().tolist()
    xs = x.float().tolist()
    step = 1 if M * K <= 16384 else 7                                                        # a plain loop over (a stride of) the elements
    for i in range(0, M * K, step):
        r, k = divmod(i, K)
        assert flat[((r // 16) * (K // 32) + k // 32) * 512 + (r % 16) * 32 + k % 32] == xs[r][k], (r, k)
    assert torch.equal(unpack_activation_panels(p, M), x)
    if Mp != M:   # the host packer zeroes the padding rows (a producer kernel leaves them unwritten)
        assert float(unpack_activation_panels(p, Mp)[M:].float().abs().max()) == 0.0


def test_refusals_of_the_host_packers():
    from ullsam_amd.packing import empty_activation_panels, pack_activation_panels, unpack_activation_panels
    for bad in (torch.zeros(32, 64), torch.zeros(32, 64, dtype=torch.float16), torch.zeros(32, 48, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            pack_activation_panels(bad)
    with pytest.raises(ValueError):
        empty_activation_panels(100, 48, "cpu")
    with pytest.raises(ValueError):
        unpack_activation_panels(torch.zeros(112, 64, dtype=torch.bfloat16), 90)             # 90 rows pad to 96, not 112
    assert empty_activation_panels(100, 64, "cpu").shape == (112, 64)


def test_header_arity_of_the_new_exports_and_abi_version(lib):
    from ullsam_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ullsam_hip.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
    assert lib.ullsam_abi_version() == _lib.ABI_VERSION == 14
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", src).group(1)) == 14
    # ... and the existing signatures the flags ride beside are what they were
    assert len(_lib.SIGNATURES["ullsam_gemm_panels"]) == 20 and len(_lib.SIGNATURES["ullsam_gemm_qkv_rope_panels"]) == 24 and len(_lib.SIGNATURES["ullsam_norm"]) == 16


def _query(lib, M, N, K, act=0, out_f32=0, bias=0, res=0, aligned=1, ws=128 << 20, dtype=R.DT_BF16):
    ra, wc = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.ullsam_gemm_act_panels_query(dtype, M, N, K, act, out_f32, bias, res, aligned, ws, ctypes.addressof(ra), ctypes.addressof(wc)) == 0, lib.ullsam_last_error_string()
    return ra.value, wc.value


def test_query_follows_the_dispatch(lib):
    """The bench step's launches say yes; whatever leaves the ring kernels, or the layout, says no."""
    assert lib.ullsam_set_gemm_variant(0) == 0 and lib.ullsam_set_gemm_tuning(5, 1) == 0
    assert _query(lib, 4324, 28672, 4096, act=R.ACT_SWIGLU) == (1, 1)                       # llm.w13: reads xn, writes hmid
    assert _query(lib, 4324, 4096, 14336, out_f32=1, res=1) == (1, 0)                       # llm.w2: reads hmid; an fp32 residual stream is no panel output
    assert _query(lib, 4324, 6144, 4096, act=4) == (1, 0)                                   # llm.wqkv + RoPE
    assert _query(lib, 16384, 5120, 1280, act=R.ACT_GELU, bias=1) == (1, 1)                 # vit.lin1 on the 320-wide tile
    assert _query(lib, 16384, 3840, 1280, bias=1) == (1, 1)                                 # vit.qkv
    assert _query(lib, 16384, 1280, 5120, out_f32=1, bias=1, res=1) == (1, 0)               # vit.lin2
    assert _query(lib, 4324, 4096, 4096, aligned=0) == (0, 0)                               # a buffer off the 1 KiB boundary
    assert _query(lib, 4325, 4096, 4096) == (1, 0)                                          # odd M: the staged epilogue writes row-major only
    assert _query(lib, 1081, 4096, 4096) == (0, 0)                                          # 128x128 kernel
    assert _query(lib, 4, 4096, 4096) == (0, 0)                                             # decode step
    assert _query(lib, 4096, 4096, 4096, dtype=R.DT_F32) == (0, 0)
    assert _query(lib, 4324, 4096, 4096, act=R.ACT_GELU, out_f32=1) == (1, 0)
    try:
        assert lib.ullsam_set_gemm_tuning(5, 0) == 0
        assert _query(lib, 4324, 28672, 4096, act=R.ACT_SWIGLU) == (0, 0)                   # the switch: nothing takes panels
        assert lib.ullsam_set_gemm_tuning(5, 2) != 0 and b"bad value 2" in lib.ullsam_last_error_string()
    finally:
        assert lib.ullsam_set_gemm_tuning(5, 1) == 0
    try:
        assert lib.ullsam_set_gemm_variant(1) == 0
        assert _query(lib, 4324, 28672, 4096, act=R.ACT_SWIGLU) == (0, 0)                   # a forced 128x128 kernel
    finally:
        lib.ullsam_set_gemm_variant(R.VARIANT_DEFAULT)


def _refused(lib, rc, text):
    assert rc != 0
    msg = lib.ullsam_last_error_string().decode()
    assert text in msg, msg


def _gemm(lib, ap=1, cp=0, A=P, C=P, M=256, N=256, K=256, lda=None, ldc=None, act=0, out_f32=0, dtype=R.DT_BF16, res=None, ws=None):
    return lib.ullsam_gemm_act_panels(dtype, A, K if lda is None else lda, P, K, None, C, N if ldc is None else ldc, out_f32, None, res, N if res else 0, 0, act, M, N, K,
                                      ws, (128 << 20) if ws else 0, ap, cp, None)


def test_a_panel_flag_off_the_ring_kernels_is_refused_before_any_launch(lib):
    assert lib.ullsam_set_gemm_variant(0) == 0 and lib.ullsam_set_gemm_tuning(5, 1) == 0
    # the layout itself
    _refused(lib, _gemm(lib, dtype=R.DT_F32, K=256), "activation K-panels (A) are bf16")
    _refused(lib, _gemm(lib, lda=256 + 64), "contiguous (lda == K)")
    _refused(lib, _gemm(lib, A=P + 512), "1 KiB aligned")
    _refused(lib, _gemm(lib, ap=0, cp=1, out_f32=1), "activation K-panels (C) are bf16")
    _refused(lib, _gemm(lib, ap=0, cp=1, N=272), "activation K-panels (C) are bf16")         # N_out % 32
    _refused(lib, _gemm(lib, ap=0, cp=1, C=P + 16), "activation K-panels (C) are bf16")
    # routes that are not a ring kernel: 128x128 (few rows), the decode-step kernels, a forced variant, the ring split-K
    for kw in (dict(M=256), dict(M=1081, N=4096, K=4096), dict(M=4, N=4096, K=4096), dict(M=256, ap=0, cp=1)):
        _refused(lib, _gemm(lib, **kw), "does not reach a ring kernel")
    try:
        for v in (1, 3):
            assert lib.ullsam_set_gemm_variant(v) == 0
            _refused(lib, _gemm(lib, M=4324, N=4096, K=4096), "does not reach a ring kernel")
        lib.ullsam_set_gemm_variant(0)
        assert lib.ullsam_set_gemm_tuning(3, 2) == 0                                          # split-K wherever it fits
        _refused(lib, _gemm(lib, M=1081, N=4096, K=14336, out_f32=1, ws=P), "does not reach a ring kernel")
    finally:
        lib.ullsam_set_gemm_variant(R.VARIANT_DEFAULT)
        lib.ullsam_set_gemm_tuning(3, 1)
    # a ring launch that cannot WRITE panels (fp32 residual stream / odd M), and everything with the switch off
    _refused(lib, _gemm(lib, M=4325, N=4096, K=4096, ap=0, cp=1), "activation K-panels refused (A 0, C 1)")
    try:
        assert lib.ullsam_set_gemm_tuning(5, 0) == 0
        _refused(lib, _gemm(lib, M=4324, N=4096, K=4096), "activation K-panels refused (A 1, C 0)")
    finally:
        assert lib.ullsam_set_gemm_tuning(5, 1) == 0
    # the RoPE launch below the ring's 1024 rows, and the norm's own layout checks
    rope = lib.ullsam_gemm_qkv_rope_act_panels(R.DT_BF16, P, 256, P, 256, None, None, 1, 64, 256, 1, 2, P, P, P, 80, P, P, P, 64, 0, None, 0, 1, None)
    _refused(lib, rope, "does not reach a ring kernel")
    _refused(lib, lib.ullsam_norm_panels(P, 0, 48, P, None, None, 100, 48, 1e-6, 0, 0, None, None, 1, None), "panels need D % 32 == 0")
    _refused(lib, lib.ullsam_norm_panels(P, 0, 64, P + 64, None, None, 100, 64, 1e-6, 0, 0, None, None, 1, None), "1 KiB aligned output")
    _refused(lib, lib.ullsam_norm_panels(P, 0, 32, P, None, None, 8192, 32, 1e-6, 0, 0, None, None, 1, None), "narrow kernel")
