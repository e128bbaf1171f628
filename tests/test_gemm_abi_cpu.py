"""CPU half of the GEMM ABI tests: the helper (tests/gemm_ref.py) against itself, and the refusals that the GEMM entry points make before
any launch -- called with dummy addresses that are never dereferenced, because each of these checks precedes the first HIP call of its
entry point (csrc/gemm.hip gemm_impl, gemm_w8_impl)."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as R


@pytest.fixture(scope="module")
def lib():
    from ullsam_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("ld,off", [(7, 0), (9, 0), (8, 1), (15, 3)])
def test_padded_buffers_round_trip(dtype, ld, off):
    logical = torch.arange(5 * 7).reshape(5, 7).to(dtype)
    buf, ptr = R.padded(logical, ld, off)
    assert ptr == buf.data_ptr() + (R.HEAD + off) * buf.element_size()
    assert buf.numel() == R.HEAD + off + (5 + R.IN_GUARD_ROWS) * ld
    assert torch.equal(R.window(buf, 5, 7, ld, off), logical)
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    R.window(outside, 5, 7, ld, off).fill_(False)
    assert int(outside.sum()) == buf.numel() - 35
    pad = buf[outside]
    assert bool((pad == R.E4M3_NAN).all()) if dtype == torch.uint8 else bool(torch.isnan(pad.float()).all())
    b1, _ = R.padded(torch.arange(6).float(), off=1, guard_rows=1)       # a 1-D operand (bias, scales): one row and a guard row behind it
    assert b1.numel() == R.HEAD + 1 + 12 and torch.equal(b1[R.HEAD + 1:R.HEAD + 7], torch.arange(6).float()) and bool(torch.isnan(b1[R.HEAD + 7:]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_assert_untouched_fires_on_one_byte_at_each_side(dtype):
    M, n, ld, off = 5, 7, 9, 1
    buf, ptr = R.out_buffer(M, n, ld, off, dtype, "cpu")
    esz = buf.element_size()
    assert buf.numel() == R.HEAD + off + (M + R.GUARD_ROWS) * ld and bool((buf.view(torch.uint8) == R.SENTINEL).all())
    R.assert_untouched(buf, M, n, ld, off)
    R.window(buf, M, n, ld, off).fill_(1.0)                       # the window itself may change
    R.assert_untouched(buf, M, n, ld, off)
    first = R.HEAD + off
    sides = {"before the first element": first - 1, "right of row 0": first + n, "left of row 1 (the end of row 0's padding)": first + ld - 1,
             "right of the last row": first + (M - 1) * ld + n, "first guard row": first + M * ld, "last element of the guard": buf.numel() - 1,
             "first element of the buffer": 0}
    for name, e in sides.items():
        for byte in range(esz):
            b = buf.clone()
            b.view(torch.uint8)[e * esz + byte] ^= 1                 # one bit of one byte
            with pytest.raises(AssertionError, match="outside"):
                R.assert_untouched(b, M, n, ld, off)
    with pytest.raises(AssertionError, match="outside"):            # a refused call must leave the window alone too
        R.assert_untouched(buf, 0, 0, ld, off)
    # against a copy (the in-place residual, whose padding is NaN and not the sentinel)
    res, _ = R.padded(torch.ones(M, n), ld, off, guard_rows=R.GUARD_ROWS)
    before = res.clone()
    R.window(res, M, n, ld, off).add_(1.0)
    R.assert_untouched(res, M, n, ld, off, before)
    res[first + n] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        R.assert_untouched(res, M, n, ld, off, before)


def test_integer_operands_stay_exact_for_every_shape_of_the_gpu_file():
    from tests import test_gemm_abi_gpu as G
    shapes = G.all_exact_shapes()
    assert len(shapes) > 50
    for M, N, K in shapes:
        assert R.check_bound(K) < 1 << 24
    assert max(K for _, _, K in shapes) >= 5120
    with pytest.raises(AssertionError):
        R.check_bound((1 << 24) // 9)
    for K in G.W8_KS:                                               # e4m3 weights: |q| = |w| * 128 <= 384 under the power-of-two scale
        assert R.check_bound(K, w_max=384) < 1 << 24
    a = R.int_matrix(64, 48, 3)
    assert a.dtype == torch.float32 and float(a.abs().max()) == 3 and torch.equal(a, a.round()) and torch.equal(a, R.int_matrix(64, 48, 3))
    assert not torch.equal(a, R.int_matrix(64, 48, 4)) and torch.equal(a.bfloat16().float(), a)
    b = R.int_bias(600)
    assert float(b.abs().max()) <= 125 and len(set(b[:251].tolist())) == 251 and len(set(b[300:551].tolist())) == 251
    r = R.int_residual(300, 270)
    assert float(r.abs().max()) <= 125 and bool((r[:, 1:] != r[:, :-1]).all()) and bool((r[1:] != r[:-1]).all())
    assert len({tuple(row) for row in r[:251, :4].tolist()}) == 251   # rows m and m + r differ for r < 251 (res_row_mod picks the right one)
    q = R.e4m3_of_small_int(torch.tensor([-3, -2, -1, 0, 1, 2, 3]))
    assert q.tolist() == [0xC4, 0xC0, 0xB8, 0x00, 0x38, 0x40, 0x44]
    if hasattr(torch, "float8_e4m3fn"):
        assert q.view(torch.float8_e4m3fn).float().tolist() == [-3, -2, -1, 0, 1, 2, 3]


def test_float64_definition_equals_a_plain_loop():
    M, N, K = 5, 7, 64
    A, W = R.int_matrix(M, K, 1).numpy(), R.int_matrix(N, K, 2).numpy()
    bias, res = R.int_bias(N).numpy(), R.int_residual(M, N).numpy()
    for use_bias in (False, True):
        for res_rows, mod in ((0, 0), (M, 0), (2, 2)):
            for act in (R.ACT_NONE, R.ACT_RELU):
                want = np.zeros((M, N), np.float64)
                for m in range(M):
                    for n in range(N):
                        s = 0.0
                        for k in range(K):
                            s += float(A[m, k]) * float(W[n, k])
                        if use_bias:
                            s += float(bias[n])
                        if act == R.ACT_RELU:
                            s = max(s, 0.0)
                        if res_rows:
                            s += float(res[m % mod if mod else m, n])
                        want[m, n] = s
                got = R.gemm_ref64(torch.from_numpy(A), torch.from_numpy(W), torch.from_numpy(bias) if use_bias else None,
                                   torch.from_numpy(res[:res_rows]) if res_rows else None, mod, act)
                assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want), (use_bias, res_rows, mod, act)
                assert (want < 0).any() or act == R.ACT_RELU
    # the bits of an output: fp32, then bf16 by round-to-nearest-even (bf16 steps by 2 above 256: the ties 257, 259, 261 go to 256, 260, 260)
    y = torch.tensor([257.0, 259.0, 261.0, -257.0, 3.0], dtype=torch.float64)
    assert R.expected_bits(y, torch.bfloat16).float().tolist() == [256.0, 260.0, 260.0, -256.0, 3.0]
    assert R.expected_bits(y, torch.float32).tolist() == y.tolist()


# ---------------------------------------------------------------------------------------------------------------- refusals before any launch
P = 1 << 20     # a 16-byte aligned dummy address: never dereferenced, every check below comes before the first HIP call


def _refused(lib, rc, text):
    assert rc != 0
    msg = lib.ullsam_last_error_string().decode()
    assert text in msg, msg


def _gemm(lib, dtype=R.DT_BF16, A=P, lda=None, W=P, ldw=None, C=P, ldc=None, out_f32=0, bias=None, res=None, ldr=0, rrm=0, act=0, M=256, N=256, K=256):
    return lib.ullsam_gemm(dtype, A, K if lda is None else lda, W, K if ldw is None else ldw, C, N if ldc is None else ldc, out_f32, bias, res, ldr, rrm, act,
                           M, N, K, None, 0, None)


def test_gemm_refusals_before_any_launch(lib):
    _refused(lib, _gemm(lib, K=96), "K=96 must be a multiple of 64")                       # bf16: 128 bytes per k tile
    _refused(lib, _gemm(lib, dtype=R.DT_F32, K=48), "K=48 must be a multiple of 32")
    _refused(lib, _gemm(lib, A=P + 8), "A/W must be 16-byte aligned")
    _refused(lib, _gemm(lib, W=P + 2), "A/W must be 16-byte aligned")
    _refused(lib, _gemm(lib, lda=256 + 4), "lda/ldw rows must be 16-byte multiples")        # 520 bytes per row
    _refused(lib, _gemm(lib, ldw=256 + 1), "lda/ldw rows must be 16-byte multiples")
    _refused(lib, _gemm(lib, dtype=R.DT_F32, lda=256 + 2), "lda/ldw rows must be 16-byte multiples")
    for empty in (dict(M=0), dict(N=0), dict(K=0)):
        _refused(lib, _gemm(lib, **empty), "empty problem")
    _refused(lib, _gemm(lib, dtype=2), "bad dtype 2")
    _refused(lib, _gemm(lib, act=R.ACT_SWIGLU, bias=P), "swiglu needs")
    _refused(lib, _gemm(lib, act=R.ACT_SWIGLU, res=P, ldr=128), "swiglu needs")
    _refused(lib, _gemm(lib, act=R.ACT_SWIGLU, N=192), "swiglu needs")
    _refused(lib, _gemm(lib, act=4), "act 4 is ullsam_gemm_qkv_rope")
    _refused(lib, _gemm(lib, act=5), "bad act 5")
    try:
        for v in (6, 8, 9):
            assert lib.ullsam_set_gemm_variant(v) == 0
            _refused(lib, _gemm(lib, dtype=R.DT_F32), "the ring kernels need bf16")         # a forced ring variant on fp32 ...
            _refused(lib, _gemm(lib, K=64), "the ring kernels need bf16")                   # ... and below the ring's four stages
            _refused(lib, _gemm(lib, bias=P, N=250), "the ring kernels need bf16")          # a bias of partial float4 groups
            _refused(lib, _gemm(lib, bias=P + 4), "the ring kernels need bf16")             # a misaligned bias
            _refused(lib, _gemm(lib, act=R.ACT_SWIGLU, N=384), "the ring kernels need bf16")
        assert lib.ullsam_set_gemm_variant(8) == 0
        _refused(lib, _gemm(lib, act=R.ACT_SWIGLU, N=512), "256x320: no SwiGLU")
        assert lib.ullsam_set_gemm_variant(3) == 0
        _refused(lib, _gemm(lib, act=R.ACT_SWIGLU, N=384), "SwiGLU epilogue needs N % 256 == 0")
    finally:
        lib.ullsam_set_gemm_variant(R.VARIANT_DEFAULT)


def test_sibling_refusals_before_any_launch(lib):
    w8 = lambda **k: lib.ullsam_gemm_w8(k.get("A", P), None, 0, None, 0.0, k.get("W8", P), k.get("ldw", k.get("K", 512)), k.get("ws", P), k.get("C", P), 128, 0, None, None, 0,
                                        k.get("act", 0), k.get("M", 4), 128, k.get("K", 512), None)
    _refused(lib, w8(ldw=504), "weight rows must be 8-byte aligned (ldw=504)")              # ldw < K
    _refused(lib, w8(ldw=516), "weight rows must be 8-byte aligned (ldw=516)")
    _refused(lib, w8(M=9), "decode-step shapes only")
    _refused(lib, w8(K=256), "decode-step shapes only")
    _refused(lib, w8(ws=None), "null weights, scales or output")
    _refused(lib, w8(act=4), "act 4 is ullsam_decode_qkv_rope_w8")
    _refused(lib, w8(A=P + 2), "bf16 activations must be 16-byte aligned")
    rms = lambda ldx: lib.ullsam_gemm_rmsnorm(P, ldx, P, 1e-5, P, 2048, P, 128, 0, None, None, 0, 0, 2, 128, 2048, None)
    _refused(lib, rms(2050), "the RMSNorm prologue needs 16-byte aligned fp32 rows")         # ldx % 4 != 0
    _refused(lib, rms(2049), "the RMSNorm prologue needs 16-byte aligned fp32 rows")
    _refused(lib, lib.ullsam_gemm_rmsnorm(P, 2048, P, 1e-5, P, 2048, P, 128, 0, None, None, 0, 4, 2, 128, 2048, None), "act 4 is ullsam_decode_qkv_rope")
    fp8 = lambda **k: lib.ullsam_gemm_fp8(k.get("A", P), k.get("lda", 256), P, P, k.get("ldw", 256), k.get("ws", P), P, 256, 0, None, None, 0, k.get("act", 0), 256, 256, k.get("K", 256), None)
    _refused(lib, fp8(K=192), "K=192 must be a positive multiple of 128")
    _refused(lib, fp8(lda=264), "16-byte aligned rows needed")
    _refused(lib, fp8(A=P + 8), "16-byte aligned rows needed")
    _refused(lib, fp8(ws=None), "scales are required")
    _refused(lib, fp8(act=3), "bad act 3")
    rope = lambda **k: lib.ullsam_gemm_qkv_rope(R.DT_BF16, P, 256, P, 256, None, 1, k.get("S", 8), 256, 1, 2, P, P, P, 16, k.get("q", P), P, P, k.get("cap", 8), k.get("pos0", 0), None, 0, None)
    _refused(lib, rope(pos0=1), "cache overflow (1 + 8 > 8)")
    _refused(lib, rope(q=P + 8), "16-byte aligned outputs needed")
    _refused(lib, rope(S=0), "bad dims")
