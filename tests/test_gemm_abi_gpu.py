"""The GEMM entry points of include/ullsam_hip.h at the leading dimensions, alignments and ragged edges that ops.gemm never passes.

Two oracles, no tolerance (tests/gemm_ref.py):
  exact      integer operands, act in {none, ReLU}: the result equals the float64 definition in bits, whatever kernel and summation order;
  invariance with the kernel held fixed, a padded / offset call equals the dense call on the same operands in bits (GELU, SwiGLU, RoPE,
             fp8 scales, the RMSNorm prologue: the stride moves addresses, not arithmetic).
Every call runs with NaN in all input padding and a sentinel guard (>= 272 rows of ldc) around the output, checked after the call."""
import pytest
import torch

from tests import gemm_ref as R
from tests.gemm_ref import Layout

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NONE, GELU, RELU, SWIGLU = R.ACT_NONE, R.ACT_GELU, R.ACT_RELU, R.ACT_SWIGLU
RING = (6, 8, 9)
RING_REFUSAL = "the ring kernels need bf16"

# name, forced variant (0 = auto), operand type
KERNELS = [("v1-f32", 1, F32), ("v1-bf16", 1, BF16), ("v3-f32", 3, F32), ("v3-bf16", 3, BF16), ("v6", 6, BF16), ("v8", 8, BF16), ("v9", 9, BF16),
           ("auto-f32", 0, F32), ("auto-bf16", 0, BF16)]
KERNEL_IDS = [k[0] for k in KERNELS]

# epilogues with one right answer: (bias, residual, res_row_mod = M // 3, act, fp32 output)
MODES = {"plain": (0, 0, 0, NONE, 0), "bias": (1, 0, 0, NONE, 0), "bias_relu": (1, 0, 0, RELU, 0), "res": (0, 1, 0, NONE, 0), "bias_res": (1, 1, 0, NONE, 0),
         "f32": (0, 0, 0, NONE, 1), "bias_relu_f32": (1, 0, 0, RELU, 1), "bias_res_f32": (1, 1, 0, NONE, 1), "rowmod_f32": (1, 1, 1, NONE, 1)}
F32_MODES = ("plain", "bias_relu", "bias_res", "rowmod_f32")          # fp32 operands: the output is fp32 either way
IN_LAYOUTS = [Layout(lda=8), Layout(ldw=16)]
OUT_LAYOUTS = [Layout(ldc=8), Layout(ldc=1), Layout(c_off=1)]          # keeps vec_ok, breaks it by the row pitch, breaks it by the base
RES_LAYOUTS = [Layout(ldr=4), Layout(ldr=1), Layout(r_off=1)]          # the same for the residual
INPLACE = Layout(ldc=4, ldr=4, inplace=True)                           # C == residual, ldc == ldr == N + 4, fp32
W8_KS = (512, 2048)


def tile_shapes(variant, dtype):
    """The smallest shapes at which the tile kernels' paths divide: M one row / one row pair around a tile (odd: the ring's staged epilogue, even: its direct
    one), N whole / ragged / not a multiple of 8 / of 4, K at the ring's minimum, % 64 only, and below it where the kernel takes it.  Every N meets an odd and an even M."""
    Ms = [1, 254, 255, 257, 258] + ([271, 273, 274] if variant == 9 else []) + ([127, 129] if variant == 1 else [])   # (around the 272-row and the 128-row tile too)
    Ns = [256, 264, 252, 250] + ([320, 328] if variant == 8 else [])
    Ks = [32, 96, 128] if dtype == F32 else [128, 192, 320] + ([64] if variant == 1 else [])
    per = len(Ns) // 2
    return [(M, Ns[(per * i + j) % len(Ns)], Ks[(i + j) % len(Ks)]) for i, M in enumerate(Ms) for j in range(per)]


MULTI_ROUND = [(6, 4098, 4352, 128), (6, 4098, 4352, 384), (9, 4352, 4352, 384), (8, 4864, 4480, 384)]   # > 256 tiles; K >= 384: the persistent form
SPLITK_RING = (1081, 4096, 5120)
SPLITK_TAIL = (4324, 4096, 4096)
AUTO_EDGE = [(M, N, 256) for M in (1023, 1024) for N in (255, 256)] + [(1023, 12288, 512), (1024, 12288, 512)]   # the last two: 192 tiles, enough for auto to pick the ring at M >= 1024
FAR_LDA = (2, 65792, 384)                                               # 257 tiles of 256 x 256 in one tile row
SKINNY = [(M, N, K) for M in (1, 4, 5, 8) for K in W8_KS for N in (128, 136, 130)]
FP8 = [(M, N, K) for M in (255, 257, 258) for N in (256, 264, 252) for K in (128, 384)]


def all_exact_shapes():
    """Every (M, N, K) this file hands the exact oracle (tests/test_gemm_abi_cpu.py checks the 2^24 bound for each)."""
    s = set()
    for _, v, dt in KERNELS:
        s.update(tile_shapes(v, dt))
    s.update((M, N, K) for _, M, N, K in MULTI_ROUND)
    s.update([SPLITK_RING, SPLITK_TAIL, FAR_LDA])
    s.update(AUTO_EDGE + SKINNY + FP8)
    return sorted(s)


def _diff(got, want):
    """None when got == want in bits (values; NaN never equals), else a description of the difference."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return None
    bad = got != want
    i = tuple(torch.nonzero(bad)[0].tolist())
    return (f"{int(bad.sum())} of {got.numel()} elements differ, {int(torch.isnan(got.float()).sum())} NaN; first at {i}: "
            f"{float(got[i])} against {float(want[i])}")


def _operands(M, N, K, dtype, seed):
    R.check_bound(K)
    return (R.int_matrix(M, K, seed, dtype, DEV), R.int_matrix(N, K, seed + 1, dtype, DEV), R.int_bias(N, DEV), R.int_residual(M, N, DEV))


def _mode_args(mode, M, bias, res):
    b, r, rowmod, act, f32 = MODES[mode]
    mod = max(1, M // 3) if rowmod else 0
    return dict(bias=bias if b else None, residual=(res[:mod] if mod else res) if r else None, res_row_mod=mod, act=act, out_f32=bool(f32))


def _extra(mode, f32_out=False):
    """The layouts that only an epilogue with a residual / a bias has."""
    b, r, _, _, f32 = MODES[mode]
    return (RES_LAYOUTS if r else []) + ([Layout(bias_off=1)] if b else []) + ([INPLACE] if r and (f32 or f32_out) else [])   # bias_off: a bias that is not 16-byte aligned


def _layouts(mode, f32_out=False):
    b, r, rowmod, _, f32 = MODES[mode]
    if rowmod:                                   # the row-broadcast residual always sits at a padded ldr
        return [Layout(ldr=4), Layout(ldr=4, ldc=8), Layout(ldr=1, ldc=1)]
    lays = [R.DENSE] + OUT_LAYOUTS
    if mode in ("plain", "bias_res_f32", "bias_res"):
        lays += IN_LAYOUTS
    return lays + _extra(mode, f32_out)


def _exact_case(fails, tag, A, W, bias, res, mode, lays, variant, f32_out=False, **kw):
    """One epilogue of one problem at every layout of `lays` against the float64 definition; a forced ring variant must refuse what ring_ok excludes."""
    M = A.shape[0]
    N, K = W.shape
    args = _mode_args(mode, M, bias, res)
    if f32_out:
        args["out_f32"] = True
    want = R.expected_bits(R.gemm_ref64(A, W, args["bias"], args["residual"], args["res_row_mod"], args["act"]), F32 if args["out_f32"] else A.dtype)
    for lay in lays:
        if lay.inplace and not args["out_f32"]:
            continue
        where = f"{tag} {M}x{N}x{K} {mode} {lay}"
        if variant in RING:
            bias_ptr = None if args["bias"] is None else 4 * lay.bias_off       # (allocations are 16-byte aligned: only the offset counts)
            if not R.ring_ok(A.dtype, args["act"], N, K, bias_ptr):
                R.run_gemm(A, W, lay=lay, refuse=RING_REFUSAL, **args, **kw)
                continue
        try:
            d = _diff(R.run_gemm(A, W, lay=lay, **args, **kw), want)
        except AssertionError as e:                # a guard band that was written
            d = str(e)
        if d:
            fails.append(f"{where}: {d}")


@pytest.mark.parametrize("name,variant,dtype", KERNELS, ids=KERNEL_IDS)
def test_gemm_is_exact_on_integer_operands_at_every_layout(name, variant, dtype):
    """Each tile kernel (forced), and the auto dispatch, on the integer problems: every linear epilogue, both output types, vec_ok on and off through the
    row pitch, the base address, the residual's pitch and base and a ragged N, padded lda / ldw, the in-place residual -- equal to float64 in bits, guards intact."""
    fails = []
    with R.forced_variant(variant):
        for s, (M, N, K) in enumerate(tile_shapes(variant, dtype)):
            A, W, bias, res = _operands(M, N, K, dtype, 100 * variant + s)
            for mode in (F32_MODES if dtype == F32 else MODES):
                _exact_case(fails, name, A, W, bias, res, mode, _layouts(mode, dtype == F32), variant, f32_out=dtype == F32)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


def _random_operands(M, N, K, dtype, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    a = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
    return a, w, torch.randn(N, device=DEV, generator=g), torch.randn(M, N, device=DEV, generator=g)


def _invariance_case(fails, tag, run, lays):
    """run(lay) at the dense layout and at every layout of `lays`: equal in bits, no NaN."""
    dense = run(R.DENSE)
    if bool(torch.isnan(dense.float()).any()):
        fails.append(f"{tag} dense: NaN in the result")
    for lay in lays:
        try:
            d = _diff(run(lay), dense)
        except AssertionError as e:
            d = str(e)
        if d:
            fails.append(f"{tag} {lay}: {d}")


@pytest.mark.parametrize("name,variant,dtype", KERNELS[:7], ids=KERNEL_IDS[:7])
def test_gemm_inexact_epilogues_do_not_depend_on_the_layout(name, variant, dtype):
    """GELU and SwiGLU on random operands with the kernel held fixed: the padded / offset / vec_ok-breaking calls equal the dense call in bits.  SwiGLU at
    the legal widths; a forced kernel refuses the others (256x320: every SwiGLU; the 256-row kernels: N % 256 != 0) and leaves the output alone."""
    fails = []
    K = 96 if dtype == F32 else 192
    lays = [Layout(lda=8, ldw=16)] + OUT_LAYOUTS
    with R.forced_variant(variant):
        for M in (254, 257):
            for N in (256, 264, 252):
                a, w, bias, res = _random_operands(M, N, K, dtype, M + N)
                _invariance_case(fails, f"{name} {M}x{N}x{K} bias_gelu", lambda lay: R.run_gemm(a, w, bias, act=GELU, lay=lay), lays)
                if dtype == BF16:
                    _invariance_case(fails, f"{name} {M}x{N}x{K} bias_gelu_f32", lambda lay: R.run_gemm(a, w, bias, act=GELU, out_f32=True, lay=lay), lays)
                _invariance_case(fails, f"{name} {M}x{N}x{K} bias_gelu_res_f32", lambda lay: R.run_gemm(a, w, bias, res, act=GELU, out_f32=True, lay=lay), lays + RES_LAYOUTS)
            for N in (256, 384, 512):
                a, w, _, _ = _random_operands(M, N, K, dtype, M + N + 1)
                if variant == 8:
                    R.run_gemm(a, w, act=SWIGLU, refuse="256x320: no SwiGLU")
                elif N % 256 != 0 and variant in RING:
                    R.run_gemm(a, w, act=SWIGLU, refuse=RING_REFUSAL)
                elif N % 256 != 0 and variant == 3:
                    R.run_gemm(a, w, act=SWIGLU, refuse="SwiGLU epilogue needs N % 256 == 0")
                else:
                    _invariance_case(fails, f"{name} {M}x{N}x{K} swiglu", lambda lay: R.run_gemm(a, w, act=SWIGLU, lay=lay), lays)
                    if dtype == BF16:
                        _invariance_case(fails, f"{name} {M}x{N}x{K} swiglu_f32", lambda lay: R.run_gemm(a, w, act=SWIGLU, out_f32=True, lay=lay), lays)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


@pytest.mark.parametrize("variant,M,N,K", MULTI_ROUND)
def test_ring_launches_of_more_than_one_round_with_strides(variant, M, N, K):
    """More than 256 ring tiles with padded lda / ldc (/ ldr): one tile per workgroup (tuning key 2 = 0) and the default (2: the persistent form, which takes
    K >= 384) give the same bits, and those are the float64 definition's."""
    fails = []
    A, W, bias, res = _operands(M, N, K, BF16, M + K)
    for mode, lay in (("plain", Layout(lda=8, ldc=8)), ("bias_relu", Layout(lda=8, ldw=16, ldc=8)), ("bias_res_f32", Layout(lda=8, ldc=8, ldr=4)),
                      ("bias_res", Layout(lda=8, ldc=8, ldr=4))):          # (a residual on a bf16 output: no direct epilogue adds one, so never the persistent form)
        args = _mode_args(mode, M, bias, res)
        want = R.expected_bits(R.gemm_ref64(A, W, args["bias"], args["residual"], 0, args["act"]), F32 if args["out_f32"] else BF16)
        got = {}
        for persist in (0, 2):
            with R.tuning(2, persist), R.forced_variant(variant):
                got[persist] = R.run_gemm(A, W, lay=lay, **args)
            d = _diff(got[persist], want)
            if d:
                fails.append(f"v{variant} {mode} key 2 = {persist} {lay}: {d}")
        if not torch.equal(got[0], got[2]):
            fails.append(f"v{variant} {mode}: key 2 = 0 and key 2 = 2 differ")
    assert not fails, "\n".join(fails)


def _ws_probe():
    ws = R.workspace(DEV)
    ws[:4096].fill_(R.SENTINEL)          # (an integer partial sum never has the sentinel's bytes)
    return lambda: bool((ws[:4096] != R.SENTINEL).any())


def test_ring_split_k_with_strides_and_where_its_plan_declines():
    """The smallest shape that plans a split (tuning key 3 = 2) with padded lda / ldw: equal to float64 -- integers make the K ranges' order irrelevant -- and
    so are the calls the plan must decline (ldc = N + 1: no vec_ok; no workspace; key 3 = 0).  The caller's workspace is written exactly when a split ran."""
    M, N, K = SPLITK_RING
    A, W, bias, res = _operands(M, N, K, BF16, 7)
    want = R.expected_bits(R.gemm_ref64(A, W), BF16)
    want_res = R.expected_bits(R.gemm_ref64(A, W, bias, res), F32)
    pad = dict(lda=8, ldw=16)
    fails = []
    for tag, key3, kw, lay, split in (("split", 2, {}, Layout(**pad), True), ("split ldc + 8", 2, {}, Layout(ldc=8, **pad), True),
                                      ("ldc + 1", 2, {}, Layout(ldc=1, **pad), False), ("no workspace", 2, dict(ws=False), Layout(**pad), False),
                                      ("key 3 = 0", 0, {}, Layout(**pad), False), ("default", 1, {}, Layout(**pad), False)):
        touched = _ws_probe()
        with R.tuning(3, key3):
            got = R.run_gemm(A, W, lay=lay, **kw)
        d = _diff(got, want)
        if d:
            fails.append(f"{tag}: {d}")
        if touched() != split:
            fails.append(f"{tag}: the workspace was {'written' if touched() else 'not written'}")
    for tag, lay, split in (("split + bias + residual", Layout(ldc=8, ldr=4, **pad), True), ("bias + residual, ldr + 1", Layout(ldr=1, **pad), False)):
        touched = _ws_probe()
        with R.tuning(3, 2):
            got = R.run_gemm(A, W, bias, res, out_f32=True, lay=lay)
        d = _diff(got, want_res)
        if d:
            fails.append(f"{tag}: {d}")
        if touched() != split:
            fails.append(f"{tag}: the workspace was {'written' if touched() else 'not written'}")
    assert not fails, "\n".join(fails)


def test_two_buffer_kernel_split_k_tail_with_a_padded_ldc():
    """272 tiles of 256 x 256 = one round and a tail of 16 that the two-buffer kernel cuts along K when it has a workspace: with and without one, at a padded
    ldc (and ldr), equal to float64."""
    M, N, K = SPLITK_TAIL
    A, W, bias, res = _operands(M, N, K, BF16, 11)
    fails = []
    with R.forced_variant(3):
        for mode, lay in (("plain", Layout(ldc=8)), ("bias_res_f32", Layout(ldc=8, ldr=4)), ("bias_relu", Layout(ldc=1))):
            args = _mode_args(mode, M, bias, res)
            want = R.expected_bits(R.gemm_ref64(A, W, args["bias"], args["residual"], 0, args["act"]), F32 if args["out_f32"] else BF16)
            for ws, split in ((True, True), (False, False)):
                touched = _ws_probe()
                d = _diff(R.run_gemm(A, W, lay=lay, ws=ws, **args), want)
                if d:
                    fails.append(f"{mode} {lay} workspace {ws}: {d}")
                if touched() != split:
                    fails.append(f"{mode} workspace {ws}: the workspace was {'written' if touched() else 'not written'}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("M,N,K", AUTO_EDGE)
def test_auto_dispatch_across_its_thresholds(M, N, K):
    """Both sides of the auto dispatch's M >= 1024 and N >= 256 conditions (csrc/gemm.hip gemm_impl), dense and padded; the kernel chosen may change with
    the layout, the integer answer may not."""
    fails = []
    A, W, bias, res = _operands(M, N, K, BF16, M + N)
    lays = [R.DENSE, Layout(lda=8, ldw=16, ldc=8, ldr=4), Layout(ldc=1, ldr=1), Layout(c_off=1, r_off=1)]
    for mode in ("plain", "bias_relu", "bias_res", "bias_res_f32", "rowmod_f32"):
        _exact_case(fails, "auto", A, W, bias, res, mode, lays[:3] if N > 256 else lays, 0)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


def test_ring_with_rows_too_far_apart_for_32_bit_offsets():
    """csrc/gemm.hip ring_persist_ok sends a launch whose A rows span 4 GiB or more away from the persistent form (32-bit descriptor offsets).  Two rows at an lda
    just below and just above that limit (a 67 MB backing buffer each), 257 tiles, forced 256 x 256 ring: both equal float64."""
    M, N, K = FAR_LDA
    A, W, bias, _ = _operands(M, N, K, BF16, 3)
    want = R.expected_bits(R.gemm_ref64(A, W, bias, act=RELU), BF16)
    limit = -(-((1 << 31) - K) // (M + 256))                  # the smallest lda with ((M + 256) lda + K) * 2 >= 2^32
    fails = []
    with R.forced_variant(6):
        for lda in ((limit + 7) // 8 * 8, (limit - 8) // 8 * 8):
            assert (((M + 256) * lda + K) * 2 >= 1 << 32) == (lda >= limit)
            d = _diff(R.run_gemm(A, W, bias, act=RELU, lay=Layout(lda=lda - K, ldc=8)), want)
            if d:
                fails.append(f"lda {lda}: {d}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------- the decode-step kernels
SKINNY_LAYOUTS = [Layout(lda=8, ldw=8), Layout(ldc=8), Layout(ldc=1), Layout(c_off=1)]


@pytest.mark.parametrize("K", W8_KS)
@pytest.mark.parametrize("M", [1, 4, 5, 8])
def test_decode_step_kernels_through_ullsam_gemm(M, K):
    """M <= 8 bf16 rows take the weight-streaming kernels (K % 2048 == 0 and N <= 8192: K split over a workgroup's waves; otherwise a wave per four rows of W):
    exact on the integer problems and layout-invariant for GELU and SwiGLU, at N whole, % 8 and % 2 only."""
    fails = []
    for N in (128, 136, 130):
        A, W, bias, res = _operands(M, N, K, BF16, M + N + K)
        for mode in ("plain", "bias_relu", "res", "bias_res_f32"):
            lays = [R.DENSE] + SKINNY_LAYOUTS + _extra(mode)
            _exact_case(fails, "decode", A, W, bias, res, mode, lays, 0)
        a, w, rb, rr = _random_operands(M, N, K, BF16, M + N + K)
        _invariance_case(fails, f"decode {M}x{N}x{K} bias_gelu", lambda lay: R.run_gemm(a, w, rb, act=GELU, lay=lay), SKINNY_LAYOUTS)
        _invariance_case(fails, f"decode {M}x{N}x{K} bias_gelu_res_f32", lambda lay: R.run_gemm(a, w, rb, rr, act=GELU, out_f32=True, lay=lay), SKINNY_LAYOUTS + RES_LAYOUTS)
        if N % 128 == 0:
            _invariance_case(fails, f"decode {M}x{N}x{K} swiglu", lambda lay: R.run_gemm(a, w, act=SWIGLU, lay=lay), SKINNY_LAYOUTS)
            _invariance_case(fails, f"decode {M}x{N}x{K} swiglu_f32", lambda lay: R.run_gemm(a, w, act=SWIGLU, out_f32=True, lay=lay), SKINNY_LAYOUTS)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


@pytest.mark.parametrize("K", [2048, 4096])
@pytest.mark.parametrize("M", [1, 3, 4])
def test_gemm_rmsnorm_does_not_depend_on_the_layout(M, K):
    """ullsam_gemm_rmsnorm with x at ldx = K + 4 (NaN in the padding), W at ldw = K + 8 and the output / residual variations against the dense call."""
    fails = []
    g = torch.Generator(device=DEV)
    g.manual_seed(M + K)
    x = torch.randn(M, K, device=DEV, generator=g) * 3
    nw = 1 + 0.1 * torch.randn(K, device=DEV, generator=g)
    lays = [Layout(ldw=8), Layout(ldc=8), Layout(ldc=1), Layout(c_off=1)]
    for N in (128, 136, 130):
        _, w, bias, res = _random_operands(M, N, K, BF16, N + K)
        for tag, kw, more in (("plain", {}, []), ("bias_gelu", dict(bias=bias, act=GELU), []), ("bias_res_f32", dict(bias=bias, residual=res, out_f32=True), RES_LAYOUTS),
                              ("swiglu", dict(act=SWIGLU), [])):
            if tag == "swiglu" and N % 128 != 0:
                continue
            dense = R.run_gemm_rmsnorm(x, nw, 1e-5, w, **kw)
            if bool(torch.isnan(dense.float()).any()):
                fails.append(f"{M}x{N}x{K} {tag}: NaN in the dense result")
            for ldx in (4, 0):
                for lay in lays + more:
                    try:
                        d = _diff(R.run_gemm_rmsnorm(x, nw, 1e-5, w, lay=lay, ldx=ldx, **kw), dense)
                    except AssertionError as e:
                        d = str(e)
                    if d:
                        fails.append(f"{M}x{N}x{K} {tag} ldx + {ldx} {lay}: {d}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


@pytest.mark.parametrize("K", W8_KS)
@pytest.mark.parametrize("M", [1, 4, 5, 8])
def test_gemm_w8_exact_and_layout_invariant(M, K):
    """ullsam_gemm_w8 with the e4m3 rows at ldw = K + 8 bytes (padding = the e4m3 NaN byte): exact on integer weights, whose power-of-two row scales
    (ops.rows_fp8_pow2) dequantise exactly, and layout-invariant for GELU, SwiGLU and the RMSNorm prologue (M <= 4, K = 2048)."""
    from ullsam_amd import ops
    fails = []
    R.check_bound(K, w_max=384)
    lays = [Layout(ldw=8), Layout(ldc=8), Layout(ldc=1), Layout(c_off=1)]
    for N in (128, 136, 130):
        A, W, bias, res = _operands(M, N, K, BF16, M + N + K + 5)
        q, sc = ops.rows_fp8_pow2(W.contiguous())
        assert float(sc.max()) <= 2.0 ** -7                     # amax 3 -> the smallest power of two with 3 / scale <= 448: q = 128 w <= 384 is exact in e4m3
        for mode in ("plain", "bias_relu", "res", "bias_res_f32"):
            args = _mode_args(mode, M, bias, res)
            want = R.expected_bits(R.gemm_ref64(A, W, args["bias"], args["residual"], 0, args["act"]), F32 if args["out_f32"] else BF16)
            for lay in [R.DENSE] + lays + _extra(mode):
                try:
                    d = _diff(R.run_gemm_w8(A, q, sc, args["bias"], args["residual"], args["act"], args["out_f32"], lay), want)
                except AssertionError as e:
                    d = str(e)
                if d:
                    fails.append(f"w8 {M}x{N}x{K} {mode} {lay}: {d}")
        a, w, rb, rr = _random_operands(M, N, K, BF16, M + N + K + 6)
        q, sc = ops.rows_fp8_pow2(w.contiguous())
        _invariance_case(fails, f"w8 {M}x{N}x{K} bias_gelu_res_f32", lambda lay: R.run_gemm_w8(a, q, sc, rb, rr, GELU, True, lay), lays + RES_LAYOUTS)
        if N % 128 == 0:
            _invariance_case(fails, f"w8 {M}x{N}x{K} swiglu", lambda lay: R.run_gemm_w8(a, q, sc, act=SWIGLU, lay=lay), lays)
        if M <= 4 and K == 2048:
            x = a.float() * 3
            nw = torch.linspace(0.9, 1.1, K, device=DEV)
            _invariance_case(fails, f"w8 {M}x{N}x{K} rmsnorm bias_gelu", lambda lay: R.run_gemm_w8(x, q, sc, rb, None, GELU, False, lay, norm_w=nw, eps=1e-5, ldx=4 if lay.ldw else 0),
                             lays)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


# ---------------------------------------------------------------------------------------------------------------- fp8 operands
FP8_IN = Layout(lda=16, ldw=32)


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [255, 257, 258])
def test_gemm_fp8_exact_and_layout_invariant(M, K):
    """ullsam_gemm_fp8 around its 256 x 256 tile: integers (exact in e4m3) with unit scales, and with power-of-two scales per row and column, equal float64 at
    padded lda / ldw / ldc / ldr and with its vec condition on and off; GELU on quantised random operands is layout-invariant."""
    from ullsam_amd import ops
    fails = []
    for N in (256, 264, 252):
        A, W, bias, res = _operands(M, N, K, F32, M + N + K + 9)
        A8, W8 = R.e4m3_of_small_int(A), R.e4m3_of_small_int(W)
        for sa, sw in ((torch.ones(M, device=DEV), torch.ones(N, device=DEV)),
                       (2.0 ** (torch.arange(M, device=DEV) % 3).float(), 2.0 ** (torch.arange(N, device=DEV) % 2).float())):
            As, Ws = A * sa[:, None], W * sw[:, None]
            assert float(As.abs().max()) * float(Ws.abs().max()) * K + 250 < 1 << 24
            for mode in ("plain", "bias_relu", "res", "f32", "bias_res_f32"):
                args = _mode_args(mode, M, bias, res)
                want = R.expected_bits(R.gemm_ref64(As, Ws, args["bias"], args["residual"], 0, args["act"]), F32 if args["out_f32"] else BF16)
                for lay in [R.DENSE, FP8_IN] + OUT_LAYOUTS + _extra(mode):
                    try:
                        d = _diff(R.run_gemm_fp8(A8, sa, W8, sw, args["bias"], args["residual"], args["act"], args["out_f32"], lay), want)
                    except AssertionError as e:
                        d = str(e)
                    if d:
                        fails.append(f"fp8 {M}x{N}x{K} {mode} {lay}: {d}")
        a, w, rb, rr = _random_operands(M, N, K, F32, M + N + K + 10)
        a8, sa = ops.rows_fp8(a.contiguous())
        w8, sw = ops.rows_fp8(w.contiguous())
        _invariance_case(fails, f"fp8 {M}x{N}x{K} bias_gelu", lambda lay: R.run_gemm_fp8(a8, sa, w8, sw, rb, None, GELU, False, lay), [FP8_IN] + OUT_LAYOUTS)
        _invariance_case(fails, f"fp8 {M}x{N}x{K} bias_gelu_res_f32", lambda lay: R.run_gemm_fp8(a8, sa, w8, sw, rb, rr, GELU, True, lay), [FP8_IN] + OUT_LAYOUTS + RES_LAYOUTS)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


# ---------------------------------------------------------------------------------------------------------------- wqkv + RoPE
ROPE = [("tile-bf16", BF16, 0, 2, 70, 1, 2, 256), ("tile-f32", F32, 0, 2, 70, 1, 2, 128), ("tile-257", BF16, 0, 1, 257, 2, 1, 192),
        ("ring-auto", BF16, 0, 1, 1081, 2, 2, 256), ("ring-v6", BF16, 6, 1, 1081, 2, 2, 320), ("ring-v9", BF16, 9, 2, 545, 2, 2, 256)]


@pytest.mark.parametrize("name,dtype,variant,B,S,KVH,G,K", ROPE, ids=[r[0] for r in ROPE])
def test_gemm_qkv_rope_does_not_depend_on_lda_and_ldw(name, dtype, variant, B, S, KVH, G, K):
    """ullsam_gemm_qkv_rope below 1024 rows (the tile kernels) and from 1024 (the ring kernel's RoPE epilogue, auto and forced) with lda = ldw = K + 8 against the
    dense call, cache_pos0 > 0; q_out and the written cache rows are guarded, the rows below cache_pos0 and above cache_pos0 + S keep their sentinel (run_qkv_rope)."""
    N = KVH * (G + 2) * 128
    x, w, bias, _ = _random_operands(B * S, N, K, dtype, S + K)
    g = torch.Generator(device=DEV)
    g.manual_seed(S)
    rows = S + 8
    cos, sin = torch.rand(rows, 128, device=DEV, generator=g) * 2 - 1, torch.rand(rows, 128, device=DEV, generator=g) * 2 - 1
    pos = ((torch.arange(S, device=DEV)[None] + 3 * torch.arange(B, device=DEV)[:, None]) % (S + 5)).to(torch.int32).reshape(-1).contiguous()
    cap, pos0 = S + 6, 3
    fails = []
    with R.forced_variant(variant):
        dense = R.run_qkv_rope(x, w, bias * 0.2, pos, cos, sin, B, S, KVH, G, cap, pos0)
        for lay in (Layout(lda=8), Layout(ldw=8), Layout(lda=8, ldw=8)):
            got = R.run_qkv_rope(x, w, bias * 0.2, pos, cos, sin, B, S, KVH, G, cap, pos0, lay=lay)
            for what, a, b in zip("qkv", got, dense):
                if what != "q":
                    a, b = a[:, :, pos0:pos0 + S], b[:, :, pos0:pos0 + S]
                d = _diff(a, b)
                if d:
                    fails.append(f"{name} {lay} {what}: {d}")
    for what, t in zip("qkv", dense):
        t = t if what == "q" else t[:, :, pos0:pos0 + S]
        assert not bool(torch.isnan(t.float()).any()) and float(t.float().abs().max()) > 0, what
    assert not fails, "\n".join(fails)
