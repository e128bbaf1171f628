"""What tests/test_gemm_abi_cpu.py and tests/test_gemm_abi_gpu.py share: integer operands whose GEMM has ONE right answer in bits, padded and
offset layouts with NaN input padding and sentinel output guards, the float64 definition of the linear epilogues, and raw callers of the GEMM
entry points of include/ullsam_hip.h that pass every leading dimension (ops.gemm and its siblings only ever pass the dense ones).

Exact oracle.  A and W hold seeded integers in [-3, 3], the bias a (periodically) distinct integer per column, the residual one per (m, n), both
within +-125.  Every partial sum of an output is then an integer below 2^24, so the fp32 accumulation is exact in ANY order (the split-K forms
included) and act in {none, ReLU} has one right fp32 result; a bf16 output is its round-to-nearest-even.  `check_bound` asserts the 2^24 limit.

Layouts.  `padded` puts a logical matrix at a leading dimension and a base offset (in elements) into a backing buffer whose other elements
hold `fill` -- NaN for inputs (a kernel that reads padding into a result shows as NaN), the byte SENTINEL for outputs.  An output's tail guard
is GUARD_ROWS = 272 rows of ldc, the tallest tile, so a ragged-row overrun lands in the guard; `assert_untouched` compares every byte
outside the [M, n_out] window with the sentinel (or with a copy taken before the call, for an in-place residual)."""
import contextlib

import torch

DT_F32, DT_BF16 = 0, 1                                  # ULLSAM_DT_*
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SWIGLU = 0, 1, 2, 3   # ULLSAM_ACT_*
HEAD = 64              # guard elements in front of every padded buffer (a multiple of 16 bytes for every element size)
GUARD_ROWS = 272       # tail guard of an output buffer: one tile of the tallest kind (272 x 256)
IN_GUARD_ROWS = 2      # NaN rows behind the last row of an input
SENTINEL = 0xA5        # every byte of an output buffer before the call
E4M3_NAN = 0x7F
VARIANT_DEFAULT = 0
TUNING_DEFAULTS = {2: 2, 3: 1}   # csrc/gemm.hip g_persist, g_ring_splitk
A_MAX, BIAS_MAX, PERIOD = 3, 125, 251
_DT = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}


# ---------------------------------------------------------------------------------------------------------------- integer operands
def check_bound(K, bias=True, residual=True, w_max=A_MAX):
    """Largest magnitude any partial sum of one output can reach, asserted to stay an exactly representable fp32 integer."""
    worst = A_MAX * w_max * K + (BIAS_MAX if bias else 0) + (BIAS_MAX if residual else 0)
    assert worst < 1 << 24, f"K={K}: partial sums up to {worst} are not exact in fp32"
    return worst


def int_matrix(rows, cols, seed, dtype=torch.float32, device="cpu"):
    """Seeded integers in [-3, 3] (generated on the CPU: the same values whatever device they end up on)."""
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randint(-A_MAX, A_MAX + 1, (rows, cols), generator=g, dtype=torch.int8).to(device).to(dtype)


def int_bias(N, device="cpu"):
    """bias[n] = 37 n mod 251 - 125: distinct over any 251 consecutive columns (37 and 251 are coprime)."""
    n = torch.arange(N, dtype=torch.int64, device=device)
    return ((n * 37) % PERIOD - BIAS_MAX).to(torch.float32)


def int_residual(rows, N, device="cpu"):
    """residual[m, n] = (29 m + 13 n) mod 251 - 125: differs from its neighbours in both directions and between rows m and m + r for every
    r that is not a multiple of 251."""
    m = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    n = torch.arange(N, dtype=torch.int64, device=device)[None, :]
    return ((m * 29 + n * 13) % PERIOD - BIAS_MAX).to(torch.float32)


def e4m3_of_small_int(t):
    """OCP e4m3 bytes of integers in [-3, 3] (0 = 0x00, 1 = 0x38, 2 = 0x40, 3 = 0x44, sign 0x80), as uint8."""
    lut = torch.tensor([0x00, 0x38, 0x40, 0x44], dtype=torch.uint8, device=t.device)
    v = t.to(torch.int64)
    assert int(v.abs().max()) <= 3
    return lut[v.abs()] | ((v < 0).to(torch.uint8) << 7)


# ---------------------------------------------------------------------------------------------------------------- the float64 definition
def gemm_ref64(A, W, bias=None, residual=None, res_row_mod=0, act=ACT_NONE):
    """C = act(A W^T + bias) + residual[m mod res_row_mod] in float64 (the linear epilogues and ReLU: the ones with one right answer)."""
    y = A.double() @ W.double().T
    if bias is not None:
        y = y + bias.double()[None, :]
    if act == ACT_RELU:
        y = y.clamp_min(0.0)
    else:
        assert act == ACT_NONE, act
    if residual is not None:
        rows = torch.arange(y.shape[0], device=y.device)
        y = y + residual.double()[rows % res_row_mod if res_row_mod > 0 else rows]
    return y


def expected_bits(y64, out_dtype):
    """float64 -> fp32 (exact for the integer problems) -> the output type by round-to-nearest-even."""
    return y64.to(torch.float32).to(out_dtype)


# ---------------------------------------------------------------------------------------------------------------- padded layouts
def nan_fill(dtype):
    return E4M3_NAN if dtype == torch.uint8 else float("nan")


def window(buf, rows, cols, ld, off=0):
    return buf.as_strided((rows, cols), (ld, 1), HEAD + off)


def address(buf, off=0):
    """The pointer a kernel is handed: element HEAD + off of the backing buffer."""
    return buf.data_ptr() + (HEAD + off) * buf.element_size()


def padded(logical, ld=None, off=0, fill=None, guard_rows=IN_GUARD_ROWS):
    """-> (backing buffer, pointer).  logical [rows, cols] (or 1-D: one row) at leading dimension ld, base offset off elements; everything else = fill."""
    if logical.dim() == 1:
        logical = logical[None, :]
    rows, cols = logical.shape
    ld = cols if ld is None else ld
    assert ld >= cols and off >= 0
    buf = torch.full((HEAD + off + (rows + guard_rows) * ld,), nan_fill(logical.dtype) if fill is None else fill, dtype=logical.dtype, device=logical.device)
    window(buf, rows, cols, ld, off).copy_(logical)
    return buf, address(buf, off)


def out_buffer(rows, cols, ld, off, dtype, device, guard_rows=GUARD_ROWS):
    """-> (backing buffer of `dtype` with every byte = SENTINEL, pointer to the [rows, cols] window at ld / off)."""
    assert ld >= cols and off >= 0
    esz = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((HEAD + off + (rows + guard_rows) * ld) * esz,), SENTINEL, dtype=torch.uint8, device=device).view(dtype)
    return buf, address(buf, off)


def assert_untouched(buf, rows, cols, ld, off=0, before=None):
    """Every byte of buf outside the [rows, cols] window at (ld, off) still holds SENTINEL -- or what `before` (a copy from before the call) holds."""
    esz = buf.element_size()
    outside = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    if rows > 0 and cols > 0:
        window(outside, rows, cols, ld, off).fill_(False)
    got = buf.view(torch.uint8).reshape(-1, esz)
    if before is None:
        changed = (got != SENTINEL).any(1)
    else:
        changed = (got != before.view(torch.uint8).reshape(-1, esz)).any(1)
    bad = changed & outside
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0]) - HEAD - off
        raise AssertionError(f"{int(bad.sum())} elements outside the [{rows}, {cols}] window (ld {ld}, offset {off}) were written; the first is "
                             f"row {i // ld}, column {i % ld} of the window's frame")


# ---------------------------------------------------------------------------------------------------------------- switches
@contextlib.contextmanager
def forced_variant(v):
    from ullsam_amd import _lib
    lib = _lib.load()
    try:
        assert lib.ullsam_set_gemm_variant(v) == 0
        yield
    finally:
        lib.ullsam_set_gemm_variant(VARIANT_DEFAULT)


@contextlib.contextmanager
def tuning(key, value):
    from ullsam_amd import _lib
    lib = _lib.load()
    try:
        assert lib.ullsam_set_gemm_tuning(key, value) == 0
        yield
    finally:
        lib.ullsam_set_gemm_tuning(key, TUNING_DEFAULTS[key])


def ring_ok(dtype, act, N, K, bias_ptr):
    """csrc/gemm.hip gemm_impl: what a forced ring variant (6 / 8 / 9) accepts."""
    bias_v4 = bias_ptr is None or (N % 4 == 0 and bias_ptr % 16 == 0)
    return dtype == torch.bfloat16 and act <= 3 and K % 64 == 0 and K >= 128 and bias_v4 and (act != ACT_SWIGLU or N % 256 == 0)


# ---------------------------------------------------------------------------------------------------------------- raw callers
_WS = {}


def workspace(device):
    """128 MiB of caller-owned scratch (what ops.gemm hands the library), one per device."""
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(128 << 20, dtype=torch.uint8, device=device)
    return ws


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Layout:
    """Paddings (elements added to the dense leading dimension) and base offsets (elements) of one call."""

    def __init__(self, lda=0, ldw=0, ldc=0, ldr=0, c_off=0, r_off=0, bias_off=0, inplace=False):
        self.lda, self.ldw, self.ldc, self.ldr, self.c_off, self.r_off, self.bias_off, self.inplace = lda, ldw, ldc, ldr, c_off, r_off, bias_off, inplace

    def __repr__(self):
        on = {k: v for k, v in vars(self).items() if v}
        return "Layout(%s)" % ", ".join(f"{k}={v}" for k, v in on.items()) if on else "Layout(dense)"


DENSE = Layout()


class Out:
    """The output of one padded call: its backing buffer and window geometry (the window itself: .get())."""

    def __init__(self, buf, rows, cols, ld, off, before=None):
        self.buf, self.rows, self.cols, self.ld, self.off, self.before = buf, rows, cols, ld, off, before

    def get(self):
        return window(self.buf, self.rows, self.cols, self.ld, self.off).clone()

    def check_guard(self):
        assert_untouched(self.buf, self.rows, self.cols, self.ld, self.off, self.before)

    def check_refused(self):
        assert_untouched(self.buf, 0, 0, self.ld, self.off, self.before)


def _epilogue_operands(M, N, n_out, bias, residual, lay, out_f32, odt, dev):
    """Padded bias / residual / output of a call -> (bias ptr, residual ptr, ldr, Out, pointer to C, keep-alive list)."""
    keep = []
    bp = rp = None
    ldr = 0
    if bias is not None:
        bb, bp = padded(bias, off=lay.bias_off, guard_rows=1)
        keep.append(bb)
    if lay.inplace:
        assert residual is not None and out_f32 and residual.shape == (M, n_out) and lay.ldc == lay.ldr and lay.c_off == lay.r_off
        cb, cp = padded(residual, n_out + lay.ldc, lay.c_off, guard_rows=GUARD_ROWS)
        out = Out(cb, M, n_out, n_out + lay.ldc, lay.c_off, before=cb.clone())
        return bp, cp, n_out + lay.ldr, out, cp, keep
    if residual is not None:
        ldr = residual.shape[1] + lay.ldr
        rb, rp = padded(residual, ldr, lay.r_off)
        keep.append(rb)
    cb, cp = out_buffer(M, n_out, n_out + lay.ldc, lay.c_off, odt, dev)
    return bp, rp, ldr, Out(cb, M, n_out, n_out + lay.ldc, lay.c_off), cp, keep


def run_gemm(A, W, bias=None, residual=None, res_row_mod=0, act=ACT_NONE, out_f32=False, lay=DENSE, ws=True, refuse=None):
    """ullsam_gemm on padded copies of the logical operands (NaN padding, sentinel output guard) -> the [M, n_out] result, guard checked.
    refuse: a substring of the error the call must fail with; the output buffer must then be untouched (-> None)."""
    from ullsam_amd import _lib
    M, K = A.shape
    N = W.shape[0]
    dev = A.device
    n_out = N // 2 if act == ACT_SWIGLU else N
    odt = torch.float32 if out_f32 else A.dtype
    ab, ap = padded(A, K + lay.lda)
    wb, wp = padded(W, K + lay.ldw)
    bp, rp, ldr, out, cp, keep = _epilogue_operands(M, N, n_out, bias, residual, lay, out_f32, odt, dev)
    wsb = workspace(dev) if ws else None
    args = (_DT[A.dtype], ap, K + lay.lda, wp, K + lay.ldw, cp, out.ld, int(out_f32), bp, rp, ldr, res_row_mod, act, M, N, K,
            None if wsb is None else wsb.data_ptr(), 0 if wsb is None else wsb.numel(), _stream())
    if refuse is not None:
        try:
            _lib.call("ullsam_gemm", *args)
        except _lib.UllsamError as e:
            assert refuse in str(e), str(e)
            torch.cuda.synchronize()
            out.check_refused()
            return None
        raise AssertionError(f"ullsam_gemm accepted a call it must refuse ({refuse})")
    _lib.call("ullsam_gemm", *args)
    out.check_guard()
    del ab, wb, keep
    return out.get()


def run_gemm_fp8(A8, a_scale, W8, w_scale, bias=None, residual=None, act=ACT_NONE, out_f32=False, lay=DENSE):
    """ullsam_gemm_fp8: A8 / W8 e4m3 bytes (padding = the e4m3 NaN byte), leading dimensions in bytes."""
    from ullsam_amd import _lib
    M, K = A8.shape
    N = W8.shape[0]
    ab, ap = padded(A8, K + lay.lda)
    wb, wp = padded(W8, K + lay.ldw)
    sab, sap = padded(a_scale, guard_rows=1)
    swb, swp = padded(w_scale, guard_rows=1)
    bp, rp, ldr, out, cp, keep = _epilogue_operands(M, N, N, bias, residual, lay, out_f32, torch.float32 if out_f32 else torch.bfloat16, A8.device)
    _lib.call("ullsam_gemm_fp8", ap, K + lay.lda, sap, wp, K + lay.ldw, swp, cp, out.ld, int(out_f32), bp, rp, ldr, act, M, N, K, _stream())
    out.check_guard()
    del ab, wb, sab, swb, keep
    return out.get()


def run_gemm_w8(a, W8, w_scale, bias=None, residual=None, act=ACT_NONE, out_f32=False, lay=DENSE, norm_w=None, eps=0.0, ldx=0):
    """ullsam_gemm_w8: a = bf16 rows [M, K] (dense: the entry takes no lda), or fp32 rows at leading dimension K + ldx with norm_w (the RMSNorm prologue)."""
    from ullsam_amd import _lib
    M, K = a.shape
    N = W8.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    ab, ap = padded(a, K + (ldx if norm_w is not None else 0))
    wb, wp = padded(W8, K + lay.ldw)
    swb, swp = padded(w_scale, guard_rows=1)
    nb, np_ = (None, None) if norm_w is None else padded(norm_w, guard_rows=1)
    bp, rp, ldr, out, cp, keep = _epilogue_operands(M, N, n_out, bias, residual, lay, out_f32, torch.float32 if out_f32 else torch.bfloat16, a.device)
    _lib.call("ullsam_gemm_w8", None if norm_w is not None else ap, ap if norm_w is not None else None, K + ldx, np_, float(eps), wp, K + lay.ldw, swp,
              cp, out.ld, int(out_f32), bp, rp, ldr, act, M, N, K, _stream())
    out.check_guard()
    del ab, wb, swb, nb, keep
    return out.get()


def run_gemm_rmsnorm(x, norm_w, eps, W, bias=None, residual=None, act=ACT_NONE, out_f32=False, lay=DENSE, ldx=0):
    """ullsam_gemm_rmsnorm: x fp32 [M, K] at leading dimension K + ldx (NaN padding), W bf16."""
    from ullsam_amd import _lib
    M, K = x.shape
    N = W.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    xb, xp = padded(x, K + ldx)
    nb, np_ = padded(norm_w, guard_rows=1)
    wb, wp = padded(W, K + lay.ldw)
    bp, rp, ldr, out, cp, keep = _epilogue_operands(M, N, n_out, bias, residual, lay, out_f32, torch.float32 if out_f32 else torch.bfloat16, x.device)
    _lib.call("ullsam_gemm_rmsnorm", xp, K + ldx, np_, float(eps), wp, K + lay.ldw, cp, out.ld, int(out_f32), bp, rp, ldr, act, M, N, K, _stream())
    out.check_guard()
    del xb, nb, wb, keep
    return out.get()


def run_qkv_rope(x, W, bias, pos, cos, sin, B, S, KVH, G, cap, pos0, lay=DENSE, ws=True):
    """ullsam_gemm_qkv_rope -> (q [B S, KVH G 128], k_cache, v_cache [B, KVH, cap, 128]).  q_out and both caches start as sentinel bytes with guards
    around them; the guards and the cache rows outside pos0 .. pos0 + S - 1 must keep the sentinel."""
    from ullsam_amd import _lib
    M, K = x.shape
    N = W.shape[0]
    assert M == B * S and N == KVH * (G + 2) * 128
    dev = x.device
    xb, xp = padded(x, K + lay.lda)
    wb, wp = padded(W, K + lay.ldw)
    bb, bp = (None, None) if bias is None else padded(bias, guard_rows=1)
    pb, pp = padded(pos, fill=-1, guard_rows=1)
    cb, cp = padded(cos, guard_rows=1)
    sb, sp = padded(sin, guard_rows=1)
    nq = KVH * G * 128
    qb, qp = out_buffer(M, nq, nq, 0, x.dtype, dev)
    kb, kp = out_buffer(B * KVH * cap, 128, 128, 0, x.dtype, dev)
    vb, vp = out_buffer(B * KVH * cap, 128, 128, 0, x.dtype, dev)
    wsb = workspace(dev) if ws else None
    _lib.call("ullsam_gemm_qkv_rope", _DT[x.dtype], xp, K + lay.lda, wp, K + lay.ldw, bp, B, S, K, KVH, G, pp, cp, sp, cos.shape[0], qp, kp, vp, cap, pos0,
              None if wsb is None else wsb.data_ptr(), 0 if wsb is None else wsb.numel(), _stream())
    assert_untouched(qb, M, nq, nq)
    res = [window(qb, M, nq, nq).clone()]
    for buf in (kb, vb):
        assert_untouched(buf, B * KVH * cap, 128, 128)
        c = window(buf, B * KVH * cap, 128, 128).clone().reshape(B, KVH, cap, 128)
        rest = torch.cat([c[:, :, :pos0], c[:, :, pos0 + S:]], 2).contiguous().view(torch.uint8)
        assert bool((rest == SENTINEL).all()), "cache rows outside cache_pos0 .. cache_pos0 + S - 1 were written"
        res.append(c)
    del xb, wb, bb, pb, cb, sb
    return res
