"""References for the row kernels (csrc/norm.hip: ullsam_norm, ullsam_norm_panels, ullsam_rows_fp8; csrc/decoder.hip: ullsam_skinny_linear), written from the
operations' definitions and from the comments of the kernels, never from the package's Python: float64 norms and linears (torch, on whatever device the
inputs live), the rounding-error bounds of the fp32 kernels, the address of an element in the activation K-panels, an OCP e4m3 codec on integers and the
row quantiser restated in float32 numpy.  tests/test_rows_ref_cpu.py checks them against independent statements."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24           # unit roundoff of fp32
BF16_STEP = 2.0 ** -8      # worst relative error of one round-to-nearest-even to bf16
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
# the erf-GELU of csrc/common.h (Abramowitz-Stegun 7.1.26 on v_rcp_f32 / v_exp_f32) against 0.5 x (1 + erf(x / sqrt 2)) in float64 OF THE SAME fp32 ARGUMENT:
# measured on an MI355X as |norm(act = GELU) - gelu64(norm(act = none))| over [4099, 60] .. [1027, 3072] outputs with |x| up to 44: 4.69e-7 absolute at most (at
# |x| around 3.1; common.h quotes 4.7e-7 from a CPU model of it), x 4
GELU_ABS = 1.9e-6
# an fp32 sum of K products in the kernels' orders, as a multiple of u sum_k |x_k w_k|: the worst-case constant K + 4 left every err / bound of the Gaussian cases of
# test_row_kernels_gpu.py at or below 0.013 (below 0.01 from K = 256 on), too slack to catch anything; measured against float64 on an MI355X over every (path, K, N, M)
# of that test without an epilogue: 1.54 at most (skinny_linear_mfma_kernel<64, 4>, K = 256; the FMA kernel 0.92), x 4
LIN_SUM = 6.2
GELU_SLOPE = 1.13          # max |d gelu / dx| (1.1289 at x = sqrt 2 ... ): how an error of the argument passes through


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------------------------------------
def norm_ref(x, w=None, b=None, eps=1e-6, rms=False, post_scale=None, post_shift=None, act=ACT_NONE, depth=None):
    """LayerNorm (biased variance) / RMSNorm of the rows of x [rows, D] (fp32 or bf16: the stored values, widened exactly) in float64, in the order of norm_kernel:
    (x - mean) rstd, * w, + b (ignored under rms), * post_scale + post_shift (either may be missing), erf-GELU.  Returns (y float64, e float64): e is the
    elementwise bound on |fp32 kernel - y| BEFORE the output is rounded to its dtype, for a kernel whose two row sums have `depth` additions on the path of a
    term (None: no bound, e is None).

    The bound, to first order in u = 2^-24 (factors (1 + u)^n are taken as 1 + n u; the worst n u below is 60 u = 4e-6):
      mean      the sum of D terms through `depth` levels of additions errs by at most depth u sum|x_i|, the division adds u:   dm = (depth + 1) u mean|x_i|
      c_i       fl(x_i - mean_f) = c_i + d_i,  |d_i| <= dm + u |c_i|                                 (rms: mean = 0, c_i = x_i exactly, dm = 0)
      var       sum (x_i - mean_f)^2 / D = var + dm'^2 exactly (dm' the mean's error), each square carries 3 u (2 from c_i, 1 of the product; a fused multiply-add
                only drops roundings), the sum depth u, the division u:  var_f = (var + dm'^2)(1 + t), |t| <= (depth + 4) u
      rstd      the addition of eps u, sqrtf u, the division u (rsqrtf under rms: 2 ulp = 4 u for the one call), so
                rstd_f = rstd (1 + r), |r| <= t / 2 + dm^2 / (2 (var + eps)) + 4 u
      xhat_i    fl(c_f rstd_f): |err| <= rstd (dm + u |c_i|) + |xhat_i| (r + u)                                        =: e0
      * w, + b  e1 = |w_i| e0 + u |xhat_i w_i|;  e2 = e1 + u |xhat_i w_i + b_i|
      post      o ps + pb (one or two roundings): e3 = |ps| e2 + u (|o ps| + |o ps + pb|)
      GELU      e4 = GELU_SLOPE e3 + GELU_ABS + 4 u |y|  (the polynomial's own error is measured, see GELU_ABS; 4 u for 0.5 x (1 + erf) in fp32)
    Every term scales with the data (|x_i|, |mean|, rstd, |w_i|, |y_i|), which the rows with a large mean or a scale of 2^+-40 need."""
    x64 = x.double()
    D = x64.shape[-1]
    if rms:
        mean = torch.zeros_like(x64[:, :1])
    else:
        mean = x64.mean(-1, keepdim=True)
    c = x64 - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = c * rstd
    y = xhat
    if depth is not None:
        u = U24
        dm = torch.zeros_like(mean) if rms else (depth + 1) * u * x64.abs().mean(-1, keepdim=True)
        r = 0.5 * (depth + 4) * u + dm * dm / (2.0 * (var + eps)) + 4 * u
        e = rstd * (dm + u * c.abs()) + xhat.abs() * (r + u)
    else:
        e = None
    if w is not None:
        w64 = w.double()[None]
        y = y * w64
        if e is not None:
            e = w64.abs() * e + U24 * y.abs()
    if b is not None and not rms:
        y = y + b.double()[None]
        if e is not None:
            e = e + U24 * y.abs()
    if post_scale is not None or post_shift is not None:
        ps = float(post_scale) if post_scale is not None else 1.0
        pb = float(post_shift) if post_shift is not None else 0.0
        o = y * ps
        y = o + pb
        if e is not None:
            e = abs(ps) * e + U24 * (o.abs() + y.abs())
    if act == ACT_GELU:
        y = gelu64(y)
        if e is not None:
            e = GELU_SLOPE * e + GELU_ABS + 4 * U24 * y.abs()
    elif act != ACT_NONE:
        raise ValueError(act)
    return y, e


def norm_depth(kernel, D):
    """additions on the path of one term of a row sum: 2 in the lane's (x + y) + (z + w), MAXV serial `s +=`, the shuffle levels (6 for a wave, 4 for the narrow
    kernel's 16-lane groups) and the 3 additions of the LDS combine of norm_block_kernel's four waves.  kernel: 'narrow', 'wave' (norm_kernel and rows_fp8_kernel:
    MAXV from D as launch_norm / ullsam_rows_fp8 choose it) or 'block'."""
    nv = D // 4
    if kernel == "narrow":
        return 2 + 1 + 4
    if kernel == "block":
        return 2 + (2 if nv <= 512 else 4) + 6 + 3
    if kernel == "wave":
        return 2 + (1 if nv <= 64 else 4 if nv <= 256 else 8 if nv <= 512 else 16 if nv <= 1024 else 32) + 6
    raise ValueError(kernel)


def panel_index(row, k, D):
    """where element (row, k) of a [rows, D] activation sits in its K-panels [ceil(rows / 16)][D / 32][16 rows][32 k] (the NormArgs comment of csrc/norm.hip)"""
    return ((row // 16) * (D // 32) + k // 32) * 512 + (row % 16) * 32 + k % 32


def panel_gather_index(rows_padded, D):
    """int64 [rows_padded, D]: panel_index of every element, for flat.take(...)"""
    r = torch.arange(rows_padded, dtype=torch.int64)[:, None]
    k = torch.arange(D, dtype=torch.int64)[None, :]
    return panel_index(r, k, D)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# OCP e4m3 (fn: no infinities, 0x7f / 0xff are NaN, largest finite 448 = 0x7e) on integers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def e4m3_decode(codes):
    """uint8 codes -> float32 values (exact): sign, 4 exponent bits of bias 7, 3 mantissa bits, subnormals m / 8 * 2^-6"""
    c = np.asarray(codes).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp((8 + m).astype(np.float64), e - 10))
    mag = np.where((c & 0x7F) == 0x7F, np.nan, mag)
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


def e4m3_encode(x):
    """float32 -> uint8 codes: round to nearest, ties to the even code, saturating at +-448 (0x7e / 0xfe); the sign of a zero result is kept; NaN -> 0x7f | sign.
    Integer arithmetic on the float32 bit pattern only."""
    bits = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.int64)
    sign = (bits >> 24) & 0x80
    a = bits & 0x7FFFFFFF
    ex, man = a >> 23, a & 0x7FFFFF
    # normal results (|x| >= 2^-6, ex >= 121): the code is the float's exponent and top three mantissa bits re-biased; a carry of the rounding walks into the exponent
    m = ((ex - 120) << 23) | man
    r, rem = m >> 20, m & 0xFFFFF
    normal = r + ((rem > 0x80000) | ((rem == 0x80000) & ((r & 1) == 1)))
    # subnormal results: |x| / 2^-9 = (2^23 + man) 2^(ex - 141), rounded to an integer 0 .. 8 (8 is the smallest normal's code)
    sh = np.clip(141 - ex, 1, 40)
    sig = np.where(ex > 0, man | 0x800000, 0)              # fp32 subnormals are far below 2^-10: 0
    r2, rem2, half = sig >> sh, sig & ((np.int64(1) << sh) - 1), np.int64(1) << (sh - 1)
    sub = r2 + ((rem2 > half) | ((rem2 == half) & ((r2 & 1) == 1)))
    mag = np.where(ex >= 121, normal, sub)
    mag = np.where(a > 0x7F800000, 0x7F, np.minimum(mag, 0x7E))
    return (sign | mag).astype(np.uint8)


def e4m3_half_spacing(dec):
    """half the distance from |dec| (an e4m3 value) to the next code above it, not below 2^-10 (the subnormals' half step)"""
    a = np.abs(np.asarray(dec, dtype=np.float64))
    return np.maximum(np.exp2(np.floor(np.log2(np.maximum(a, 2.0 ** -6))) - 4), 2.0 ** -10)


def quantise_rows_f32(x):
    """ullsam_rows_fp8 without the LayerNorm, one float32 operation per kernel operation: sc = fl(amax * fl(1 / 448)) (1 for a zero row), inv = fl(1 / sc),
    q = enc(clamp(fl(x * inv), +-448)).  x float32 [rows, D] -> (codes uint8 [rows, D], sc float32 [rows])."""
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x).max(-1)
    c448 = np.float32(1.0) / np.float32(448.0)
    with np.errstate(over="ignore"):
        sc = np.where(amax > 0, amax * c448, np.float32(1.0)).astype(np.float32)
        inv = (np.float32(1.0) / sc).astype(np.float32)
        t = (x * inv[:, None]).astype(np.float32)
    t = np.minimum(np.maximum(t, np.float32(-448.0)), np.float32(448.0))
    return e4m3_encode(t), sc


def layer_norm_f32(x, w, b, eps):
    """the LayerNorm of rows_fp8_kernel in float32 numpy (numpy's pairwise sums, not the kernel's order): the stand-in of test_rows_ref_cpu.py"""
    x = np.asarray(x, dtype=np.float32)
    D = np.float32(x.shape[-1])
    mean = (x.sum(-1, dtype=np.float32) / D)[:, None]
    c = x - mean
    var = ((c * c).sum(-1, dtype=np.float32) / D)[:, None]
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    return (c * rstd * w[None] + b[None]).astype(np.float32)


FP8_LN_EPS = 1e-6


def fp8_ln_case(D, bf16, rows=67):
    """the inputs of the quantiser-with-LayerNorm tests, shared by the CPU check of the seeds and the GPU test: x [rows, D] (rounded to bf16 if asked; returned as
    float32 either way), w, b float32 [D]"""
    rng = np.random.default_rng(1000 * D + (1 if bf16 else 0))
    x = (rng.standard_normal((rows, D), dtype=np.float32) * np.float32(2.0) + np.float32(0.3)).astype(np.float32)
    if bf16:
        x = torch.from_numpy(x).bfloat16().float().numpy()
    w = (1.0 + 0.25 * rng.standard_normal(D, dtype=np.float32)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D, dtype=np.float32)).astype(np.float32)
    return x, w, b


def fp8_ln_ref(x, w, b, eps=FP8_LN_EPS):
    """float64: (y64 [rows, D], e [rows, D] the fp32 bound of the LayerNorm as rows_fp8_kernel computes it, sc64 = amax / 448, codes enc(y64 / sc64))"""
    D = x.shape[-1]
    y, e = norm_ref(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), eps, depth=norm_depth("wave", D))
    y, e = y.numpy(), e.numpy()
    sc = np.abs(y).max(-1) / 448.0
    t = np.clip(y / sc[:, None], -448.0, 448.0)
    return y, e, sc, e4m3_encode(t.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------------------------------------------------------
def linear_ref(x, wt, b=None, res=None, act=ACT_NONE):
    """float64 act(x @ W^T + b) + res with wt = W^T [K, N]; -> (y, e): e is min(K + 4, LIN_SUM) u sum_k |x_k w_k| for the fp32 sum of the K products ((K + 4) u is the
    worst case of any order; LIN_SUM is the measured constant that replaces it, see there), plus the epilogue's roundings: u |v + b| of the bias,
    GELU_SLOPE e + GELU_ABS + 4 u |y| of the erf-GELU (ReLU passes e through), u |y| of the residual."""
    x64, w64 = x.double(), wt.double()
    K = x64.shape[-1]
    y = x64 @ w64
    e = min(K + 4, LIN_SUM) * U24 * (x64.abs() @ w64.abs())
    if b is not None:
        y = y + b.double()[None]
        e = e + U24 * y.abs()
    if act == ACT_GELU:
        y = gelu64(y)
        e = GELU_SLOPE * e + GELU_ABS + 4 * U24 * y.abs()
    elif act == ACT_RELU:
        y = y.clamp(min=0.0)
    elif act != ACT_NONE:
        raise ValueError(act)
    if res is not None:
        y = y + res.double()
        e = e + U24 * y.abs()
    return y, e
