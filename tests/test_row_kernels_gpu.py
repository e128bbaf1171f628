"""The row kernels -- ullsam_norm / ullsam_norm_panels (csrc/norm.hip: norm_narrow_kernel, norm_kernel<1 / 4 / 8 / 16>, norm_block_kernel<2 / 4>), ullsam_rows_fp8
(rows_fp8_kernel<4 / 8 / 16 / 32>) and ullsam_skinny_linear (csrc/decoder.hip: skinny_linear_mfma_kernel<32,4 / 64,4 / 128,4 / 64,16 / 128,16>,
skinny_linear_kernel<32 / 64>) -- every cell of their dispatch by name, against the float64 references of tests/rows_ref.py, at the strides, dtypes, row counts and
D / K / N / M on both sides of every switch, with sentinels around every strided output.

Tolerances follow the rule at the top of tests/test_infer_kernels_gpu.py.  The norms and the linears are held to the DERIVED fp32 bounds of rows_ref.norm_ref /
rows_ref.linear_ref (they scale with the data; one bf16 step of 2^-8 relative on top for bf16 outputs); the erf-GELU's own error in them is measured (rows_ref.GELU_ABS).
Whatever has an exact answer is compared in bits: panel output against row-major output, the quantiser without LayerNorm against its float32 restatement, the
linears on small integers, constant rows, equal rows, and rows next to poisoned rows."""
import numpy as np
import pytest
import torch

from tests import rows_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)]
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as o
    return o


def _lib():
    from ullsam_amd import _lib as L
    return L


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dt(dtype):
    return 0 if dtype == F32 else 1


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _randn(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, device=DEV, generator=g, dtype=F32) * scale + shift


def _within(got, ref64, bound, what, quiet=True):
    """|got - ref| <= bound elementwise, everything finite; returns the worst share of the bound (printed by the caller, once per test)"""
    got64 = got.double()
    assert got64.shape == ref64.shape, (what, got64.shape, ref64.shape)
    assert bool(torch.isfinite(got64).all()), f"{what}: non-finite values"
    e = (got64 - ref64).abs()
    ratio = float((e / bound.clamp(min=1e-300)).max())
    if not quiet:
        print(f"{what}: max |err| {float(e.max()):.3e}, worst err / bound {ratio:.3f}")
    assert bool((e <= bound).all()), f"{what}: max |err| {float(e.max()):.3e}, worst err / bound {ratio:.3f}"
    return ratio


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. norms
# ---------------------------------------------------------------------------------------------------------------------------------------------
SENT = -7777.0        # in the gaps of strided outputs and in the pad rows of panel buffers (a bf16 buffer holds its rounding; compared as stored)
JUNK = 3.0e4          # in the gaps of strided inputs: a kernel that read them would show it in the statistics


def _norm(x, out_dtype, w=None, b=None, eps=EPS, rms=False, act=0, ps=None, pb=None, strided=False):
    """ullsam_norm through the library entry.  strided: in_stride = D + 4 and out_stride = D + 8, the input gaps hold JUNK, the output is filled with a sentinel
    first and its gaps must still hold it."""
    rows, D = x.shape
    if not strided:
        out = torch.empty((rows, D), dtype=out_dtype, device=DEV)
        _lib().call("ullsam_norm", x.data_ptr(), _dt(x.dtype), D, out.data_ptr(), _dt(out_dtype), D, _p(w), _p(b), rows, D, eps, int(rms), act, _p(ps), _p(pb), _s())
        return out
    xb = torch.full((rows, D + 4), JUNK, dtype=x.dtype, device=DEV)
    xb[:, :D] = x
    ob = torch.full((rows, D + 8), SENT, dtype=out_dtype, device=DEV)
    sent = ob[0, 0].clone()
    _lib().call("ullsam_norm", xb.data_ptr(), _dt(x.dtype), D + 4, ob.data_ptr(), _dt(out_dtype), D + 8, _p(w), _p(b), rows, D, eps, int(rms), act, _p(ps), _p(pb), _s())
    assert bool((ob[:, D:] == sent).all()), "the gap between the output rows was written"
    return ob[:, :D].contiguous()


def _norm_bound(y64, e, out_dtype):
    return e if out_dtype == F32 else y64.abs() * R.BF16_STEP + e


# name -> (kernel of rows_ref.norm_depth, Ds, row counts, ullsam_set_norm_variant)
CELLS = {
    "narrow": ("narrow", (4, 36, 60, 64), (4096, 4099), 0),
    "wave1_below_narrow": ("wave", (4, 36, 60, 64), (4095,), 0),
    "wave1": ("wave", (252, 256), (5, 67), 0),
    "wave4": ("wave", (260, 1024), (5, 67), 0),
    "wave8": ("wave", (1028, 2044), (5, 67), 0),
    "wave8_between_block": ("wave", (2048,), (65, 1023), 0),
    "wave16_between_block": ("wave", (2052, 4096), (65, 1023), 0),
    "wave8_16_by_variant": ("wave", (2048, 4096), (1027,), 1),
    "block2": ("block", (2048,), (1, 3, 64, 1024, 1027), 0),
    "block4": ("block", (2052, 3072, 4096), (1, 3, 64, 1024, 1027), 0),
}
# one D (and row count) per kernel for the sweeps and the invariants; the *_P2 entries are powers of two (constant rows: the mean is exact)
KERNELS = {
    "narrow": ("narrow", 60, 4099, 0), "wave1": ("wave", 252, 67, 0), "wave4": ("wave", 260, 67, 0), "wave8": ("wave", 2044, 67, 0),
    "wave16": ("wave", 2052, 65, 0), "block2": ("block", 2048, 1027, 0), "block4": ("block", 3072, 1027, 0),
}
KERNELS_P2 = {
    "narrow": ("narrow", 64, 4099, 0), "wave1": ("wave", 256, 67, 0), "wave4": ("wave", 1024, 67, 0), "wave8": ("wave", 2048, 67, 0),
    "wave16": ("wave", 4096, 67, 0), "block2": ("block", 2048, 3, 0), "block4": ("block", 4096, 1027, 0),
}


class _variant:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        if self.v:
            _lib().load().ullsam_set_norm_variant(self.v)

    def __exit__(self, *a):
        _lib().load().ullsam_set_norm_variant(0)


@pytest.mark.parametrize("cell", list(CELLS))
def test_norm_every_cell_of_launch_norm(cell):
    """LayerNorm with w and b in every cell of launch_norm, all four (in, out) dtype pairs, and one strided case per shape (in_stride = D + 4, out_stride = D + 8,
    sentinel intact; the pair it uses rotates over the shapes) against float64 within the derived bound.  Reaches, by cell: narrow -> norm_narrow_kernel (nv <= 16,
    rows >= 4096); wave1_below_narrow -> norm_kernel<1> at the same D with 4095 rows; wave1 -> norm_kernel<1> (nv <= 64); wave4 -> norm_kernel<4> (nv 65 .. 256);
    wave8 -> norm_kernel<8> (nv 257 .. 511); wave8_between_block / wave16_between_block -> norm_kernel<8> / <16> at nv >= 512 with 64 < rows < 1024;
    wave8_16_by_variant -> the same two through ullsam_set_norm_variant(1) at 1027 rows; block2 -> norm_block_kernel<2> (nv == 512, rows <= 64 or >= 1024);
    block4 -> norm_block_kernel<4> (nv > 512).  Each in the <float, float>, <float, bf16>, <bf16, bf16> and <bf16, float> form."""
    kernel, Ds, rows_list, variant = CELLS[cell]
    worst, n = {F32: 0.0, BF16: 0.0}, 0
    with _variant(variant):
        for D in Ds:
            g = _gen(D)
            w, b = _randn((D,), g), _randn((D,), g)
            for rows in rows_list:
                x32 = _randn((rows, D), g, 2.0, 0.3)
                s_in, s_out = PAIRS[n % 4]          # the dtype pair of this shape's strided case
                n += 1
                for in_dt in (F32, BF16):
                    x = x32.to(in_dt)
                    y64, e = R.norm_ref(x, w, b, EPS, depth=R.norm_depth(kernel, D))
                    for out_dt in (F32, BF16):
                        r = _within(_norm(x, out_dt, w, b), y64, _norm_bound(y64, e, out_dt), f"{cell} D={D} rows={rows} {in_dt}->{out_dt}")
                        worst[out_dt] = max(worst[out_dt], r)
                    if in_dt == s_in:
                        got = _norm(x, s_out, w, b, strided=True)
                        r = _within(got, y64, _norm_bound(y64, e, s_out), f"{cell} D={D} rows={rows} strided {s_in}->{s_out}")
                        worst[s_out] = max(worst[s_out], r)
    print(f"{cell}: worst err / bound {worst[F32]:.3f} (fp32 outputs), {worst[BF16]:.3f} (bf16 outputs)")


@pytest.mark.parametrize("name", list(KERNELS))
def test_norm_option_sweep(name):
    """rms x {no w, w} x {no b, b} x {no post, post_scale only, post_shift only, both} x {no act, GELU}, fp32 -> fp32, at one D per kernel (norm_narrow_kernel D = 60,
    norm_kernel<1> 252, <4> 260, <8> 2044, <16> 2052, norm_block_kernel<2> 2048, <4> 3072), against float64 within the derived bound.  Under rms, b is passed and
    must be ignored."""
    kernel, D, rows, variant = KERNELS[name]
    g = _gen(100 + D)
    x, w, b = _randn((rows, D), g, 2.0, 0.3), _randn((D,), g), _randn((D,), g)
    ps, pb = torch.tensor([0.37], device=DEV), torch.tensor([-1.25], device=DEV)
    worst = 0.0
    for rms in (False, True):
        for ww in (None, w):
            for bb in (None, b):
                for pps, ppb in ((None, None), (ps, None), (None, pb), (ps, pb)):
                    for act in (R.ACT_NONE, R.ACT_GELU):
                        y64, e = R.norm_ref(x, ww, bb, EPS, rms, None if pps is None else pps[0], None if ppb is None else ppb[0], act, R.norm_depth(kernel, D))
                        got = _norm(x, F32, ww, bb, EPS, rms, act, pps, ppb)
                        what = f"{name} rms={rms} w={ww is not None} b={bb is not None} ps={pps is not None} pb={ppb is not None} act={act}"
                        worst = max(worst, _within(got, y64, e, what))
    print(f"{name}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(KERNELS))
def test_norm_rows_with_a_large_mean_and_scaled_rows(name):
    """Data beyond unit Gaussians, LayerNorm and RMSNorm with w and b, fp32 -> fp32 and bf16 -> bf16, per kernel (the instantiations of test_norm_option_sweep):
    rows whose mean is 1000 times their spread, and rows scaled by 2^40 and 2^-40 next to unit rows.  |x| stays below 1e15, so that the fp32 squares (< 1e30, their
    sum over 4096 < 1e34) neither overflow nor vanish: outside that range the fp32 kernel and float64 disagree by design.  The bound scales with the data."""
    kernel, D, rows, variant = KERNELS[name]
    g = _gen(200 + D)
    w, b = _randn((D,), g), _randn((D,), g)
    big = _randn((rows, D), g) + 1000.0
    scale = torch.tensor([1.0, 2.0 ** 40, 2.0 ** -40], device=DEV)[torch.arange(rows, device=DEV) % 3][:, None]
    scaled = _randn((rows, D), g, 2.0, 0.3) * scale
    assert float(scaled.abs().max()) < 1e15
    worst = 0.0
    for what, x32 in (("mean1000", big), ("2^+-40", scaled)):
        for dt in (F32, BF16):
            x = x32.to(dt)
            for rms in (False, True):
                y64, e = R.norm_ref(x, w, b, EPS, rms, depth=R.norm_depth(kernel, D))
                worst = max(worst, _within(_norm(x, dt, w, b, rms=rms), y64, _norm_bound(y64, e, dt), f"{name} {what} {dt} rms={rms}"))
    print(f"{name}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(KERNELS_P2))
def test_norm_constant_rows_are_exact(name):
    """Constant rows of a power of two (2^-10 .. 2^9 by row) at a power-of-two D: every partial sum is exact, so the mean is the value, the centred row is 0 and the
    LayerNorm output is b exactly -- after post_scale = 0.5 and post_shift = 2 it is fl(0.5 b + 2), one rounding whether fused or not; under rms with w = 0 it is 0,
    and post_shift after post.  norm_narrow_kernel D = 64, norm_kernel<1> 256, <4> 1024, <8> 2048 at 67 rows, <16> 4096 at 67 rows, norm_block_kernel<2> 2048 at 3
    rows, <4> 4096 at 1027 rows; fp32 and bf16 inputs, fp32 output."""
    kernel, D, rows, variant = KERNELS_P2[name]
    g = _gen(300 + D)
    w, b = _randn((D,), g), _randn((D,), g)
    val = torch.exp2((torch.arange(rows, device=DEV) % 20 - 10).float())[:, None].expand(rows, D).contiguous()
    ps, pb = torch.tensor([0.5], device=DEV), torch.tensor([2.0], device=DEV)
    zero = torch.zeros((D,), device=DEV)
    for dt in (F32, BF16):
        x = val.to(dt)
        assert torch.equal(_norm(x, F32, w, b), b[None].expand(rows, D))
        assert torch.equal(_norm(x, F32, w, b, ps=ps, pb=pb), (b * 0.5 + 2.0)[None].expand(rows, D))
        assert torch.equal(_norm(x, F32, zero, None, rms=True), torch.zeros((rows, D), device=DEV))
        assert torch.equal(_norm(x, F32, zero, b, rms=True, ps=ps, pb=pb), torch.full((rows, D), 2.0, device=DEV))


@pytest.mark.parametrize("name", list(KERNELS))
def test_norm_a_row_does_not_depend_on_its_neighbours(name):
    """Two invariants without a tolerance, per kernel (the instantiations of test_norm_option_sweep; fp32 -> fp32 and bf16 -> bf16, LayerNorm and RMSNorm):
    (a) equal rows give bit-equal output rows; (b) with row 1 replaced by NaN, row 6 by +Inf and row rows - 2 by 3e38, every other row keeps the bits of the clean
    run.  In norm_narrow_kernel rows 4 j .. 4 j + 3 share a wave (rows 0 - 3, 4 - 7 and 4096 - 4098 each hold one poisoned row); in norm_kernel they share a
    workgroup; norm_block_kernel's workgroups share nothing but must not either.  Non-finite arithmetic does not fault."""
    kernel, D, rows, variant = KERNELS[name]
    g = _gen(400 + D)
    w, b = _randn((D,), g), _randn((D,), g)
    x32 = _randn((rows, D), g, 2.0, 0.3)
    poison = {1: float("nan"), 6: float("inf"), rows - 2: 3e38}
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[list(poison)] = False
    for dt in (F32, BF16):
        for rms in (False, True):
            x = x32.to(dt)
            clean = _norm(x, dt, w, b, rms=rms)
            same = _norm(x[3:4].expand(rows, D).contiguous(), dt, w, b, rms=rms)
            assert torch.equal(_bits(same), _bits(clean[3:4].expand(rows, D))), "equal rows, different outputs"
            xp = x.clone()
            for r, v in poison.items():
                xp[r] = v
            got = _norm(xp, dt, w, b, rms=rms)
            assert torch.equal(_bits(got[keep]), _bits(clean[keep])), "a poisoned row changed its neighbours"
            assert bool(torch.isfinite(clean.float()).all()) and not bool(torch.isfinite(got[1].float()).any())


def _panel_buffer(rows_padded, D):
    """a sentinel-filled bf16 buffer of rows_padded * D elements on a 1 KiB boundary"""
    raw = torch.full((rows_padded * D + 512,), SENT, dtype=BF16, device=DEV)
    off = (-raw.data_ptr() % 1024) // 2
    return raw[off:off + rows_padded * D]


@pytest.mark.parametrize("rows,D", [(5, 2048), (64, 2048), (1027, 2048), (5, 4096), (64, 4096), (1027, 4096), (67, 32), (67, 1280)])
def test_norm_panels_hold_the_row_major_bits(rows, D):
    """ullsam_norm_panels with out_panels = 1: the panel buffer, unpacked with the address formula of the NormArgs comment (rows_ref.panel_index), equals the
    row-major bf16 output of ullsam_norm in bits, and the pad rows of the sentinel-filled buffer are untouched.  norm_block_kernel<2> (D = 2048) and <4> (D = 4096)
    at 5 and 64 rows (the grid rounded up to 16, the workgroups of each 16 dealt as 0, 2, .. 14, 1, 3, .. 15) and at 1027; norm_kernel<1> (D = 32) and <8> (D = 1280)
    at 67 rows; <float, bf16> with LayerNorm + GELU and <bf16, bf16> with RMSNorm."""
    g = _gen(500 + D + rows)
    w, b = _randn((D,), g), _randn((D,), g)
    x32 = _randn((rows, D), g, 2.0, 0.3)
    pad = (rows + 15) // 16 * 16
    idx = R.panel_gather_index(pad, D).to(DEV)
    for dt, rms, act in ((F32, False, R.ACT_GELU), (BF16, True, R.ACT_NONE)):
        x = x32.to(dt)
        flat = _panel_buffer(pad, D)
        sent = flat[0].clone()
        _lib().call("ullsam_norm_panels", x.data_ptr(), _dt(dt), D, flat.data_ptr(), _p(w), _p(b), rows, D, EPS, int(rms), act, None, None, 1, _s())
        got = flat[idx.reshape(-1)].reshape(pad, D)
        assert torch.equal(_bits(got[:rows]), _bits(_norm(x, BF16, w, b, rms=rms, act=act)))
        assert bool((got[rows:] == sent).all()), "pad rows of the panel buffer were written"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. ullsam_rows_fp8
# ---------------------------------------------------------------------------------------------------------------------------------------------
FP8_DS = [4, 252, 256, 260, 1024, 1028, 2048, 2052, 4096, 4100, 5120, 8192]      # MAXV 4 | 8 | 16 | 32 switches at D = 1024 / 2048 / 4096
ROW_KINDS = ["amax448", "zero", "amax448/8", "amax448*32", "negzero", "gauss", "outlier", "tiny", "huge"]


def _special_row(rng, D, k, negative):
    """amax = 448 2^k exactly (sc = 2^k), with the exact ties 17 2^k and 19 2^k, the subnormal ties 2^(k - 10) and 1.5 2^(k - 9) and the smallest normal
    2^(k - 6); everything is a bf16 value times a power of two.  Returns the row and the positions of the seven specials (the first min(7, D) of them)."""
    s = np.float32(2.0 ** k)
    row = (np.clip(rng.standard_normal(D, dtype=np.float32) * 50, -400, 400) * s).astype(np.float32)
    spec = np.float32([-448.0 if negative else 448.0, 17, 19, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.0 ** -6, -17]) * s
    n = min(len(spec), D)
    pos = np.arange(n) * max(1, D // n)
    row[pos] = spec[:n]
    return row, pos


def _fp8_rows(rows, D, bf16):
    rng = np.random.default_rng(17 * D + rows)
    x = np.zeros((rows, D), np.float32)
    meta = {}
    for r in range(rows):
        kind = ROW_KINDS[r % len(ROW_KINDS)]
        gauss = (rng.standard_normal(D, dtype=np.float32) * 2 + np.float32(0.3)).astype(np.float32)
        if kind.startswith("amax448"):
            k = {"amax448": 0, "amax448/8": -3, "amax448*32": 5}[kind]
            x[r], pos = _special_row(rng, D, k, negative=(r // len(ROW_KINDS)) % 2 == 1)
            meta[r] = (k, pos)
        elif kind == "zero":
            pass
        elif kind == "negzero":
            x[r] = gauss
            x[r, ::3] = -0.0
        elif kind == "gauss":
            x[r] = gauss
        elif kind == "outlier":
            x[r] = gauss
            x[r, D // 2] = 1000.0 * np.abs(gauss).max()
        elif kind == "tiny":
            x[r] = gauss * np.float32(2.0 ** -100)
        elif kind == "huge":
            x[r] = gauss * np.float32(2.0 ** 60)
    if bf16:
        x = torch.from_numpy(x).bfloat16().float().numpy()
    return x, meta


def _rows_fp8(x, w=None, b=None, eps=0.0, strided=False):
    """ullsam_rows_fp8 through the library entry -> (codes uint8 [rows, D], scales fp32 [rows]) as numpy.  strided: in_stride = D + 4 (gaps hold 1e30, which would
    show in amax), out_stride = D + 4 bytes over a 0xA5-filled buffer whose gaps must stay."""
    rows, D = x.shape
    ins, outs = (D + 4, D + 4) if strided else (D, D)
    xb = torch.full((rows, ins), 1e30, dtype=x.dtype, device=DEV)
    xb[:, :D] = x
    q = torch.full((rows, outs), 0xA5, dtype=torch.uint8, device=DEV)
    sc = torch.full((rows,), -1.0, device=DEV)
    _lib().call("ullsam_rows_fp8", xb.data_ptr(), _dt(x.dtype), ins, q.data_ptr(), outs, sc.data_ptr(), _p(w), _p(b), rows, D, eps, _s())
    assert bool((q[:, D:] == 0xA5).all()), "the gap between the output rows was written"
    return q[:, :D].cpu().numpy(), sc.cpu().numpy()


def _check_fp8_exact(x_np, meta, dtype, strided):
    q, sc = _rows_fp8(torch.from_numpy(x_np).to(DEV).to(dtype), strided=strided)
    q_ref, sc_ref = R.quantise_rows_f32(x_np)
    assert np.array_equal(sc.view(np.uint32), sc_ref.view(np.uint32)), "scales differ from the float32 restatement"
    assert np.array_equal(q, q_ref), f"{int((q != q_ref).sum())} codes differ from the float32 restatement"
    rows, D = x_np.shape
    for r in range(rows):
        if ROW_KINDS[r % len(ROW_KINDS)] == "zero":
            assert sc[r] == 1.0 and not q[r].any()
    dec = R.e4m3_decode(q)
    for r, (k, pos) in meta.items():          # the specials by name (the restatement agrees; tests/test_rows_ref_cpu.py derives them by hand)
        assert sc[r] == np.float32(2.0 ** k)
        want = [448.0 if x_np[r, pos[0]] > 0 else -448.0, 16.0, 20.0, 0.0, 2.0 ** -8, 2.0 ** -6, -16.0][:len(pos)]
        assert dec[r, pos].tolist() == want and q[r, pos[0]] in (0x7E, 0xFE)


@pytest.mark.parametrize("D", FP8_DS)
def test_rows_fp8_equals_its_float32_restatement_in_bits(D):
    """ullsam_rows_fp8 without LayerNorm at rows in {1, 5, 67}, fp32 and bf16 input: scales and codes equal rows_ref.quantise_rows_f32 in bits, on rows built to hold
    a zero row (scale 1, codes 0), -0.0, amax = 448 2^k for k in {0, -3, 5} (scale 2^k; the amax element is 0x7e / 0xfe; the ties 17 -> 16, 19 -> 20,
    2^-10 -> 0, 1.5 2^-9 -> 2^-8; the smallest normal), an outlier of 1000 times the rest, rows scaled by 2^-100 and by 2^60.
    rows_fp8_kernel<float / bf16, MAXV>: MAXV = 4 for D <= 1024, 8 for 1028 .. 2048, 16 for 2052 .. 4096, 32 for 4100 .. 8192."""
    for rows in (1, 5, 67):
        for dtype in (F32, BF16):
            x_np, meta = _fp8_rows(rows, D, dtype == BF16)
            _check_fp8_exact(x_np, meta, dtype, strided=False)


@pytest.mark.parametrize("D", [256, 1028, 2052, 4100])
def test_rows_fp8_strided(D):
    """in_stride = D + 4 elements and out_stride = D + 4 bytes, once per MAXV (rows_fp8_kernel<., 4> D = 256, <., 8> 1028, <., 16> 2052, <., 32> 4100), fp32 and bf16:
    the same bits as the restatement, the 0xA5 between the output rows intact, the 1e30 between the input rows unseen."""
    for dtype in (F32, BF16):
        x_np, meta = _fp8_rows(67, D, dtype == BF16)
        _check_fp8_exact(x_np, meta, dtype, strided=True)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D", [256, 1280, 5120])
def test_rows_fp8_with_layernorm_against_float64(D, bf16):
    """ullsam_rows_fp8 with LayerNorm (rows_fp8_kernel<., 4> D = 256, <., 8> D = 1280, <., 32> D = 5120, the fp8 ViT's MLP rows) against float64, with e the derived
    fp32 bound of the LayerNorm (rows_ref.norm_ref at the depth of the MAXV reached):
      scale   |sc - amax64 / 448| <= e_max / 448 + 2^-23 sc
      codes   |dec(q) sc - y64| <= max(half the e4m3 spacing at |dec(q)|, 2^-10) sc + e, elementwise
      and at most 0.5 % of the codes differ from enc(y64 / sc64) (tests/test_rows_ref_cpu.py holds a float32 numpy LayerNorm on the same inputs to a tenth of that)."""
    x, w, b = R.fp8_ln_case(D, bf16)
    y64, e, sc64, q64 = R.fp8_ln_ref(x, w, b)
    q, sc = _rows_fp8(torch.from_numpy(x).to(DEV).to(BF16 if bf16 else F32), torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), R.FP8_LN_EPS)
    sc_err, sc_bound = np.abs(sc.astype(np.float64) - sc64), e.max(-1) / 448.0 + 2.0 ** -23 * sc
    dec = R.e4m3_decode(q).astype(np.float64)
    assert np.isfinite(dec).all()
    err, bound = np.abs(dec * sc[:, None] - y64), R.e4m3_half_spacing(dec) * sc[:, None] + e
    frac = float((q != q64).mean())
    print(f"D={D} bf16={bf16}: scale worst err / bound {float((sc_err / sc_bound).max()):.3f}, codes worst err / bound {float((err / bound).max()):.3f}, "
          f"{frac * 100:.4f} % of the codes differ from enc(y64 / sc64)")
    assert (sc_err <= sc_bound).all() and (err <= bound).all() and frac <= 0.005


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. ullsam_skinny_linear
# ---------------------------------------------------------------------------------------------------------------------------------------------
EPILOGUES = [(R.ACT_NONE, True, True), (R.ACT_GELU, True, False), (R.ACT_RELU, False, True), (R.ACT_NONE, False, False), (R.ACT_GELU, False, True),
             (R.ACT_RELU, True, False)]          # (act, b, res)
SKINNY = {  # path -> (Ks, Ns, Ms, mfma switch)
    "mfma": ((128, 256, 512, 1024, 2048), (32, 96), (1, 31, 32, 33, 65), 1),
    "fma_kc32": ((128, 384, 640), (1, 4, 63, 65, 130), (1, 15, 16, 17, 33), 1),
    "fma_kc64": ((256, 768, 1536), (1, 4, 63, 65, 130), (1, 15, 16, 17, 33), 1),
    "fma_behind_switch": ((128, 256, 512, 1024, 2048), (32, 96), (33,), 0),
}
SKINNY_CASES = [(path, K) for path, v in SKINNY.items() for K in v[0]]
YSENT = -12345.0


def _skinny(x, wt, b, res, act):
    """ullsam_skinny_linear through the library entry with ldx = K + 4 (the gap holds 1e30), ldr = N + 3 and ldy = N + 5 over a sentinel-filled y whose gaps must stay"""
    M, K = x.shape
    N = wt.shape[1]
    xb = torch.full((M, K + 4), 1e30, device=DEV)
    xb[:, :K] = x
    rb = None
    if res is not None:
        rb = torch.full((M, N + 3), 1e30, device=DEV)
        rb[:, :N] = res
    y = torch.full((M, N + 5), YSENT, device=DEV)
    _lib().call("ullsam_skinny_linear", xb.data_ptr(), K + 4, wt.data_ptr(), _p(b), _p(rb), N + 3, y.data_ptr(), N + 5, M, N, K, act, _s())
    assert bool((y[:, N:] == YSENT).all()), "the gap between the output rows was written"
    return y[:, :N].contiguous()


@pytest.mark.parametrize("path,K", SKINNY_CASES)
def test_skinny_linear_against_float64_and_exact_on_integers(path, K):
    """ullsam_skinny_linear with ldx = K + 4, ldr = N + 3, ldy = N + 5 at every (N, M) of its path, the epilogue (act in {none, GELU, ReLU}, b / res on and off)
    rotating so that every K sees every one:
      mfma               skinny_linear_mfma_kernel<32, 4> K = 128, <64, 4> 256, <128, 4> 512, <64, 16> 1024, <128, 16> 2048; N in {32, 96}, M in {1, 31, 32, 33, 65}
      fma_kc32           skinny_linear_kernel<32> K in {128, 384, 640} (K % 256 != 0); N in {1, 4, 63, 65, 130}, M in {1, 15, 16, 17, 33}
      fma_kc64           skinny_linear_kernel<64> K in {256, 768, 1536}; the same N and M
      fma_behind_switch  skinny_linear_kernel<32> (K = 128) / <64> at the MFMA shapes with ullsam_set_skinny_linear_mfma(0); N in {32, 96}, M = 33
    (1) Gaussian x, W / sqrt K, b, res against float64 within rows_ref.linear_ref's bound: LIN_SUM u sum_k |x_k w_k| plus the epilogue's roundings -- the derived
    (K + 4) u sum_k |x_k w_k| left the worst err / bound at 0.013 (K = 128) down to 0.0004 (K = 2048), so its constant is replaced by the measured one x 4.
    (2) x and W integers in [-4, 4], b and res integers in [-8, 8], no activation or ReLU: every partial sum is an integer below 2^24, exact in fp32 in any order, and
    the output equals the integer result in bits -- a dropped chunk, a swapped lane half or a wrong wave share of K has no tolerance to hide behind."""
    Ks, Ns, Ms, mfma = SKINNY[path]
    lib = _lib().load()
    old = lib.ullsam_set_skinny_linear_mfma(mfma)
    worst, n = 0.0, Ks.index(K)
    try:
        g = _gen(600 + K)
        for N in Ns:
            wt = _randn((K, N), g, K ** -0.5)
            wi = torch.randint(-4, 5, (K, N), device=DEV, generator=g).float()
            b, bi = _randn((N,), g), torch.randint(-8, 9, (N,), device=DEV, generator=g).float()
            for M in Ms:
                x, res = _randn((M, K), g), _randn((M, N), g)
                xi = torch.randint(-4, 5, (M, K), device=DEV, generator=g).float()
                ri = torch.randint(-8, 9, (M, N), device=DEV, generator=g).float()
                few = len(Ns) * len(Ms) < len(EPILOGUES)            # too few shapes for the rotation to show this K every epilogue: all of them at each shape
                for act, use_b, use_r in (EPILOGUES if few else [EPILOGUES[n % len(EPILOGUES)]]):
                    y64, e = R.linear_ref(x, wt, b if use_b else None, res if use_r else None, act)
                    got = _skinny(x, wt, b if use_b else None, res if use_r else None, act)
                    worst = max(worst, _within(got, y64, e, f"{path} K={K} N={N} M={M} act={act} b={use_b} res={use_r}"))
                use_b, use_r = EPILOGUES[n % len(EPILOGUES)][1:]
                n += 1
                for act_i, bb, rr in ((R.ACT_NONE, bi if use_b else None, ri if use_r else None), (R.ACT_RELU, bi, ri)):
                    want, _ = R.linear_ref(xi, wi, bb, rr, act_i)
                    assert float(want.abs().max()) < 2 ** 24
                    assert torch.equal(_skinny(xi, wi, bb, rr, act_i), want.float()), f"{path} K={K} N={N} M={M} act={act_i}: not the integer result"
    finally:
        lib.ullsam_set_skinny_linear_mfma(old)
    print(f"{path} K={K}: worst err / bound {worst:.3f}")


def test_skinny_linear_contiguous_through_ops(ops):
    """the ops wrapper (ldx = K, ldr = ldy = N): skinny_linear_mfma_kernel<64, 4> at K = 256, N = 96, M = 65 and skinny_linear_kernel<32> at K = 384, N = 65, M = 33,
    GELU with b and res, against float64 within the derived bound; and the integer case in bits"""
    g = _gen(700)
    for K, N, M in ((256, 96, 65), (384, 65, 33)):
        x, wt, b, res = _randn((M, K), g), _randn((K, N), g, K ** -0.5), _randn((N,), g), _randn((M, N), g)
        y64, e = R.linear_ref(x, wt, b, res, R.ACT_GELU)
        _within(ops.skinny_linear(x, wt, b, ops.ACT_GELU, res), y64, e, f"ops.skinny_linear K={K} N={N} M={M}", quiet=False)
        xi, wi = torch.randint(-4, 5, (M, K), device=DEV, generator=g).float(), torch.randint(-4, 5, (K, N), device=DEV, generator=g).float()
        assert torch.equal(ops.skinny_linear(xi, wi, None), (xi.double() @ wi.double()).float())
