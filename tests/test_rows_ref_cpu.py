"""tests/rows_ref.py against independent statements of the same things (torch's own LayerNorm / GELU / float8_e4m3fn on the CPU, plain Python loops), the seeds of
the quantiser-with-LayerNorm cases, and -- without a GPU, since every check comes before the first HIP call -- what ullsam_norm, ullsam_norm_panels,
ullsam_rows_fp8, ullsam_skinny_linear and ullsam_small_linear refuse."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rows_ref as R

P = 1 << 20     # a 1 KiB aligned dummy address: never dereferenced, every check below comes before the first HIP call


@pytest.fixture(scope="module")
def lib():
    from ullsam_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_norm_ref_equals_torch_in_float64():
    g = torch.Generator(); g.manual_seed(0)
    x = torch.randn(9, 36, generator=g, dtype=torch.float64) * 3 + 1
    w, b = torch.randn(36, generator=g, dtype=torch.float64), torch.randn(36, generator=g, dtype=torch.float64)
    y, e = R.norm_ref(x, w, b, 1e-5)
    assert e is None and torch.allclose(y, F.layer_norm(x, (36,), w, b, 1e-5), rtol=0, atol=1e-13)
    y, _ = R.norm_ref(x, w, b, 1e-5, rms=True)                                       # b is ignored under rms
    assert torch.allclose(y, x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-5) * w, rtol=0, atol=1e-13)
    # the order: affine, then post, then act; post_scale and post_shift each on its own
    ln = F.layer_norm(x, (36,), w, b, 1e-5)
    y, _ = R.norm_ref(x, w, b, 1e-5, post_scale=torch.tensor(0.5), post_shift=torch.tensor(2.0), act=R.ACT_GELU)
    assert torch.allclose(y, F.gelu(ln * 0.5 + 2.0), rtol=0, atol=1e-13)
    y, _ = R.norm_ref(x, w, b, 1e-5, post_scale=torch.tensor(0.5))
    assert torch.allclose(y, ln * 0.5, rtol=0, atol=1e-13)
    y, _ = R.norm_ref(x, w, b, 1e-5, post_shift=torch.tensor(2.0))
    assert torch.allclose(y, ln + 2.0, rtol=0, atol=1e-13)
    # bf16 inputs are taken as stored
    xb = x.bfloat16()
    y, _ = R.norm_ref(xb, None, None, 1e-6)
    assert torch.allclose(y, F.layer_norm(xb.double(), (36,), None, None, 1e-6), rtol=0, atol=1e-13)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("kind", ["unit", "mean1000", "2^40", "2^-40"])
def test_norm_bound_holds_for_a_float32_numpy_norm_and_scales_with_the_data(kind, rms):
    """a float32 numpy norm (pairwise sums: a depth below any kernel's) stays inside the bound on every kind of row the GPU tests use, and the bound of a scaled
    row is the unit row's (relative to the output, which does not change), not an absolute number"""
    rng = np.random.default_rng(3)
    D = 1024
    x = rng.standard_normal((5, D), dtype=np.float32)
    x = {"unit": x, "mean1000": x + np.float32(1000.0), "2^40": x * np.float32(2.0 ** 40), "2^-40": x * np.float32(2.0 ** -40)}[kind]
    w = rng.standard_normal(D, dtype=np.float32)
    b = rng.standard_normal(D, dtype=np.float32)
    y, e = R.norm_ref(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 1e-6, rms=rms, depth=R.norm_depth("wave", D))
    if rms:
        got = x * (np.float32(1.0) / np.sqrt((x * x).sum(-1, dtype=np.float32) / np.float32(D) + np.float32(1e-6), dtype=np.float32))[:, None] * w[None]
    else:
        got = R.layer_norm_f32(x, w, b, 1e-6)
    err = np.abs(got.astype(np.float64) - y.numpy())
    assert (err <= e.numpy()).all(), float((err / e.numpy()).max())
    if kind == "mean1000" and not rms:      # the mean's error, 17 u 1000 = 1e-3 of a spread of 1, times |w| up to 3.5: far above the unit row's bound, as it must be
        assert 1e-3 < float(e.max()) < 5e-3
    else:
        assert float(e.max()) < 2e-5 * max(1.0, float(y.abs().max()))


def test_norm_depth_follows_the_dispatch():
    assert [R.norm_depth("wave", D) for D in (4, 256, 260, 1024, 1028, 2048, 2052, 4096)] == [9, 9, 12, 12, 16, 16, 24, 24]
    assert R.norm_depth("wave", 4100) == R.norm_depth("wave", 8192) == 40          # rows_fp8_kernel<., 32>
    assert R.norm_depth("narrow", 64) == 7 and R.norm_depth("block", 2048) == 13 and R.norm_depth("block", 2052) == R.norm_depth("block", 4096) == 15


def test_panel_index_is_a_bijection_onto_the_padded_buffer():
    for rows, D in ((5, 32), (67, 1280), (64, 2048)):
        pad = (rows + 15) // 16 * 16
        idx = R.panel_gather_index(pad, D)
        assert sorted(idx.reshape(-1).tolist()) == list(range(pad * D))
        assert int(idx[0, 0]) == 0 and int(idx[1, 0]) == 32 and int(idx[0, 31]) == 31
        if D > 32:
            assert int(idx[0, 32]) == 512                               # the next 32 k of the same 16 rows: the next 1 KiB cell
        if pad > 16:
            assert int(idx[16, 0]) == (D // 32) * 512
        assert R.panel_index(17, 40, 64) == ((1 * 2 + 1) * 512 + 1 * 32 + 8)


def test_linear_ref_equals_torch_in_float64():
    g = torch.Generator(); g.manual_seed(1)
    x, wt = torch.randn(7, 128, generator=g), torch.randn(128, 5, generator=g)
    b, r = torch.randn(5, generator=g), torch.randn(7, 5, generator=g)
    lin = F.linear(x.double(), wt.double().t(), b.double())
    for act, f in ((R.ACT_NONE, lambda t: t), (R.ACT_GELU, F.gelu), (R.ACT_RELU, F.relu)):
        y, e = R.linear_ref(x, wt, b, r, act)
        assert torch.allclose(y, f(lin) + r.double(), rtol=0, atol=1e-13)
        got = f(F.linear(x, wt.t().contiguous(), b)) + r                # torch's fp32 linear lies inside the bound
        assert bool(((got.double() - y).abs() <= e).all())
    y, _ = R.linear_ref(x, wt)
    assert torch.allclose(y, x.double() @ wt.double(), rtol=0, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# e4m3
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_e4m3_decoder_on_all_256_codes():
    codes = np.arange(256, dtype=np.uint8)
    ref = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    got = R.e4m3_decode(codes)
    nan = np.isnan(ref)
    assert nan.sum() == 2 and nan[0x7F] and nan[0xFF] and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))          # bits: -0.0 at 0x80 included
    assert got[0x7E] == 448.0 and got[0xFE] == -448.0 and got[0x08] == 2.0 ** -6 and got[0x01] == 2.0 ** -9


def _torch_cast(x):
    return torch.from_numpy(np.clip(x, np.float32(-448.0), np.float32(448.0))).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_e4m3_encoder_against_torch_on_every_midpoint_and_a_dense_sweep():
    vals = R.e4m3_decode(np.arange(0x7F, dtype=np.uint8)).astype(np.float32)               # the 127 finite magnitudes, ascending
    assert (np.diff(vals) > 0).all()
    mid = ((vals[:-1].astype(np.float64) + vals[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (vals[:-1].astype(np.float64) + vals[1:]) / 2)      # every midpoint is a float32
    pts = np.concatenate([vals, mid])
    pts = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))])
    rng = np.random.default_rng(0)
    dense = np.exp2(rng.uniform(-14, 9.2, 200000)).astype(np.float32)                         # below the smallest subnormal's half step up to beyond 448
    grid = (np.arange(0, 448 * 64 + 1, dtype=np.float32) / np.float32(64.0))
    pts = np.concatenate([pts, dense, grid, np.float32([0.0, 448.0, 449.0, 1000.0, 3e38, 1e-40, 2.0 ** -10, 17.0, 19.0, 1.5 * 2.0 ** -9])])
    pts = np.concatenate([pts, -pts]).astype(np.float32)
    got = R.e4m3_encode(pts)
    assert np.array_equal(got, _torch_cast(pts)), pts[got != _torch_cast(pts)][:10]
    # the tie rule and the saturation by name, and the encoder saturating on its own
    enc = lambda v: int(R.e4m3_encode(np.float32([v]))[0])
    assert R.e4m3_decode([enc(17.0)])[0] == 16.0 and R.e4m3_decode([enc(19.0)])[0] == 20.0
    assert enc(2.0 ** -10) == 0 and enc(-(2.0 ** -10)) == 0x80 and enc(-0.0) == 0x80 and enc(1.5 * 2.0 ** -9) == 2 and enc(2.0 ** -6) == 8
    assert enc(448.0) == enc(1e9) == enc(float("inf")) == 0x7E and enc(-448.0) == enc(-1e9) == 0xFE and enc(float("nan")) == 0x7F
    # decode(encode) is the identity on the codes
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
    assert np.array_equal(R.e4m3_encode(R.e4m3_decode(codes)), codes)


def test_e4m3_half_spacing():
    assert R.e4m3_half_spacing(0.0) == R.e4m3_half_spacing(7 * 2.0 ** -9) == 2.0 ** -10
    assert R.e4m3_half_spacing(2.0 ** -6) == 2.0 ** -10 and R.e4m3_half_spacing(16.0) == R.e4m3_half_spacing(-30.0) == 1.0 and R.e4m3_half_spacing(448.0) == 16.0


def test_quantiser_restatement_on_rows_whose_scale_is_a_power_of_two():
    """amax = 448 2^k gives sc = 2^k exactly (fl(448 fl(1 / 448)) = 1), so the codes are the e4m3 codes of x / 2^k: the ties and the subnormals by hand"""
    for k in (-3, 0, 5):
        s = 2.0 ** k
        x = np.float32([[448 * s, -448 * s, 17 * s, 19 * s, -17 * s, 2.0 ** -10 * s, 1.5 * 2.0 ** -9 * s, 2.0 ** -6 * s, 0.0, -0.0, 3.0 * s, 100.0 * s]])
        q, sc = R.quantise_rows_f32(x)
        assert sc[0] == np.float32(s)
        assert q[0].tolist() == [0x7E, 0xFE, R.e4m3_encode(np.float32([16.0]))[0], R.e4m3_encode(np.float32([20.0]))[0],
                                 R.e4m3_encode(np.float32([-16.0]))[0], 0, 2, 8, 0, 0x80, R.e4m3_encode(np.float32([3.0]))[0], R.e4m3_encode(np.float32([96.0]))[0]]             # 100 is a tie too: 96 has the even mantissa
    q, sc = R.quantise_rows_f32(np.zeros((2, 8), np.float32))
    assert (sc == 1).all() and (q == 0).all()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D", [256, 1280, 5120])
def test_seeds_of_the_layernorm_quantiser_cases(D, bf16):
    """the GPU test allows 0.5 % of a case's codes to differ from enc(y64 / sc64); with these seeds a float32 numpy LayerNorm in the kernel's place stays under a
    tenth of that, and inside the scale and the elementwise bounds the GPU test applies"""
    x, w, b = R.fp8_ln_case(D, bf16)
    y64, e, sc64, q64 = R.fp8_ln_ref(x, w, b)
    q, sc = R.quantise_rows_f32(R.layer_norm_f32(x, w, b, R.FP8_LN_EPS))
    frac = float((q != q64).mean())
    print(f"D={D} bf16={bf16}: {frac * 100:.4f} % of the codes differ")
    assert frac <= 0.0005
    assert (np.abs(sc.astype(np.float64) - sc64) <= e.max(-1) / 448.0 + 2.0 ** -23 * sc).all()
    dec = R.e4m3_decode(q).astype(np.float64)
    assert (np.abs(dec * sc[:, None] - y64) <= R.e4m3_half_spacing(dec) * sc[:, None] + e).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals (the entry returns before any launch)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, text):
    assert rc != 0
    msg = lib.ullsam_last_error_string().decode()
    assert text in msg, msg


def test_rows_fp8_refusals(lib):
    f = lambda **kw: lib.ullsam_rows_fp8(*[kw.get(k, d) for k, d in (("inp", P), ("dt", 0), ("ins", 64), ("out", P), ("outs", 64), ("sc", P), ("w", None), ("b", None),
                                                                       ("rows", 8), ("D", 64), ("eps", 0.0), ("stream", None))])
    _refused(lib, f(dt=2), "bad dtype")
    for D in (0, -4, 6, 8196):
        _refused(lib, f(D=D, ins=8200, outs=8200), "positive multiple of 4")
    _refused(lib, f(w=P), "weight and bias go together")
    _refused(lib, f(w=P + 4, b=P), "16-byte aligned")
    _refused(lib, f(ins=60), "input rows must be aligned")              # in_stride < D
    _refused(lib, f(ins=66), "input rows must be aligned")              # in_stride % 4
    _refused(lib, f(inp=P + 8), "input rows must be aligned")           # fp32 needs 16 bytes
    _refused(lib, f(inp=P + 4, dt=1), "input rows must be aligned")     # bf16 needs 8
    _refused(lib, f(outs=60), "output rows must be 4-byte aligned")     # out_stride < D
    _refused(lib, f(outs=66), "output rows must be 4-byte aligned")
    _refused(lib, f(out=P + 2), "output rows must be 4-byte aligned")
    for kw in (dict(inp=None), dict(out=None), dict(sc=None)):
        _refused(lib, f(**kw), "null argument")
    assert f(rows=0, inp=None, out=None, sc=None) == 0                  # nothing to do
    assert f(rows=0, inp=P + 8, dt=1) == 0


def test_norm_refusals(lib):
    f = lambda **kw: lib.ullsam_norm(*[kw.get(k, d) for k, d in (("inp", P), ("idt", 0), ("ins", 64), ("out", P), ("odt", 0), ("outs", 64), ("w", None), ("b", None),
                                                                   ("rows", 8), ("D", 64), ("eps", 1e-6), ("rms", 0), ("act", 0), ("ps", None), ("pb", None), ("stream", None))])
    g = lambda **kw: lib.ullsam_norm_panels(*[kw.get(k, d) for k, d in (("inp", P), ("idt", 0), ("ins", 64), ("out", P), ("w", None), ("b", None), ("rows", 8), ("D", 64),
                                                                          ("eps", 1e-6), ("rms", 0), ("act", 0), ("ps", None), ("pb", None), ("panels", 1), ("stream", None))])
    for fn, name in ((f, "ullsam_norm:"), (g, "ullsam_norm_panels:")):
        _refused(lib, fn(inp=None), name + " null argument")
        _refused(lib, fn(out=None), name + " null argument")
        _refused(lib, fn(ins=60), "must be >= D=64")
        _refused(lib, fn(inp=P + 8), "must be aligned to 4 elements")               # fp32 input: 16 bytes
        _refused(lib, fn(inp=P + 4, idt=1), "must be aligned to 4 elements")        # bf16 input: 8 bytes
        _refused(lib, fn(w=P + 8), "weight and bias must be 16-byte aligned")
        _refused(lib, fn(b=P + 4), "weight and bias must be 16-byte aligned")
        _refused(lib, fn(idt=3), "bad")
        assert fn(rows=0, inp=None, out=None) == 0
    _refused(lib, f(outs=60), "must be >= D=64")
    _refused(lib, f(out=P + 8), "must be aligned to 4 elements")
    _refused(lib, f(out=P + 4, odt=1), "must be aligned to 4 elements")
    _refused(lib, f(odt=2), "bad dtypes")
    _refused(lib, g(out=P + 4, panels=0), "must be aligned to 4 elements")            # (row-major through the panels entry: a bf16 output needs 8 bytes)
    _refused(lib, f(ins=66), "multiples of 4")                                       # what was refused before still is


def test_skinny_and_small_linear_refusals(lib):
    f = lambda **kw: lib.ullsam_skinny_linear(*[kw.get(k, d) for k, d in (("x", P), ("ldx", 128), ("wt", P), ("b", None), ("res", None), ("ldr", 0), ("y", P), ("ldy", 32),
                                                                            ("M", 8), ("N", 32), ("K", 128), ("act", 0), ("stream", None))])
    _refused(lib, f(K=0, ldx=0), "K=0 must be positive")
    _refused(lib, f(K=-128), "must be positive")
    _refused(lib, f(M=-1, N=-32), "must not be negative")
    _refused(lib, f(ldy=31), "must be >= N=32")
    _refused(lib, f(res=P, ldr=31), "must be >= N=32")
    _refused(lib, f(K=100), "K % 128")                                               # what was refused before still is
    _refused(lib, f(x=P + 8), "16-byte aligned x")
    assert f(M=0) == 0 and f(M=0, ldr=0, res=None, ldy=32) == 0
    s = lambda **kw: lib.ullsam_small_linear(*[kw.get(k, d) for k, d in (("x", P), ("ldx", 16), ("w", P), ("b", None), ("res", None), ("ldr", 0), ("y", P), ("ldy", 4),
                                                                           ("M", 2), ("N", 4), ("K", 16), ("act", 0), ("stream", None))])
    _refused(lib, s(x=P + 8), "x and W must be 16-byte aligned")
    _refused(lib, s(w=P + 4), "x and W must be 16-byte aligned")
    _refused(lib, s(K=18), "multiples of 4")
    assert s(M=0) == 0
