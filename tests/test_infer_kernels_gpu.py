"""The inference kernels around the GEMM / ViT / causal / token-to-image attention / fused decoder kernels (those have their own tests in
test_kernels_gpu.py; the fused decoder kernels in test_decoder_kernels_gpu.py), one by one, against float64 definitions of the reference's operations written here, at the shapes, dtypes, strides and
edges where their code paths divide: LLM data movement (csrc/llm_misc.hip), ViT / projector data movement (csrc/vit_misc.hip, csrc/norm.hip),
the prompt encoder's and mask decoder's small kernels (csrc/decoder.hip, csrc/dectok.hip, csrc/amg.hip) and the edges of the small attention
kernels (csrc/attention.hip: naive, few-keys, decode).

Pure moves, casts and integer kernels must match exactly.  Outputs with a stride or a limited write region are filled with a sentinel first and
nothing outside the region may change.  Every tolerance is (a) a derived bound written out at its test, (b) the bound of the existing test of the
same kind of kernel (test_kernels_gpu.py: 1e-5 fp32 linears / attention / resize, 2e-5 fp32 LayerNorm chains, 2e-2 decode attention), or (c) a
margin over a value measured against the float64 reference and recorded in the docstring.  "One bf16 step" is 2^-8 relative (the worst case of
one round-to-nearest-even of the float64 value), added to the fp32 bound of the same result (the kernels compute in fp32 and round once).

Contract of the image-token scan for a sample WITHOUT an image token (modeling_internvl_sam.py:194-203 raises "Can not find vision token!"): the
kernel reports an EMPTY range, range[1] <= range[0] (it writes [S, 0]) and rank -1 everywhere; InternVLSAMModel._forward_inference raises the
reference's ValueError on exactly that condition.  ullsam_gather_rows, which is stream-ordered and runs before the host has looked, clamps every
source row into [0, S): with the empty range it reads row S - 1 only -- in bounds, finite, discarded by the raise."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ullsam_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMIN = float(torch.finfo(torch.float32).min)
DTYPES = [torch.float32, torch.bfloat16]
U24, U23, BF16_STEP = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8


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


def _gen(seed, device=DEV):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def _randn(shape, g, scale=1.0, dtype=torch.float32):
    return (torch.randn(shape, device=g.device, generator=g, dtype=torch.float32) * scale).to(dtype)


def _within(got, ref64, bound, what):
    """|got - ref| <= bound elementwise (bound: scalar or tensor), everything finite; prints the worst error and the worst share of its bound."""
    got64 = got.double()
    assert got64.shape == ref64.shape, (what, got64.shape, ref64.shape)
    assert bool(torch.isfinite(got64).all()), f"{what}: non-finite values"
    e = (got64 - ref64).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(e, float(bound))
    ratio = float((e / b.clamp(min=1e-300)).max()) if e.numel() else 0.0
    print(f"{what}: max |err| {float(e.max()) if e.numel() else 0.0:.3e}, worst err / bound {ratio:.3f}")
    assert bool((e <= b).all()), f"{what}: max |err| {float(e.max()):.3e}, worst err / bound {ratio:.3f}"
    return ratio


def _bf16_bound(ref64, f32_bound):
    """one bf16 rounding (2^-8 relative, worst case) of an fp32 result that is itself within f32_bound of the float64 value"""
    return ref64.abs() * BF16_STEP + f32_bound


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. LLM data movement (csrc/llm_misc.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
IMG = 7          # the image-token id of these tests; every other id is drawn from [8, 1000)


def image_token_layouts(S):
    """ids int64 [3, S] (CPU), one layout per sample: 0 = image tokens at positions 0 and S - 1 (and, for S = 200, a run over the 128 boundary:
    three runs, range = [first, last + 1)); 1 = a run that crosses the 64-token boundary where S allows (the rank carries across trips of the
    64-lane scan) and a second, separate run for S = 200; 2 = no image token at all."""
    g = torch.Generator(); g.manual_seed(S)
    ids = torch.randint(8, 1000, (3, S), generator=g, dtype=torch.int64)
    ids[0, 0] = IMG; ids[0, S - 1] = IMG
    if S == 200:
        ids[0, 100:141] = IMG
    lo, hi = (60, min(S, 71)) if S >= 65 else (S // 3, max(S // 3 + 1, 2 * S // 3))
    ids[1, lo:hi] = IMG
    if S == 200:
        ids[1, 150:160] = IMG
    return ids


def scan_reference(ids):
    """numpy: rank = (cumulative count of image tokens) - 1 at image tokens, -1 elsewhere; range = [first, last + 1) or None without one"""
    a = ids.numpy() == IMG
    rank = np.where(a, np.cumsum(a, -1) - 1, -1).astype(np.int32)
    rng = [(int(np.nonzero(r)[0][0]), int(np.nonzero(r)[0][-1]) + 1) if r.any() else None for r in a]
    return rank, rng


@pytest.mark.parametrize("S", [1, 63, 64, 65, 200])
def test_scan_image_tokens_against_cumsum(ops, S):
    """ullsam_scan_image_tokens: ranks and [first, last + 1) ranges, exact; the sample without an image token reports an empty range
    (range[1] <= range[0], the condition the Python caller raises on -- see the header) and rank -1 everywhere."""
    ids = image_token_layouts(S)
    rank_ref, rng_ref = scan_reference(ids)
    rank, rng = ops.scan_image_tokens(ids.to(DEV), IMG)
    rank, rng = rank.cpu().numpy(), rng.cpu().numpy()
    assert np.array_equal(rank, rank_ref)
    for b in range(3):
        if rng_ref[b] is None:
            assert rng[b, 1] <= rng[b, 0], rng[b]
            assert (rank[b] == -1).all()
        else:
            assert tuple(rng[b]) == rng_ref[b], (b, rng[b], rng_ref[b])
    assert rng_ref[2] is None and rng_ref[0] == (0, S)
    if S >= 65:
        assert rng_ref[1][0] < 64 < rng_ref[1][1]          # the run crosses the boundary of the first trip


def _embed_case(B, S, D, vocab, n_img, dtype, seed):
    g = _gen(seed)
    table = _randn((vocab, D), g, dtype=dtype)
    ids = torch.randint(0, vocab, (B, S), device=DEV, generator=g, dtype=torch.int64)
    ids[ids == IMG] = IMG + 1
    ids[0, 1:1 + min(S - 1, 2 * n_img + 2)] = IMG                # more image tokens than n_img: the `rank % n_img` repeat branch (:142-145)
    ids[-1, S // 2:S // 2 + 3] = IMG
    ids[0, 0] = -3; ids[-1, S - 1] = vocab + 5; ids[-1, S - 2] = vocab          # clamp to row 0 / row vocab - 1, as the kernel documents
    vit = _randn((B, n_img, D), g)
    return table, ids, vit


def _embed_reference(table, ids, rank, vit):
    B, S = ids.shape
    ref = table.float()[ids.clamp(0, table.shape[0] - 1).reshape(-1)]
    if rank is not None and vit is not None:
        n_img = vit.shape[1]
        r = rank.reshape(-1).long()
        b = torch.arange(B, device=ids.device).repeat_interleave(S)
        ref = torch.where((r >= 0)[:, None], vit[b, r.clamp(min=0) % n_img], ref)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [4, 260, 4096])
def test_embed_tokens_gather_and_image_splice(ops, dtype, D):
    """ullsam_embed_tokens: table rows (fp32 / bf16 tables widened exactly) with the ViT rows spliced in at image tokens; rank None, rank given
    with vit None (both: the plain gather), more image tokens than n_img, ids < 0 and >= vocab.  Exact."""
    B, S, vocab, n_img = 2, 37, 50, 5
    table, ids, vit = _embed_case(B, S, D, vocab, n_img, dtype, D)
    rank, _ = ops.scan_image_tokens(ids, IMG)
    assert int(rank[0].max()) >= n_img                              # the repeat branch is taken
    plain = _embed_reference(table, ids, None, None)
    assert torch.equal(ops.embed_tokens(table, ids, None, None), plain)
    assert torch.equal(ops.embed_tokens(table, ids, rank, None), plain)
    got = ops.embed_tokens(table, ids, rank, vit.reshape(B * n_img, D))
    ref = _embed_reference(table, ids, rank, vit)
    assert torch.equal(got, ref) and not torch.equal(ref, plain)


def test_embed_tokens_grid_stride_wrap(ops):
    """4200 rows of D = 4096 are 4 300 800 quads, more than the launch's 2048 * 8 * 256 = 4 194 304 threads: the last rows come from the second
    trip of the grid-stride loop.  Exact."""
    B, S, D, vocab, n_img = 2, 2100, 4096, 64, 3
    table, ids, vit = _embed_case(B, S, D, vocab, n_img, torch.bfloat16, 1)
    assert B * S * (D // 4) > 2048 * 8 * 256
    rank, _ = ops.scan_image_tokens(ids, IMG)
    got = ops.embed_tokens(table, ids, rank, vit.reshape(B * n_img, D))
    assert torch.equal(got, _embed_reference(table, ids, rank, vit))


@pytest.mark.parametrize("dtype,D", [(torch.float32, 4), (torch.bfloat16, 8), (torch.float32, 260), (torch.bfloat16, 264)])
def test_gather_rows_with_clamped_and_empty_ranges(ops, dtype, D):
    """ullsam_gather_rows: rows [range[0], range[0] + n) of each sample, 16-byte rows included; a range that runs past the sample
    (range[0] + n > S) repeats row S - 1, and the empty range of a sample without image token ([S, 0], produced here by the scan kernel itself)
    reads row S - 1 only.  Exact."""
    B, S, n = 3, 20, 6
    ids = torch.randint(8, 1000, (B, S), generator=_gen(D, "cpu"), dtype=torch.int64)
    ids[0, 2:8] = IMG; ids[1, 17:20] = IMG
    _, rng = ops.scan_image_tokens(ids.to(DEV), IMG)
    r = rng.cpu().numpy()
    assert tuple(r[0]) == (2, 8) and tuple(r[1]) == (17, 20) and r[2, 1] <= r[2, 0]
    x = _randn((B * S, D), _gen(D), dtype=dtype)
    got = ops.gather_rows(x, rng, B, S, n)
    src = (torch.from_numpy(r[:, :1].astype(np.int64)) + torch.arange(n)[None]).clamp(0, S - 1) + S * torch.arange(B)[:, None]
    assert torch.equal(got, x[src.reshape(-1).to(DEV)])
    assert int(src[1].max()) == 2 * S - 1 and bool((src[2] == 3 * S - 1).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("G", [1, 4])
def test_rope_split_positions_cache_offset_and_clamping(ops, dtype, hd, G):
    """ullsam_rope_split with cache_pos0 > 0 and cap > cache_pos0 + S, per-sample position ids (a left-padded sample's differ from 0 .. S - 1),
    positions < 0 and >= tab_rows (clamped: the reference row is the clamped one), cos / sin tables WITHOUT the cat(freqs, freqs) symmetry (the two
    halves of a table row are read separately).  q, the appended K rows against q cos + rotate_half(q) sin in float64; V rows exact; cache rows
    outside [pos0, pos0 + S) keep their sentinel.
    fp32 bound, derived: each output is two products and one sum, |err| <= 3 * 2^-24 (|x1 c| + |x2 s|) elementwise; bf16: one bf16 step on top."""
    B, S, KVH, cap, pos0, tab = 2, 5, 2, 12, 3, 16
    g = _gen(hd + G)
    qkv = _randn((B * S, KVH * (G + 2) * hd), g, dtype=dtype)
    cos, sin = torch.rand((tab, hd), device=DEV, generator=g) * 2 - 1, torch.rand((tab, hd), device=DEV, generator=g) * 2 - 1
    pos = torch.tensor([[-2, -1, 0, 1, 2], [13, 14, 15, 16, 40]], dtype=torch.int32, device=DEV)
    kc = torch.full((B, KVH, cap, hd), 7.0, dtype=dtype, device=DEV)
    vc = torch.full((B, KVH, cap, hd), -3.0, dtype=dtype, device=DEV)
    q = ops.rope_split(qkv, kc, vc, pos, cos, sin, B, S, KVH, G, hd, pos0)
    x = qkv.double().reshape(B, S, KVH, G + 2, hd)
    pc = pos.long().clamp(0, tab - 1)
    c, s_ = cos.double()[pc][:, :, None, None, :], sin.double()[pc][:, :, None, None, :]
    rot = torch.cat([-x[..., hd // 2:], x[..., :hd // 2]], -1)                       # rotate_half (modeling_internlm2.py:233-237)
    ref = x * c + rot * s_
    f32b = 3 * U24 * ((x * c).abs() + (rot * s_).abs())
    bound = f32b if dtype == torch.float32 else _bf16_bound(ref, f32b)
    _within(q.reshape(B, S, KVH, G, hd), ref[..., :G, :], bound[..., :G, :], "rope_split q")
    _within(kc[:, :, pos0:pos0 + S].permute(0, 2, 1, 3), ref[..., G, :], bound[..., G, :], "rope_split k rows")
    assert torch.equal(vc[:, :, pos0:pos0 + S].permute(0, 2, 1, 3), qkv.reshape(B, S, KVH, G + 2, hd)[..., G + 1, :])
    keep = torch.ones(cap, dtype=torch.bool, device=DEV); keep[pos0:pos0 + S] = False
    assert bool((kc[:, :, keep] == 7.0).all()) and bool((vc[:, :, keep] == -3.0).all())


ARGMAX_V = [1, 1023, 1024, 1025, 4096, 4097, 92553]


def argmax_rows(V):
    """fp32 rows [R, V] (CPU) and the indices of the rows that hold NaN.  Rows: random; maximum at 0; maximum at V - 1; ties (value 50, above
    everything else) in neighbouring lanes (i, i + 1), in different waves (i, i + 64), in different unroll slots (i, i + 1024), in different trips
    (i, i + 4096), in different trips with the LATER index in the LOWER thread (5, 4096 + 3); all equal; all -inf; NaN among ordinary values;
    all NaN.  A tie whose second member does not fit into V leaves its row random."""
    g = torch.Generator(); g.manual_seed(V)
    names = ["random", "max0", "maxlast", "tie1", "tie64", "tie1024", "tie4096", "tie_cross", "equal", "neginf", "nan_some", "nan_all"]
    x = torch.randn((len(names), V), generator=g)
    x[1, 0] = 50.0
    x[2, V - 1] = 50.0
    t1024 = (0, 1024) if V <= 1027 else (3, 3 + 1024)            # (the smallest V that holds such a pair has it at index 0)
    t4096 = (0, 4096) if V <= 4105 else (9, 9 + 4096)
    for row, (i, j) in ((3, (10, 11)), (4, (17, 17 + 64)), (5, t1024), (6, t4096), (7, (5, 4096 + 3))):
        if j < V:
            x[row, i] = x[row, j] = 50.0
    x[8] = 1.25
    x[9] = float("-inf")
    x[10, ::3] = float("nan")
    x[11] = float("nan")
    return x, [10, 11]


@pytest.mark.parametrize("V", ARGMAX_V)
def test_argmax_ties_edges_and_padded_rows(ops, V):
    """ullsam_argmax against torch.argmax on the CPU copy (first maximum wins) for every NaN-free row, ties placed in every pair of places the
    kernel treats differently (argmax_rows), a row of nothing but -inf (index 0), through the wrapper (ld = V) and directly with ld > V and LARGER
    values in the pad columns.  Every result, the two NaN rows' included (only the range is asserted for those: 2 of 12 rows), lies in [0, V)."""
    x, nan_rows = argmax_rows(V)
    R = x.shape[0]
    clean = [r for r in range(R) if r not in nan_rows]
    assert len(nan_rows) == 2 and not bool(torch.isnan(x[clean]).any())
    want = torch.argmax(x, -1)
    got = ops.argmax(x.to(DEV)).cpu()
    ld = V + 5
    buf = torch.full((R, ld), 1e9)
    buf[:, :V] = x
    out = torch.full((R + 1,), -77, dtype=torch.int64, device=DEV)
    bd = buf.to(DEV)
    _lib().call("ullsam_argmax", bd.data_ptr(), out.data_ptr(), R, V, ld, _s())
    out = out.cpu()
    assert int(out[R]) == -77
    for res in (got, out[:R]):
        assert bool(((res >= 0) & (res < V)).all()), res.tolist()
        assert res[clean].tolist() == want[clean].tolist()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. ViT and projector data movement (csrc/vit_misc.hip, csrc/norm.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("Hs,Ws", [(37, 45), (64, 64)])
def test_patch_im2col_normalise_then_pad(ops, dtype, norm, Hs, Ws):
    """ullsam_patch_im2col: (x - mean) / std per channel, THEN zero padding to S x S (sam.py:164-174), then the patch rows of PatchEmbed
    (image_encoder.py:391-395); 37 x 45 in 64 x 64 at patch 16 puts the image edge inside a patch and inside a quad of four pixels.
    fp32 bound: the subtraction and the division are rounded once each: 2 ulp of the value (exact without mean / std); bf16: one step on top."""
    B, C, S, p = 2, 3, 64, 16
    g = _gen(Hs + 2 * norm)
    x = torch.rand((B, C, Hs, Ws), device=DEV, generator=g) * 255
    mean = torch.tensor([123.675, 116.28, 103.53], device=DEV) if norm else None
    std = torch.tensor([58.395, 57.12, 57.375], device=DEV) if norm else None
    got = ops.patch_im2col(x, S, p, dtype, mean, std)
    v = x.double()
    if norm:
        v = (v - mean.double()[None, :, None, None]) / std.double()[None, :, None, None]
    v = F.pad(v, (0, S - Ws, 0, S - Hs))
    gq = S // p
    ref = v.reshape(B, C, gq, p, gq, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gq * gq, C * p * p)
    ulp = torch.from_numpy(np.spacing(np.abs(ref.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(DEV)
    f32b = 2 * ulp if norm else torch.zeros_like(ref)
    _within(got, ref, f32b if dtype == torch.float32 else _bf16_bound(ref, f32b), "patch_im2col")
    if Hs < S:      # (the bound at a reference of 0 is 0: the padding must be exactly zero, not (0 - mean) / std)
        assert bool((got.reshape(B, gq, gq, C, p, p)[:, gq - 1, :, :, (Hs - (gq - 1) * p):, :] == 0).all())


@pytest.mark.parametrize("dtype,C", [(torch.float32, 4), (torch.bfloat16, 8), (torch.float32, 12)])
def test_im2col3x3_non_square(ops, dtype, C):
    """ullsam_im2col3x3 (image_encoder.py:96-102 as im2col): 5 x 9 pixels, three images, the smallest pixel (16 bytes) and one of three chunks. Exact."""
    B, H, W = 3, 5, 9
    x = _randn((B, H, W, C), _gen(C), dtype=dtype)
    got = ops.im2col3x3(x, B, H, W, C)
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1)).to(dtype)
    ref = torch.cat([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], -1).reshape(B * H * W, 9 * C)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("R,C", [(33, 31), (1, 70), (70, 1)])
def test_transpose_f32_ragged_tiles(ops, R, C):
    """ullsam_transpose_f32: [3, R, C] -> [3, C, R] with R, C just past / far below the 32 x 32 tile. Exact."""
    x = _randn((3, R, C), _gen(R))
    assert torch.equal(ops.transpose(x, 3, R, C), x.transpose(1, 2).contiguous())


def test_pixel_unshuffle_non_square(ops):
    """ullsam_pixel_unshuffle (text_aware_dense_feature, modeling_internvl_sam.py:256-268) is the inverse of pixel_shuffle v2 (:226-240, the oracle's
    port): tokens made by shuffling an NHWC image must come back as that image -- 4 x 6 pixels (the reference itself only forms square grids),
    three images, the smallest C (one 16-byte chunk).  Exact."""
    B, H, W, C = 3, 4, 6, 4
    img = np.random.default_rng(0).standard_normal((B, H, W, C), dtype=np.float32)
    tok = O.pixel_shuffle_v2(img).reshape(B, (H // 2) * (W // 2), 4 * C)
    got = ops.pixel_unshuffle(torch.from_numpy(tok).to(DEV), B, H, W, C)
    assert torch.equal(got.reshape(B, H, W, C).cpu(), torch.from_numpy(img))


@pytest.mark.parametrize("a_dt", DTYPES)
@pytest.mark.parametrize("o_dt", DTYPES)
@pytest.mark.parametrize("cols", [4, 260])
def test_add_cast_broadcast_rows_and_pure_cast(ops, a_dt, o_dt, cols):
    """ullsam_add_cast: out[r] = a[r % a_rows] (+ b[r % b_rows]) for the four dtype pairs, a_rows < rows, b_rows < rows, b None: equal to torch's
    fp32 sum followed by ONE round-to-nearest-even conversion.  Exact."""
    rows = 7
    g = _gen(cols)
    for a_rows, b_rows in ((3, 7), (7, 2), (7, 0)):
        a = _randn((a_rows, cols), g, dtype=a_dt)
        b = _randn((b_rows, cols), g) if b_rows else None
        got = ops.add_cast(a, b, o_dt, rows=rows)
        r = torch.arange(rows, device=DEV)
        ref = a.float()[r % a_rows]
        if b is not None:
            ref = ref + b[r % b_rows]
        assert got.dtype == o_dt and torch.equal(got, ref.to(o_dt)), (a_rows, b_rows)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pixel_shuffle_ln_non_square_and_large_mean(ops, dtype):
    """ullsam_pixel_shuffle_ln: pixel_shuffle v2 + LayerNorm(4C) on 4 x 6 pixels, three images, in float64.  Half of the tokens have mean 100 and
    spread 0.011: their values lie on the grid 100 + k / 128, |k| <= 2, on which every fp32 partial sum of 1024 values is exact, so the two-pass
    variance the kernel uses is as accurate as on ordinary rows, while a one-pass E[x^2] - E[x]^2 (x^2 = 10^4 with fp32 steps of 10^-3 against a
    variance of 1.2 x 10^-4) is not.  (Off such a grid the fp32 rounding of the MEAN alone costs 4e-4 in any fp32 LayerNorm, torch's included.)
    fp32: the 2e-5 bound of the existing check (test_data_movement_kernels); bf16: one bf16 step on top."""
    B, H, W, C = 3, 4, 6, 256
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    x[:, :2] = (100.0 + rng.integers(-2, 3, size=(B, 2, W, C)) / 128.0).astype(np.float32)
    w = rng.standard_normal(4 * C).astype(np.float32); b = rng.standard_normal(4 * C).astype(np.float32)
    got = ops.pixel_shuffle_ln(torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV), B, H, W, C, 1e-5, dtype)
    t = torch.from_numpy(O.pixel_shuffle_v2(x).reshape(B * (H // 2) * (W // 2), 4 * C)).double().to(DEV)
    assert float(t[0].mean()) > 99 and float(t[0].std()) < 0.02
    ref = F.layer_norm(t, (4 * C,), torch.from_numpy(w).double().to(DEV), torch.from_numpy(b).double().to(DEV), 1e-5)
    _within(got, ref, 2e-5 if dtype == torch.float32 else _bf16_bound(ref, 2e-5), "pixel_shuffle_ln")


@pytest.mark.parametrize("cdt", DTYPES)
@pytest.mark.parametrize("D", [4, 64, 256])
def test_norm_fanout_every_output_combination(ops, cdt, D):
    """ullsam_norm_fanout: y = LayerNorm(x) as fp32, as the compute dtype and as (y + pe[row % pe_rows]) in the compute dtype, every combination
    the wrapper allows, pe_rows < rows.  pe is chosen close to -y, so that |y + pe| << |y|: the third output must be the rounding of the fp32
    (y + pe) -- held to one bf16 step of |y + pe| -- where round(y) + pe would be off by a bf16 step of |y|, two orders more.  fp32 results: the
    2e-5 bound of the fp32 LayerNorm checks (test_norms)."""
    pe_rows, rows, eps = 5, 10, 1e-6
    g = _gen(D)
    x = _randn((pe_rows, D), g, 2.0).repeat(2, 1).contiguous() + 0.3
    w, b = _randn((D,), g), _randn((D,), g)
    y = F.layer_norm(x.double(), (D,), w.double(), b.double(), eps)
    pe = (-y[:pe_rows] + 0.01 * _randn((pe_rows, D), g).double()).float().contiguous()
    ype = y + pe.double().repeat(2, 1)
    assert float(ype.abs().max()) < 0.1 * float(y.abs().max())
    bf = cdt == torch.bfloat16
    for want_f32 in (False, True):
        for want_c in (False, True):
            for use_pe in (False, True):
                of, oc, ope = ops.norm_fanout(x, w, b, eps, cdt, pe if use_pe else None, want_f32=want_f32, want_c=want_c)
                what = f"norm_fanout f32={want_f32} c={want_c} pe={use_pe}"
                assert (of is not None) == (want_f32 or (want_c and not bf)) and (oc is not None or not want_c) and (ope is not None) == use_pe
                if of is not None:
                    _within(of, y, 2e-5, what + " fp32")
                if want_c:
                    assert oc.dtype == cdt
                    _within(oc, y, _bf16_bound(y, 2e-5) if bf else 2e-5, what + " compute dtype")
                if ope is not None:
                    assert ope.dtype == cdt
                    _within(ope, ype, _bf16_bound(ype, 2e-5) if bf else 2e-5, what + " y + pe")
                    if of is not None:      # ... and exactly: the fp32 sum of the fp32 y, rounded once
                        assert torch.equal(ope, (of + pe.repeat(2, 1)).to(cdt))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. prompt encoder and mask decoder small kernels (csrc/decoder.hip, csrc/dectok.hip, csrc/amg.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
PE_C = 4.0     # see test_sparse_embed_against_float64_sin_cos


def _pe_check(got, ang64, add64, what):
    """sin | cos of the float64 angle (+ the added embedding row).  The error of sin / cos of an fp32-rounded angle is governed by the angle's own
    rounding: |err| <= PE_C * 2^-23 * max(1, max |angle| of the case) + one ulp (2^-23 relative) of the sum with the embedding."""
    ref = torch.cat([torch.sin(ang64), torch.cos(ang64)], -1) + add64
    amax = max(1.0, float(ang64.abs().max()))
    e = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all())
    ulp_sum = U23 * ref.abs()
    c = float(((e - ulp_sum).clamp(min=0) / (U23 * amax)).max())
    print(f"{what}: max |err| {float(e.max()):.3e}, max |angle| {amax:.2f}, measured c = {c:.3f} (bound {PE_C})")
    assert bool((e <= PE_C * U23 * amax + ulp_sum).all()), (what, c)
    return c


@pytest.mark.parametrize("C", [8, 256, 512])
def test_sparse_embed_against_float64_sin_cos(ops, C):
    """ullsam_sparse_embed (prompt_encoder.py:76-103, 220-250): points only / points + pad point / boxes only (no coords) / points + boxes, labels
    -1 / 0 / 1 and both box corners, img_w != img_h, coordinates at 0 and at size - 1, C / 2 below, at and above the 128 threads.  A label -1 row
    (a given one and the pad point) equals the not_a_point row exactly.  Bound: _pe_check; c measured on an MI355X over these cases and the
    dense_pe cases: worst 1.09 (angles up to 29; dense_pe alone 0.88), asserted at PE_C = 4 = twice that, rounded up to a power of two."""
    P, Np, img_w, img_h = 2, 3, 64.0, 48.0
    g = _gen(C)
    G = _randn((2, C // 2), g)
    emb = _randn((5, C), g)
    coords = torch.tensor([[[0.0, 0.0], [63.0, 47.0], [20.25, 31.5]], [[63.0, 0.0], [0.0, 47.0], [11.0, 5.75]]], device=DEV)
    labels = torch.tensor([[1, 0, -1], [-1, 1, 0]], dtype=torch.int32, device=DEV)
    boxes = torch.tensor([[0.0, 0.0, 63.0, 47.0], [5.5, 7.25, 40.0, 30.0]], device=DEV)

    def reference(pts, lab):                                       # pts [P, n, 2] ALREADY shifted by + 0.5 (float64), lab: row of emb per point
        nrm = 2 * (pts / torch.tensor([img_w, img_h], device=DEV, dtype=torch.float64)) - 1
        ang = 2 * math.pi * (nrm @ G.double())
        keep = (lab != 0).double()[..., None]                       # label -1 (emb row 0): positional part zeroed (:90)
        return ang, keep, emb.double()[lab]

    for name, use_pts, pad, use_box in (("points", True, 0, False), ("points+pad", True, 1, False), ("boxes", False, 0, True), ("points+boxes", True, 0, True)):
        got = ops.sparse_embed(coords if use_pts else None, labels if use_pts else None, boxes if use_box else None, G, emb, P,
                               Np if use_pts else 0, pad, C, img_w, img_h)
        pts, lab = [], []
        if use_pts:
            pts.append(coords.double() + 0.5); lab.append(labels.long() + 1)
        if pad:
            pts.append(torch.zeros((P, 1, 2), device=DEV, dtype=torch.float64)); lab.append(torch.zeros((P, 1), device=DEV, dtype=torch.long))
        if use_box:
            pts.append(boxes.double().reshape(P, 2, 2) + 0.5); lab.append(torch.tensor([[3, 4]] * P, device=DEV))
        pts, lab = torch.cat(pts, 1), torch.cat(lab, 1)
        assert got.shape == (P, pts.shape[1], C)
        ang, keep, add = reference(pts, lab)
        ref_pos = torch.cat([torch.sin(ang), torch.cos(ang)], -1) * keep
        e = (got.double() - (ref_pos + add)).abs()
        amax = max(1.0, float(ang.abs().max()))
        ulp_sum = U23 * (ref_pos + add).abs()
        c = float(((e - ulp_sum).clamp(min=0) / (U23 * amax)).max())
        print(f"sparse_embed {name} C={C}: max |err| {float(e.max()):.3e}, max |angle| {amax:.2f}, measured c = {c:.3f} (bound {PE_C})")
        assert bool(torch.isfinite(got).all()) and bool((e <= PE_C * U23 * amax + ulp_sum).all()), (name, c)
        assert torch.equal(got[lab == 0], emb[0].expand(int((lab == 0).sum()), C))


@pytest.mark.parametrize("H,W,C", [(3, 5, 8), (3, 5, 512), (64, 64, 256)])
def test_dense_pe_against_float64_sin_cos(ops, H, W, C):
    """ullsam_dense_pe (prompt_encoder.py:230-241): sin | cos of 2 pi ((2 (x + 0.5) / W - 1) G0 + (2 (y + 0.5) / H - 1) G1) on the H x W grid, NHWC.
    Bound and measured constant: test_sparse_embed_against_float64_sin_cos."""
    G = _randn((2, C // 2), _gen(H + C))
    got = ops.dense_pe(G, H, W)
    ys = (torch.arange(H, device=DEV, dtype=torch.float64) + 0.5) / H
    xs = (torch.arange(W, device=DEV, dtype=torch.float64) + 0.5) / W
    nrm = 2 * torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W)], -1) - 1
    ang = 2 * math.pi * (nrm.reshape(H * W, 2) @ G.double())
    _pe_check(got, ang, torch.zeros((), device=DEV, dtype=torch.float64), f"dense_pe {H}x{W} C={C}")


@pytest.mark.parametrize("c1,c2", [(4, 16), (16, 64)])
@pytest.mark.parametrize("C", [8, 256, 260])
def test_mask_downscale_against_float64(ops, c1, c2, C):
    """ullsam_mask_downscale (prompt_encoder.py:54-62: conv k2 s2, LayerNorm2d, GELU, conv k2 s2, LayerNorm2d, GELU, conv 1x1) at SAM's widths and
    at the kernel's limits, C above its 256 threads, 2 x 3 output pixels, three masks; one 4 x 4 input patch constant and one all zero.  The first
    convolution's bias is 0.25 for every channel (its fp32 sums are exact), so the zero patch gives a channel vector of variance 0 (LayerNorm2d on eps alone); the
    constant patch has the same four values at its four sub-positions.  Float64 with erf GELU, at the 2e-5 bound of the fp32 LayerNorm chains."""
    P, H, W = 3, 2, 3
    g = _gen(c1 + C)
    masks = _randn((P, 1, 4 * H, 4 * W), g, 2.0)
    masks[1, 0, 0:4, 4:8] = 1.5
    masks[1, 0, 4:8, 0:4] = 0.0
    params = [_randn((c1, 1, 2, 2), g, 0.5), torch.full((c1,), 0.25, device=DEV), 1 + 0.1 * _randn((c1,), g), 0.1 * _randn((c1,), g),
              _randn((c2, c1, 2, 2), g, (4 * c1) ** -0.5), 0.1 * _randn((c2,), g), 1 + 0.1 * _randn((c2,), g), 0.1 * _randn((c2,), g),
              _randn((C, c2, 1, 1), g, c2 ** -0.5), 0.1 * _randn((C,), g)]
    got = ops.mask_downscale(masks, H, W, C, params)
    w0, b0, g1, be1, w3, b3, g4, be4, w6, b6 = [t.double() for t in params]

    def ln2d(x, wt, bs):                                            # common.py:38-43, eps 1e-6
        u = x.mean(1, keepdim=True)
        s_ = ((x - u) ** 2).mean(1, keepdim=True)
        return wt[None, :, None, None] * ((x - u) / torch.sqrt(s_ + 1e-6)) + bs[None, :, None, None]
    gelu = lambda t: 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))
    h1 = F.conv2d(masks.double(), w0, b0, stride=2)
    assert float(h1[1, :, 2:4, 0:2].var(0, unbiased=False).max()) == 0.0          # the zero patch: no spread over the channels
    h = gelu(ln2d(h1, g1, be1))
    h = gelu(ln2d(F.conv2d(h, w3, b3, stride=2), g4, be4))
    ref = F.conv2d(h, w6, b6).permute(0, 2, 3, 1).reshape(P, H * W, C)
    _within(got, ref, 2e-5, "mask_downscale")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("NM,H,W", [(1, 3, 5), (3, 3, 5), (4, 3, 5), (8, 3, 5), (3, 96, 96)])
def test_hyper_masks_against_float64_einsum(ops, dtype, NM, H, W):
    """ullsam_hyper_masks (mask_decoder.py:143-144) on the layout the two transposed convolutions leave as GEMM outputs:
    up2[nb, y, x, (ky, kx), (ky2, kx2), c] -> out[nb, m, 4 y + 2 ky + ky2, 4 x + 2 kx + kx2] = sum_c hyper[nb, m, c] up2[...].  96 x 96 x 16 outputs
    per image exceed the launch's 512 * 256 threads (grid-stride wrap).  Bound, derived: a sum of 32 products in fp32: 32 * 2^-24 * sum |h v|."""
    NB, CU = 2, 32
    g = _gen(NM + H)
    up2 = _randn((NB * H * W * 4, 4 * CU), g, dtype=dtype)
    hyper = _randn((NB, NM, CU), g)
    assert (H * W * 16 > 512 * 256) == (H == 96)
    got = ops.hyper_masks(up2, hyper, NB, NM, H, W, CU)
    u = up2.double().reshape(NB, H, W, 2, 2, 2, 2, CU)                              # [nb, y, x, ky, kx, ky2, kx2, c]
    ref = torch.einsum("nmc,nyxabdec->nmyadxbe", hyper.double(), u).reshape(NB, NM, 4 * H, 4 * W)
    bound = 32 * U24 * torch.einsum("nmc,nyxabdec->nmyadxbe", hyper.double().abs(), u.abs()).reshape(NB, NM, 4 * H, 4 * W)
    _within(got, ref, bound, "hyper_masks")


RESIZE_CASES = [  # name, stored (h, w), valid (h, w) | None, out (h, w)
    ("up", (16, 16), None, (64, 64)), ("down", (64, 48), None, (16, 12)), ("ratio", (37, 53), None, (64, 48)), ("same", (20, 20), None, (20, 20)),
    ("valid", (40, 56), (37, 53), (64, 48))]


def resize_case(name):
    """inputs uniform in (-0.5, 0.5) (CPU, [3, 1, h, w]) and the float64 F.interpolate(align_corners=False) of the valid region.  (The 1e-5 bound is
    absolute: at a ratio that is no power of two the fp32 source coordinate is off by ~3e-6 of a pixel, so the inputs' differences stay below 1.)"""
    _, stored, valid, out = next(c for c in RESIZE_CASES if c[0] == name)
    g = torch.Generator(); g.manual_seed(len(name))
    x = torch.rand((3, 1) + stored, generator=g) - 0.5
    ih, iw = valid or stored
    ref = F.interpolate(x.double()[..., :ih, :iw], size=out, mode="bilinear", align_corners=False)
    return x, valid, out, ref


@pytest.mark.parametrize("name", [c[0] for c in RESIZE_CASES])
def test_resize_bilinear_ratios_valid_region_and_mask(ops, name):
    """ullsam_resize_bilinear: 4x up, 4x down, 37 x 53 -> 64 x 48, same size (an exact copy), a valid region smaller than the stored plane
    (in_ld != IW), three planes, against float64 F.interpolate on the CPU at the existing 1e-5 bound.  The mask (threshold 0) equals
    `float output > thr` exactly, with and without the float output requested; against the float64 reference it is compared wherever
    |ref - thr| > 1e-5 (the share left out is computed from the reference and must be below 1 %)."""
    x, valid, out_hw, ref = resize_case(name)
    thr = 0.0
    got, mask = ops.resize_bilinear(x.to(DEV), out_hw, valid_hw=valid, threshold=thr)
    none, mask_only = ops.resize_bilinear(x.to(DEV), out_hw, valid_hw=valid, want_float=False, threshold=thr)
    only_float, no_mask = ops.resize_bilinear(x.to(DEV), out_hw, valid_hw=valid)
    assert none is None and no_mask is None and torch.equal(only_float, got)
    _within(got.cpu(), ref, 1e-5, f"resize_bilinear {name}")
    if name == "same":
        assert torch.equal(got.cpu(), x)
    assert mask.dtype == torch.uint8 and torch.equal(mask, (got > thr).to(torch.uint8)) and torch.equal(mask_only, mask)
    sure = (ref - thr).abs() > 1e-5
    assert float((~sure).double().mean()) < 0.01
    assert torch.equal(mask.cpu()[sure].bool(), (ref > thr)[sure])


@pytest.mark.parametrize("per", [1, 63, 257, 4097])
def test_mask_iou_counts_exact(ops, per):
    """ullsam_mask_iou_counts (train_joint_v2.py:683-694): {intersection, union} of byte masks, any non-zero byte counts as set (255 too), one pair
    of empty masks, three pairs; exact integers, and ops.mask_iou's (i + 1e-7) / (u + 1e-7) in float64."""
    g = _gen(per)
    vals = torch.tensor([0, 0, 1, 2, 255], dtype=torch.uint8, device=DEV)
    a = vals[torch.randint(0, 5, (3, per), device=DEV, generator=g)]
    b = vals[torch.randint(0, 5, (3, per), device=DEV, generator=g)]
    a[2] = 0; b[2] = 0
    a[0, 0] = 255; b[0, 0] = 255
    counts = torch.full((3, 2), -5, dtype=torch.int64, device=DEV)
    _lib().call("ullsam_mask_iou_counts", a.data_ptr(), b.data_ptr(), counts.data_ptr(), 3, per, _s())
    inter = ((a != 0) & (b != 0)).sum(-1)
    union = ((a != 0) | (b != 0)).sum(-1)
    assert counts[:, 0].tolist() == inter.tolist() and counts[:, 1].tolist() == union.tolist()
    assert counts[2].tolist() == [0, 0] and int(inter[0]) >= 1
    iou = ops.mask_iou(a, b)
    assert torch.equal(iou, (inter.double() + 1e-7) / (union.double() + 1e-7)) and float(iou[2]) == 1.0


@pytest.mark.parametrize("n", [4, 4 * 1027])
def test_threshold_u8_strict_and_special_values(n):
    """ullsam_threshold_u8: out = in > thr (strict), four values and a length that is no multiple of the 256-thread block; values equal to thr
    give 0, +-0.0 against thr = 0 give 0, NaN gives 0, +-inf as ordered.  Exact; one byte past the end keeps its sentinel."""
    for thr in (0.0, 0.75):
        x = _randn((n,), _gen(n))
        x[0], x[1], x[2], x[3] = thr, float("nan"), -0.0, 0.0
        if n > 8:
            x[4], x[5] = float("inf"), float("-inf")
            x[6], x[7] = float(np.nextafter(np.float32(thr), np.float32(1))), float(np.nextafter(np.float32(thr), np.float32(-1)))
        out = torch.full((n + 4,), 9, dtype=torch.uint8, device=DEV)
        _lib().call("ullsam_threshold_u8", x.data_ptr(), out.data_ptr(), n, thr, _s())
        assert torch.equal(out[:n], (x > thr).to(torch.uint8)) and bool((out[n:] == 9).all())
        assert out[:4].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("K", [4, 260, 2048])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_small_linear_strides_and_activations(K, act):
    """ullsam_small_linear with ldx > K, ldr > N, ldy > N (the sentinel between the output rows untouched), M * N = 15 outputs (the last workgroup
    is ragged), no activation / erf GELU / ReLU, with and without bias and residual.  Float64, at the existing 1e-5 bound (test_skinny_linear)."""
    M, N, ldx, ldr, ldy = 3, 5, K + 4, 8, 7
    g = _gen(K + act)
    xb, rb = _randn((M, ldx), g), _randn((M, ldr), g)
    W, b = _randn((N, K), g, K ** -0.5), _randn((N,), g)
    for use_b, use_r in ((True, True), (False, False)):
        y = torch.full((M, ldy), -77.0, device=DEV)
        _lib().call("ullsam_small_linear", xb.data_ptr(), ldx, W.data_ptr(), _p(b if use_b else None), _p(rb if use_r else None), ldr, y.data_ptr(), ldy,
                    M, N, K, act, _s())
        ref = xb[:, :K].double() @ W.double().T + (b.double() if use_b else 0)
        if act == 1:
            ref = 0.5 * ref * (1 + torch.erf(ref / math.sqrt(2.0)))
        elif act == 2:
            ref = ref.clamp(min=0)
        if use_r:
            ref = ref + rb[:, :N].double()
        _within(y[:, :N], ref, 1e-5, f"small_linear K={K} act={act}")
        assert bool((y[:, N:] == -77.0).all())


@pytest.mark.parametrize("n0,n1", [(0, 3), (5, 0), (5, 2)])
def test_concat_token_rows_empty_sides(ops, n0, n1):
    """ullsam_concat_token_rows (mask_decoder.py:119-123): no shared rows, no per-prompt rows, both; C = 4 (one 16-byte chunk per row), three prompts. Exact."""
    P, C = 3, 4
    g = _gen(n0 + 10 * n1)
    prefix, rows = _randn((n0, C), g), _randn((P, n1, C), g)
    got = ops.concat_token_rows(prefix, rows)
    assert torch.equal(got, torch.cat([prefix[None].expand(P, n0, C), rows], 1))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. attention edges (csrc/attention.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def masked_softmax_reference(q64, k64, v64, scale, key_mask):
    """float64 softmax of the fp32-FORMED masked logits (the product rounded to fp32, then the reference's additive finfo.min in fp32: a masked
    logit IS finfo.min, so a sequence whose keys are all masked is the plain mean of V): q [B, H, Sq, hd], k / v [B, H, Sk, hd], key_mask [B, Sk]"""
    sc = (q64 @ k64.transpose(-1, -2) * scale).float()
    if key_mask is not None:
        sc = sc + torch.where(key_mask[:, None, None, :] == 0, FMIN, 0.0).float()
    return torch.softmax(sc.double(), -1) @ v64


def naive_key_mask(B, Sk, device=DEV):
    """sample 0: left padding (up to three keys, one key always stays); sample 1: every key masked; the others: none"""
    m = torch.ones((B, Sk), dtype=torch.int32, device=device)
    m[0, :min(3, Sk - 1)] = 0
    m[1] = 0
    return m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,Sk,H,KVH", [(16, 1, 4, 4), (48, 257, 4, 2), (128, 1000, 4, 1), (256, 257, 2, 1)])
def test_naive_attention_strides_gqa_and_masks(dtype, hd, Sk, H, KVH):
    """ullsam_naive_attention, the q_len == 1 decode fallback: both dtypes, GQA, head widths that leave idle threads (48) or a single slice (256) in
    the P V pass, Sk of one key / just past the 256 threads / several trips, q taken from a packed qkv row, K / V in the cache layout [B, KVH, cap,
    hd], the output written into a wider buffer (sentinel intact), a left-padded key mask and a sequence whose keys are ALL masked (= mean of V).
    fp32: the existing 1e-5 bound (test_naive_and_fewkeys_attention); bf16: one bf16 step of the output scale on top."""
    B, Sq, cap, G = 3, 2, Sk + 3, H // KVH
    g = _gen(hd + Sk)
    row = (H + 2 * KVH) * hd
    qkv = _randn((B, Sq, row), g, dtype=dtype)
    kc, vc = _randn((B, KVH, cap, hd), g, dtype=dtype), _randn((B, KVH, cap, hd), g, dtype=dtype)
    mask = naive_key_mask(B, Sk)
    ldo = H * hd + 8
    out = torch.full((B * Sq, ldo), 5.0, dtype=dtype, device=DEV)
    scale = hd ** -0.5
    _lib().call("ullsam_naive_attention", 0 if dtype == torch.float32 else 1, qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), mask.data_ptr(),
                B, H, KVH, hd, Sq, Sk, Sq * row, row, hd, KVH * cap * hd, hd, cap * hd, KVH * cap * hd, hd, cap * hd, Sq * ldo, ldo, hd, scale, _s())
    q64 = qkv[..., :H * hd].double().reshape(B, Sq, H, hd).permute(0, 2, 1, 3)
    k64 = kc[:, :, :Sk].double().repeat_interleave(G, 1)
    v64 = vc[:, :, :Sk].double().repeat_interleave(G, 1)
    ref = masked_softmax_reference(q64, k64, v64, scale, mask)
    mean_v = v64[1].mean(-2, keepdim=True).expand(H, Sq, hd)
    assert float((ref[1] - mean_v).abs().max()) < 1e-12                           # the fully masked sequence really is uniform
    ref = ref.permute(0, 2, 1, 3).reshape(B * Sq, H * hd)
    bound = 1e-5 if dtype == torch.float32 else BF16_STEP * float(ref.abs().max()) + 1e-5
    _within(out[:, :H * hd], ref, bound, f"naive_attention hd={hd} Sk={Sk}")
    assert bool((out[:, H * hd:] == 5.0).all())


@pytest.mark.parametrize("hd,Sk", [(16, 1), (16, 512), (32, 256)])
def test_fewkeys_attention_key_count_limits(ops, hd, Sk):
    """ullsam_fewkeys_attention: one key, and the most keys the entry point accepts (K and V of a head in 64 KiB of LDS: Sk * hd * 8 <= 65536, i.e.
    512 keys at hd 16, 256 at hd 32; one more is refused with an error), 300 queries (a full and a ragged workgroup), shared and per-batch q.
    Float64, at the existing 1e-5 bound."""
    B, H, Sq = 2, 2, 300
    g = _gen(hd + Sk)
    q, k, v = _randn((B, Sq, H * hd), g), _randn((B, Sk, H * hd), g), _randn((B, Sk, H * hd), g)
    sp = lambda t: t.double().reshape(t.shape[0], t.shape[1], H, hd).permute(0, 2, 1, 3)
    for shared in (False, True):
        qq = q[:1].contiguous() if shared else q
        got = ops.fewkeys_attention(qq, k, v, B, H, hd, Sq, Sk, hd ** -0.5, q_shared=shared)
        ref = masked_softmax_reference(sp(qq).expand(B, H, Sq, hd), sp(k), sp(v), hd ** -0.5, None).permute(0, 2, 1, 3).reshape(B * Sq, H * hd)
        _within(got, ref, 1e-5, f"fewkeys_attention hd={hd} Sk={Sk} shared={shared}")
    if Sk > 1:
        assert Sk * hd * 8 == 64 * 1024
        big = torch.zeros((B, Sk + 1, H * hd), device=DEV)
        with pytest.raises(_lib().UllsamError):
            ops.fewkeys_attention(q, big, big, B, H, hd, Sq, Sk + 1, hd ** -0.5)


@pytest.mark.parametrize("B,KVH,G,Sk,pad,nsplit", [(2, 2, 1, 200, 70, 4), (2, 2, 3, 200, 70, 1), (2, 1, 4, 200, 70, 2), (2, 1, 8, 200, 70, 32),
                                                   (1, 2, 3, 5, 2, 32), (2, 2, 8, 70, 0, 32), (2, 1, 4, 513, 300, 2)])
def test_decode_attention_split_edges(B, KVH, G, Sk, pad, nsplit):
    """ullsam_decode_attention called directly with split counts the wrapper would not pick: 1, 2, 4, 32; more splits than keys (Sk 5 at 32 splits:
    27 trailing splits have no key; Sk 200 at 32: the last three); groups of 1 / 3 / 4 (the 4-wide kernel, filled and not) and 8 (the 8-wide
    one); left padding longer than a split (pad 70 of 200 at 4 splits of 50, ten whole splits at 32; pad 300 of 513 at 2 splits of 257), so that whole partials hold only
    finfo.min scores and the merge must give them zero weight.  Float64 as test_decode_attention, at its 2e-2 bound."""
    hd, H, cap = 128, KVH * G, Sk + 7
    g = _gen(Sk + G + nsplit)
    q = _randn((B, H * hd), g, dtype=torch.bfloat16)
    kc, vc = _randn((B, KVH, cap, hd), g, dtype=torch.bfloat16), _randn((B, KVH, cap, hd), g, dtype=torch.bfloat16)
    mask = torch.ones((B, Sk), dtype=torch.int32, device=DEV)
    mask[0, :pad] = 0
    per = -(-Sk // nsplit)
    if pad and nsplit >= 4:
        assert pad >= per                                                         # at least one split is wholly padded
    ws = torch.empty((B * KVH * nsplit * G * (hd + 2),), dtype=torch.float32, device=DEV)
    out = torch.full((B + 1, H * hd), 3.0, dtype=torch.bfloat16, device=DEV)
    _lib().call("ullsam_decode_attention", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), mask.data_ptr(), out.data_ptr(), B, H, KVH, hd, Sk, cap,
                hd ** -0.5, ws.data_ptr(), nsplit, _s())
    q64 = q.double().reshape(B, H, 1, hd)
    ref = masked_softmax_reference(q64, kc[:, :, :Sk].double().repeat_interleave(G, 1), vc[:, :, :Sk].double().repeat_interleave(G, 1), hd ** -0.5, mask)
    _within(out[:B], ref.reshape(B, H * hd), 2e-2, f"decode_attention G={G} Sk={Sk} nsplit={nsplit}")
    assert bool((out[B] == 3.0).all())
