"""The prefill attention kernels (ullsam_causal_attention, ullsam_vit_attention: ten instantiations behind one dispatcher) against the float64
definitions of tests/attention_ref.py, at their tile edges.

What is compared is the kernel's PROBABILITY MATRIX, entry by entry and relative to the entry: with V one-hot (attention_ref.probe_v) the
output columns are probabilities, and ceil(keys / head_dim) launches return all of them.  Per case:
  * every unmasked entry of every defined row:  |got - ref| <= tol * ref + 2^-100  (the tables keep ref >= 2^-90: the floor never decides);
  * masked entries of defined rows are exactly 0.0; every defined row sums to 1 within tol;
  * one random-V launch against the float64 outputs, the error normalised per row by that row's largest reference output, same tol;
  * undefined causal rows (left-padded queries): finite, non-negative weights that sum to 1 -- a convex combination of V rows;
  * causal128_attn_kernel and the tiled kernel (variant 11) equal bit for bit on every launch; variants 12 / 13 within 2^-6 * max of the default.
ViT windows: every pad token's V is the one vector qkv.bias, so no probe can tell two pad keys apart -- their probabilities are compared as
their sum (one extra probe slot, fed through bias_v); the live keys entry by entry.
64 x 64 global: the two marginals of the probability matrix (one-hot on the key's grid row, on its column) instead of 52 launches.

tol, bf16: 2^-6.  Derived, not measured: the format costs three half-ulps (2^-9 each: the P operand, the denominator summed from rounded P,
the stored output; attention_ref.bf16_model stays inside 3 * 2^-8 on every case, tests/test_attention_ref_cpu.py), one more half-ulp covers
fp32 arithmetic and v_exp_f32.
tol, fp32: 4 x the largest relative error, over the same entries, of a plain float32 evaluation of the same definition on the CPU (the
margin: another summation order, online rescaling, the hardware exponential), computed per case when the test runs.

Cache rows [Sk, k_cap) of K and V hold NaN in every causal launch here: a kernel that read them, at probability 0 even, would show.
Unaligned bases are refused before any launch (tests/test_attention_ref_cpu.py); there is no fallback left to run here.

Measured on an MI355X, largest over each family (CPU float32 error / kernel error / bound; bf16: kernel error against 2^-6 = 1.56e-2):
  bf16   causal, all five families        causal128 = tiled (variant 11) bit for bit: probabilities 7.4e-3 .. 7.6e-3, outputs 5.0e-3 .. 5.3e-3;
                                          head_dim 64: 7.4e-3 .. 7.7e-3, outputs 5.6e-3 .. 5.9e-3
         windows of 14                    win14r 8.0e-3 (outputs 5.6e-3); win14 (13), tiled 4-wave (2), tiled 7-wave (1): 8.3e-3 (outputs 5.8e-3)
         windows of 7 / 8 / 13            tiled 4-wave and 7-wave 7.6e-3 (outputs 4.9e-3)
         global, small and non-square     7.7e-3 (hd 64), 7.8e-3 (hd 80), outputs 5.3e-3
         global 64 x 64, marginals        vitglob 5.6e-3, tiled 8-wave (12) and 4-wave (9) 5.5e-3, hd 64 5.7e-3; outputs 5.2e-3 .. 6.0e-3
  fp32   the case of each family with the least room: CPU float32 / kernel / bound, and kernel : bound
         causal hd 128  shapes            sq2_past126        6.0e-7 / 1.4e-6 / 2.4e-6    0.59
                        leftpad           sq200_left32       1.9e-6 / 2.2e-6 / 7.5e-6    0.29
                        masks             hole_tile_64_127   1.9e-6 / 2.2e-6 / 7.5e-6    0.30
                        gqa               gqa_h8_kvh1        1.6e-6 / 1.7e-6 / 6.5e-6    0.27
                        logits            logits_rand1       1.8e-6 / 2.1e-6 / 7.4e-6    0.28   (the ramps: 8.2e-5 / 8.0e-5 / 3.3e-4)
         causal hd 64   shapes            sq2_past126        6.5e-7 / 1.0e-6 / 2.6e-6    0.39
                        leftpad           sq200_left32       1.4e-6 / 1.8e-6 / 5.7e-6    0.32
                        masks             tail70             1.3e-6 / 1.4e-6 / 5.3e-6    0.27
                        gqa               gqa_h2_kvh1        1.3e-6 / 1.7e-6 / 5.2e-6    0.32
                        logits            logits_spike_key0  1.1e-5 / 1.2e-5 / 4.2e-5    0.27   (the ramps: 3.9e-5 / 3.8e-5 / 1.6e-4)
         windows of 14                    win14_29x29_q6     1.2e-5 / 1.5e-5 / 4.9e-5    0.31
         windows of 7 / 8 / 13            win7_10x10         1.3e-6 / 2.0e-6 / 5.0e-6    0.40
         global, small and non-square     glob_8x8_hd64      1.3e-6 / 1.8e-6 / 5.1e-6    0.34   (1 x 1: 0 / 0 / 0, the one probability is exactly 1)
         global 64 x 64, marginals        glob_64x64_hd80    1.8e-6 / 2.3e-6 / 7.4e-6    0.31   (its random-V outputs: 6.2e-6, 0.85 of the bound)
  The random-V outputs of the other fp32 cases stay under 0.4 of their bound.
"""
import contextlib

import pytest
import torch

from tests import attention_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as o
    return o


@contextlib.contextmanager
def attn_variant(v):
    from ullsam_amd import _lib
    lib = _lib.load()
    try:
        lib.ullsam_set_attn_variant(v)
        yield
    finally:
        lib.ullsam_set_attn_variant(0)


def _dev(t):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in t.items()}


# ================================================================================================================ causal
def _causal_launch(ops, t, v, variant=0, fill=float("nan"), cap=None, rows=None):
    """-> out [B, Sq, H, hd].  K / V go into caches of `cap` rows whose rows [Sk, cap) hold `fill`."""
    B, H, KVH, hd, Sq, Sk = t["B"], t["H"], t["KVH"], t["hd"], t["Sq"], t["Sk"]
    cap = t["cap"] if cap is None else cap
    kc = torch.full((B, KVH, cap, hd), fill, dtype=t["q"].dtype, device=DEV)
    vc = torch.full((B, KVH, cap, hd), fill, dtype=t["q"].dtype, device=DEV)
    kc[:, :, :Sk] = t["k"]
    vc[:, :, :Sk] = v
    q, m = t["q"], t["mask"]
    if rows is not None:                                                                     # a call on some batch rows only
        q, kc, vc, m, B = q[rows].contiguous(), kc[rows].contiguous(), vc[rows].contiguous(), None if m is None else m[rows].contiguous(), len(rows)
    with attn_variant(variant):
        out = ops.causal_attention(q.reshape(B * Sq, H * hd), kc, vc, m, B, H, KVH, hd, Sq, Sk, t["q_pos0"])
    return out.reshape(B, Sq, H, hd)


def _causal_tol(name, c, dtype, hd, keep_cpu):
    """bf16: 2^-6.  fp32: 4 x the error of the float32 evaluation on the CPU over the same entries."""
    if dtype == torch.bfloat16:
        return R.BF16_TOL, None
    t = R.build_causal(name, c, dtype, hd)
    _, P64, _ = R.causal_ref(t["q"], t["k"], t["v"], t["mask"], t["q_pos0"])
    _, P32, _ = R.causal_ref(t["q"], t["k"], t["v"], t["mask"], t["q_pos0"], dtype=torch.float32)
    e32 = R.rel_err(P32, P64, keep_cpu)
    return R.F32_MARGIN * e32, e32


def _run_causal_case(ops, kernel, name, c):
    dtype, hd, variant = R.CAUSAL_KERNELS[kernel]
    t = _dev(R.build_causal(name, c, dtype, hd))
    B, H, KVH, Sq, Sk, p0 = t["B"], t["H"], t["KVH"], t["Sq"], t["Sk"], t["q_pos0"]
    ref_out, P, defined = R.causal_ref(t["q"], t["k"], t["v"], t["mask"], p0)
    ok = R.causal_unmasked(t["mask"], B, Sq, Sk, p0, DEV)[:, None].expand(B, H, Sq, Sk)
    tol, e32 = _causal_tol(name, c, dtype, hd, ok.cpu())
    what = f"causal {kernel} {name}"
    twin = kernel == "causal128"                                                             # documented bit-identical: the tiled kernel under variant 11
    outs = []
    for run in range(R.n_runs(Sk, hd)):
        v = R.probe_v(Sk, hd, run).to(DEV).to(dtype).expand(B, KVH, Sk, hd)
        outs.append(_causal_launch(ops, t, v, variant))
        if twin:
            assert torch.equal(outs[-1], _causal_launch(ops, t, v, 11)), f"{what}: probe run {run} differs from the tiled kernel"
    got = R.recover_p(outs, Sk).permute(0, 2, 1, 3).double()                                 # [B, H, Sq, Sk]
    assert bool(torch.isfinite(got).all()), what
    drow = defined[:, None, :, None].expand_as(ok)
    worst = R.check_entries(got, P, ok, tol, what)
    assert bool((got[drow & ~ok] == 0).all()), f"{what}: a masked key of a defined row has weight"
    sums = got.sum(-1)
    assert float((sums - 1).abs()[defined[:, None].expand_as(sums)].max()) <= tol, what
    und = ~defined[:, None].expand_as(sums)
    if bool(und.any()):                                                                      # left-padded queries: a convex combination of V rows
        assert bool((got >= 0).all()) and float((sums - 1).abs()[und].max()) <= max(tol, R.BF16_TOL), f"{what}: undefined rows"
    out = _causal_launch(ops, t, t["v"], variant)
    if twin:
        assert torch.equal(out, _causal_launch(ops, t, t["v"], 11)), f"{what}: random V differs from the tiled kernel"
    assert bool(torch.isfinite(out.float()).all()), what
    wout = R.check_outputs(out, ref_out, defined[:, :, None].expand(B, Sq, H), tol, what)
    if bool(und.any()):
        assert float(out[~defined].float().abs().max()) <= float(t["v"][-1].float().abs().max()) * (1 + R.BF16_TOL)
    if e32 is not None:
        print(f"{what}: fp32 figures: CPU float32 {e32:.3e}, kernel {worst:.3e}, bound {tol:.3e}, outputs {wout:.3e}")
    return worst


@pytest.mark.parametrize("family", list(R.CAUSAL_FAMILIES))
@pytest.mark.parametrize("kernel", list(R.CAUSAL_KERNELS))
def test_causal_attention_probabilities_against_float64(ops, kernel, family):
    """Every case of the family through one kernel: 128-query workgroups, 32-query waves, 64-key tiles and 32-key blocks with their edges at
    31 / 32 / 33, 63 / 65, 127 / 128 / 129 and q_pos0 not a multiple of 32; padding that fills whole blocks and tiles; holes and right padding;
    GQA groups; logits whose maximum moves in every block, never, or sits on key 0 / on the diagonal."""
    worst = max(_run_causal_case(ops, kernel, name, c) for name, c in R.CAUSAL_FAMILIES[family].items())
    print(f"FAMILY causal {kernel} {family}: largest relative error {worst:.3e}")


@pytest.mark.parametrize("kernel", list(R.CAUSAL_KERNELS))
def test_causal_attention_a_batch_row_without_any_key(ops, kernel):
    """One batch row's mask is all zeros: that row is only finite, and the other batch row keeps its bits against the same call without it."""
    dtype, hd, variant = R.CAUSAL_KERNELS[kernel]
    t = _dev(R.build_causal("all_zero_row", dict(Sq=200, q_pos0=0, mask=("left", 200)), dtype, hd))
    assert int(t["mask"][-1].sum()) == 0 and int(t["mask"][0].sum()) == 200
    both = _causal_launch(ops, t, t["v"], variant)
    alone = _causal_launch(ops, t, t["v"], variant, rows=[0])
    assert bool(torch.isfinite(both.float()).all())
    assert torch.equal(both[:1], alone)


@pytest.mark.parametrize("Sq,q_pos0", [(64, 0), (129, 0), (200, 190)])
@pytest.mark.parametrize("kernel", list(R.CAUSAL_KERNELS))
def test_causal_attention_never_reads_cache_rows_past_sk(ops, kernel, Sq, q_pos0):
    """k_cap = Sk + 5 with NaN in rows [Sk, cap) of K and V gives the bits that zeros there give, and that k_cap == Sk gives."""
    dtype, hd, variant = R.CAUSAL_KERNELS[kernel]
    t = _dev(R.build_causal(f"cache_{Sq}_{q_pos0}", dict(Sq=Sq, q_pos0=q_pos0), dtype, hd))
    nan = _causal_launch(ops, t, t["v"], variant)
    zero = _causal_launch(ops, t, t["v"], variant, fill=0.0)
    tight = _causal_launch(ops, t, t["v"], variant, cap=t["Sk"])
    assert bool(torch.isfinite(nan.float()).all())
    assert torch.equal(nan, zero) and torch.equal(nan, tight)


# ================================================================================================================ ViT
def _vit_launch(ops, t, qkv, bias, variant=0):
    """-> out [B, gh*gw, heads, hd]"""
    with attn_variant(variant):
        out = ops.vit_attention(qkv, t["rel_h"], t["rel_w"], bias, t["B"], t["heads"], t["hd"], t["gh"], t["gw"], t["window"])
    return out.reshape(t["B"], t["gh"] * t["gw"], t["heads"], t["hd"])


_VIT_REF = {}


def _vit_reference(name, c, dtype):
    """Computed once per (case, dtype) and shared, never changed: float64 probabilities in the layout of the kernel's output rows, the compared
    slots, the float64 outputs, and for fp32 the error of the float32 evaluation on the CPU over the same entries."""
    key = (name, dtype)
    if key not in _VIT_REF:
        cpu = R.build_vit(name, c, dtype)
        t = _dev(cpu)
        args = (c["B"], c["heads"], c["hd"], c["gh"], c["gw"], c["window"])
        out, P = R.vit_ref(t["qkv"], t["rel_h"], t["rel_w"], t["bias"], *args)
        W = c["window"]
        tok = R.window_layout(c["gh"], c["gw"], W)[0] if W else torch.arange(c["gh"] * c["gw"])[None]
        big = W == 0 and c["gh"] * c["gw"] > 2048                                            # 64 x 64 global: the two marginals
        if big:
            Pg = P.reshape(c["B"], c["heads"], 4096, 64, 64)
            want = torch.stack([Pg.sum(-1), Pg.sum(-2)]).permute(0, 1, 3, 2, 4)              # [row | col, B, N, heads, 64]
            keys = None
        else:
            want = R.vit_token_p(P, tok.to(DEV), c["gh"], c["gw"])                           # [B, N, heads, Nw + 1]
            keys = R.vit_token_keys(tok, c["gh"], c["gw"]).to(DEV)
        e32 = None
        if dtype == torch.float32:
            targs = (cpu["qkv"], cpu["rel_h"], cpu["rel_w"], cpu["bias"])
            P32 = R.vit_ref(*targs, *args, dtype=torch.float32)[1]
            P64 = P.cpu()
            if big:
                m = lambda X: torch.stack([X.reshape(c["B"], c["heads"], 4096, 64, 64).sum(-1), X.reshape(c["B"], c["heads"], 4096, 64, 64).sum(-2)])
                e32 = R.rel_err(m(P32), m(P64), torch.ones(2, c["B"], c["heads"], 4096, 64, dtype=torch.bool))
            else:
                a, b = R.vit_token_p(P32.double(), tok, c["gh"], c["gw"]), R.vit_token_p(P64, tok, c["gh"], c["gw"])
                e32 = R.rel_err(a, b, keys.cpu()[None, :, None, :].expand_as(b))
        _VIT_REF[key] = dict(t=t, want=want, keys=keys, out=out.reshape(c["B"], -1, c["heads"], c["hd"]), e32=e32, N=tok.shape[1], big=big)
        del P
    return _VIT_REF[key]


def _run_vit_case(ops, kernel, name, c, dtype, variant, noise_twin=None):
    ref = _vit_reference(name, c, dtype)
    t, N = ref["t"], ref["N"]
    tol = R.BF16_TOL if dtype == torch.bfloat16 else R.F32_MARGIN * ref["e32"]
    what = f"vit {kernel} {name}"
    if ref["big"]:
        got = torch.stack([_vit_launch(ops, t, *[x.to(DEV) for x in R.vit_probe_qkv(t["qkv"].cpu(), t["bias"].cpu(), c, 0, mode)], variant)[..., :64]
                           for mode in ("row", "col")]).double()
        keep = torch.ones_like(got, dtype=torch.bool)
        want = ref["want"]
        sums = got.sum(-1)
    else:
        outs = [_vit_launch(ops, t, *[x.to(DEV) for x in R.vit_probe_qkv(t["qkv"].cpu(), t["bias"].cpu(), c, run)], variant)
                for run in range(R.vit_probe_runs(c))]
        got = torch.cat(outs, -1).double()
        n = min(got.shape[-1], N + 1)
        got, want = got[..., :n], ref["want"][..., :n]
        keep = ref["keys"][None, :, None, :n].expand_as(got)
        assert int(ref["keys"][:, n:].sum()) == 0                                            # no compared slot is left out
        assert bool((got[~keep] == 0).all())
        sums = got.sum(-1)
    assert bool(torch.isfinite(got).all()), what
    worst = R.check_entries(got, want, keep, tol, what)
    assert float((sums - 1).abs().max()) <= tol, (what, float((sums - 1).abs().max()))
    out = _vit_launch(ops, t, t["qkv"], t["bias"], variant)
    assert bool(torch.isfinite(out.float()).all()), what
    wout = R.check_outputs(out, ref["out"], torch.ones(out.shape[:-1], dtype=torch.bool, device=DEV), tol, what)
    if noise_twin is not None:                                                               # documented equal to bf16 noise: against the default kernel
        base = _vit_launch(ops, t, t["qkv"], t["bias"], noise_twin)
        d = float((out.float() - base.float()).abs().max())
        assert d <= 2.0 ** -6 * max(1.0, float(base.float().abs().max())), (what, d)
    if ref["e32"] is not None:
        print(f"{what}: fp32 figures: CPU float32 {ref['e32']:.3e}, kernel {worst:.3e}, bound {tol:.3e}, outputs {wout:.3e}")
    return worst


@pytest.mark.parametrize("kernel", list(R.WINDOW14_KERNELS))
def test_vit_window14_attention_probabilities_against_float64(ops, kernel):
    """SAM's 14 x 14 windows at head_dim 80 through the row-group kernel, the block kernel (variant 13), the 4-wave and 7-wave tiled kernels
    (variants 2 and 1) and fp32: whole windows, windows with one live row or column (15 x 15, 29 x 29, 57 x 14), non-square grids, 25 windows
    of the 64 x 64 grid; three probe launches recover the full 196 x 196 matrix of every window, the pad keys as their sum."""
    dtype, variant = R.WINDOW14_KERNELS[kernel]
    worst = max(_run_vit_case(ops, kernel, name, c, dtype, variant, noise_twin=0 if variant == 13 else None) for name, c in R.WINDOW14_CASES.items())
    print(f"FAMILY vit window14 {kernel}: largest relative error {worst:.3e}")


@pytest.mark.parametrize("kernel", list(R.WINDOW_OTHER_KERNELS))
def test_vit_other_windows_attention_probabilities_against_float64(ops, kernel):
    """Windows of 7, 8 and 13 tokens (49, 64 and 169 keys: under one tile, exactly one, ragged) through the tiled kernels."""
    dtype, variant = R.WINDOW_OTHER_KERNELS[kernel]
    worst = max(_run_vit_case(ops, kernel, name, c, dtype, variant) for name, c in R.WINDOW_OTHER_CASES.items())
    print(f"FAMILY vit window_other {kernel}: largest relative error {worst:.3e}")


@pytest.mark.parametrize("kernel", list(R.GLOBAL_SMALL_KERNELS))
@pytest.mark.parametrize("hd", [64, 80])
def test_vit_global_attention_on_small_and_non_square_grids_against_float64(ops, kernel, hd):
    """Global attention with full recovery of the probability matrix: 1, 4, 49 keys, exactly one 64-key tile (8 x 8), 72 keys, 1089 keys with a
    ragged last tile, and grid_h != grid_w (5 x 64, 64 x 5, 33 x 20), where rel_h has 2*grid_h - 1 rows and its own offset."""
    dtype, variant = R.GLOBAL_SMALL_KERNELS[kernel]
    cases = {n: c for n, c in R.GLOBAL_SMALL_CASES.items() if c["hd"] == hd}
    worst = max(_run_vit_case(ops, kernel, name, c, dtype, variant) for name, c in cases.items())
    print(f"FAMILY vit global_small {kernel} hd{hd}: largest relative error {worst:.3e}")


@pytest.mark.parametrize("kernel", list(R.GLOBAL64_KERNELS))
def test_vit_global_attention_64x64_marginals_against_float64(ops, kernel):
    """The 64 x 64 grid through the LDS-DMA kernel, the 8-wave and 4-wave tiled kernels (variants 12 and 9), fp32, and head_dim 64: the row and
    column marginals of the 4096 x 4096 probability matrix, and one random-V launch."""
    dtype, variant, name = R.GLOBAL64_KERNELS[kernel]
    worst = _run_vit_case(ops, kernel, name, R.GLOBAL64_CASES[name], dtype, variant, noise_twin=0 if variant == 12 else None)
    print(f"FAMILY vit global64 {kernel}: largest relative error {worst:.3e}")


# ================================================================================================================ launch and memory contract
GUARD = 4096          # elements of NaN on both sides of a test-owned output (a multiple of 16 bytes)


def _guarded(n, dtype):
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def _assert_written_and_guarded(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), f"{what}: wrote outside its output"
    assert not bool(torch.isnan(buf[GUARD:GUARD + n]).any()), f"{what}: left part of its output unwritten"


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("kernel", list(R.CAUSAL_KERNELS))
@pytest.mark.parametrize("Sq,q_pos0", [(70, 0), (130, 62)])
def test_causal_attention_writes_its_output_and_nothing_else(ops, kernel, Sq, q_pos0):
    from ullsam_amd import _lib
    from ullsam_amd.ops import dt_code
    dtype, hd, variant = R.CAUSAL_KERNELS[kernel]
    t = _dev(R.build_causal(f"contract_{Sq}", dict(Sq=Sq, q_pos0=q_pos0, mask=("left", q_pos0 + 9)), dtype, hd))   # left-padded queries are written too
    B, H, KVH, Sk = t["B"], t["H"], t["KVH"], t["Sk"]
    n = B * Sq * H * hd
    buf, ptr = _guarded(n, dtype)
    kc, vc, q = t["k"].contiguous(), t["v"].contiguous(), t["q"].contiguous()
    with attn_variant(variant):
        _lib.call("ullsam_causal_attention", dt_code(dtype), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ptr, t["mask"].data_ptr(),
                  B, H, KVH, hd, Sq, Sk, Sk, q_pos0, _stream())
    _assert_written_and_guarded(buf, n, f"causal {kernel}")
    out = _causal_launch(ops, t, t["v"], variant, cap=Sk)                                    # the same call into an output of its own
    assert torch.equal(buf[GUARD:GUARD + n].reshape(out.shape), out)


@pytest.mark.parametrize("kernel,name", [("win14r", "win14_29x29"), ("win14_v13", "win14_29x29"), ("tiled4_v2", "win14_16x30"), ("tiled7_v1", "win14_30x16"),
                                         ("fp32", "win14_15x15"), ("glob_bf16", "glob_8x9_hd80"), ("glob_fp32", "glob_33x20_hd64"),
                                         ("vitglob", "glob_64x64_hd80")])
def test_vit_attention_writes_its_output_and_nothing_else(kernel, name):
    """Windows with cropped query rows (their pad queries are computed and must not be stored anywhere) and global grids."""
    from ullsam_amd import _lib
    from ullsam_amd.ops import dt_code
    c = next(cs[name] for cs in R.VIT_FAMILIES.values() if name in cs)
    dtype, variant = ({**R.WINDOW14_KERNELS, "glob_bf16": (torch.bfloat16, 0), "glob_fp32": (torch.float32, 0), "vitglob": (torch.bfloat16, 0)})[kernel]
    t = _dev(R.build_vit(name, c, dtype))
    n = c["B"] * c["gh"] * c["gw"] * c["heads"] * c["hd"]
    buf, ptr = _guarded(n, dtype)
    with attn_variant(variant):
        _lib.call("ullsam_vit_attention", dt_code(dtype), t["qkv"].data_ptr(), ptr, t["rel_h"].data_ptr(), t["rel_w"].data_ptr(), t["bias"].data_ptr(),
                  c["B"], c["heads"], c["hd"], c["gh"], c["gw"], c["window"], _stream())
    _assert_written_and_guarded(buf, n, f"vit {kernel} {name}")
