"""tests/decoder_ref.py on the CPU: (1) its float64 definitions of the fused decoder launches, composed into a whole mask-decoder pass, against the independent
numpy oracle (oracle/ullsam_oracle.py two_way_transformer / mask_decoder) -- this pins the layer-0 "no pe, no residual" rule, where pe is added, which
tensors are keys and values of which attention, the chain order of the heads and the (ky, kx, c) layouts of the two transposed convolutions, without anything
under ullsam_amd/; (2) every limit tests/test_decoder_kernels_gpu.py sets is attainable by the arithmetic the kernels declare: for the GPU file's own inputs
the two-term evaluation D2 of the definition sits at least 2x inside the limit (which is stated in the one-term evaluation D1's error)."""
import numpy as np
import pytest
import torch

from oracle import ullsam_oracle as O
from tests import decoder_ref as R

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()


def _decoder_pass(Pm, img, pe, sparse, dense):
    """MaskDecoder.predict_masks from decoder_ref's launches; Pm: the oracle's parameter dict (fp32 values, used as given); img / pe [1, 256, h, w]"""
    W = lambda n: T64(Pm[n])
    P, h, w = sparse.shape[0], img.shape[2], img.shape[3]
    N = h * w
    tokens = torch.cat([torch.cat([W("iou_token.weight"), W("mask_tokens.weight")], 0)[None].expand(P, -1, -1), T64(sparse)], 1)
    keys = (T64(img) + T64(dense)).reshape(-1, 256, N).transpose(1, 2).expand(P, -1, -1)
    key_pe = T64(pe).reshape(256, N).T

    def att(pre):
        return [W(pre + n + s) for n in ("q_proj", "k_proj", "v_proj", "out_proj") for s in (".weight", ".bias")]

    def norm(pre):
        return (W(pre + ".weight"), W(pre + ".bias"), 1e-5)

    queries, qpe = tokens, tokens
    for i in range(2):
        b = f"transformer.layers.{i}."
        sa, t2i, i2t = att(b + "self_attn."), att(b + "cross_attn_token_to_image."), att(b + "cross_attn_image_to_token.")
        queries, q2 = R.tok_attn(queries, qpe, *sa, *norm(b + "norm1"), t2i[0], t2i[1], skip_pe=(i == 0), mode=0)
        k, v = R.kv_proj(keys + key_pe, keys, t2i[2], t2i[3], t2i[4], t2i[5])
        a = R.attention_core(q2, k, v, R.HEADS)
        queries, kt, vt = R.tok_mlp(queries, a, qpe, t2i[6], t2i[7], norm(b + "norm2"), W(b + "mlp.lin1.weight"), W(b + "mlp.lin1.bias"), W(b + "mlp.lin2.weight"),
                                    W(b + "mlp.lin2.bias"), norm(b + "norm3"), i2t[2], i2t[3], i2t[4], i2t[5], do_mlp=1)
        keys = R.i2t(keys + key_pe, keys, i2t[0], i2t[1], kt, vt, i2t[6], i2t[7], *norm(b + "norm4"), key_pe, 0.25, cast=False)
    fin = att("transformer.final_attn_token_to_image.")
    _, q2 = R.tok_attn(queries, qpe, None, None, None, None, None, None, None, None, None, None, 0.0, fin[0], fin[1], skip_pe=0, mode=1)
    k, v = R.kv_proj(keys + key_pe, keys, fin[2], fin[3], fin[4], fin[5])
    queries, _, _ = R.tok_mlp(queries, R.attention_core(q2, k, v, R.HEADS), None, fin[6], fin[7], norm("transformer.norm_final_attn"), *([None] * 4), None,
                              *([None] * 4), do_mlp=0)
    chains = [[(W(f"output_hypernetworks_mlps.{c}.layers.{l}.weight"), W(f"output_hypernetworks_mlps.{c}.layers.{l}.bias")) for l in range(3)] for c in range(4)]
    chains.append([(W(f"iou_prediction_head.layers.{l}.weight"), W(f"iou_prediction_head.layers.{l}.bias")) for l in range(3)])
    hyper, iou = R.heads(queries, chains, 0, 4, 4)
    ct = lambda n: (W(n + ".weight").permute(2, 3, 1, 0).reshape(-1, W(n + ".weight").shape[0]), W(n + ".bias").repeat(4))     # [Cin, Cout, ky, kx] -> [(ky, kx, c), Cin]
    u1 = R.up1(keys.reshape(P * N, 256), *ct("output_upscaling.0"), W("output_upscaling.1.weight"), W("output_upscaling.1.bias"), 1e-6)
    masks = R.up2(u1, *ct("output_upscaling.3"), hyper, P, 4, h, w, cast=False)
    return queries, keys, masks, iou


def test_definitions_compose_into_the_oracles_mask_decoder():
    """depth 2, P = 2, T = 7, N = 64 (8 x 8): tokens and image side of the two-way transformer within 2e-5 (the project's bound for fp32 LayerNorm chains: the
    oracle is fp32, both outputs leave a LayerNorm with values of order 1), masks and IoU within 1e-4 of their largest value (three / five more fp32 linears
    behind those).  A misplaced pe, a residual in layer 0, swapped keys / values or a wrong chain moves these numbers by 1e-1 and more."""
    Pm = O.fill_state(O.mask_decoder_shapes())
    rng = np.random.default_rng(5)
    img, pe = rng.standard_normal((1, 256, 8, 8), dtype=np.float32), rng.standard_normal((1, 256, 8, 8), dtype=np.float32)
    sparse, dense = rng.standard_normal((2, 2, 256), dtype=np.float32), rng.standard_normal((1, 256, 8, 8), dtype=np.float32)
    tokens = np.concatenate([np.broadcast_to(np.concatenate([Pm["iou_token.weight"], Pm["mask_tokens.weight"]], 0)[None], (2, 5, 256)), sparse], 1).astype(np.float32)
    hs_o, keys_o = O.two_way_transformer(Pm, "transformer.", np.repeat(img, 2, 0) + dense, np.repeat(pe, 2, 0), tokens)
    m3, i3 = O.mask_decoder(Pm, img, pe, sparse, dense, True)
    m1, i1 = O.mask_decoder(Pm, img, pe, sparse, dense, False)
    masks_o, iou_o = np.concatenate([m1, m3], 1), np.concatenate([i1, i3], 1)
    hs, keys, masks, iou = _decoder_pass(Pm, img, pe, sparse, dense)
    assert hs.shape == (2, 7, 256) and keys.shape == (2, 64, 256) and masks.shape == (2, 4, 32, 32) and iou.shape == (2, 4)
    for name, got, ref, tol in (("tokens", hs, hs_o, 2e-5), ("keys", keys, keys_o, 2e-5), ("masks", masks, masks_o, 1e-4), ("iou", iou, iou_o, 1e-4)):
        ref = T64(ref)
        e, scale = float((got - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print(f"{name}: max |definition - oracle| {e:.3e} (scale {scale:.2f})")
        assert e <= tol * scale, (name, e, scale)


def _two_term_inside(outs, what):
    """outs: [(name, D, D1, D2)]: D2's error at least 2x inside the GPU limit E1 / 64, max and rms"""
    for name, D, D1, D2 in outs:
        (m1, r1), (m2, r2) = R.err(D1, D), R.err(D2, D)
        print(f"{what} {name}: D1 max {m1:.2e} rms {r1:.2e}; D2 max {m2:.2e} rms {r2:.2e}; D2 / limit max {m2 / (m1 / 64):.3f} rms {r2 / (r1 / 64):.3f}")
        assert m1 > 0 and r1 > 0, (what, name)
        assert m2 <= m1 / 128 and r2 <= r1 / 128, (what, name, m1, m2, r1, r2)


@pytest.mark.parametrize("T", R.TOK_T)
@pytest.mark.parametrize("P", R.TOK_P)
def test_two_terms_sit_inside_the_token_kernels_limits(P, T):
    d = R.tok_attn_case(P, T)
    for skip_pe, mode in ((0, 0), (1, 0), (0, 1)):
        D, D1, D2 = (R.tok_attn(*R.tok_attn_args(d, skip_pe, mode, r)) for r in (R.ident, R.bf1, R.bf2))
        names = ("queries", "q_t2i") if mode == 0 else (None, "q_t2i")
        _two_term_inside([(n, D[i], D1[i], D2[i]) for i, n in enumerate(names) if n], f"tok_attn P={P} T={T} skip_pe={skip_pe} mode={mode}")
    d = R.tok_mlp_case(P, T)
    for do_mlp in (1, 0):
        D, D1, D2 = (R.tok_mlp(*R.tok_mlp_args(d, do_mlp, r)) for r in (R.ident, R.bf1, R.bf2))
        names = ("queries", "k", "v") if do_mlp else ("queries",)
        _two_term_inside([(n, D[i], D1[i], D2[i]) for i, n in enumerate(names)], f"tok_mlp P={P} T={T} do_mlp={do_mlp}")


@pytest.mark.parametrize("case", R.HEADS_CASES)
def test_two_terms_sit_inside_the_heads_limits(case):
    P, T, m0, nm, n_iou = case
    hs, chains = R.heads_case(P, T, n_iou)
    D, D1, D2 = (R.heads(hs, chains, m0, nm, n_iou, r) for r in (R.ident, R.bf1, R.bf2))
    _two_term_inside([(n, D[i], D1[i], D2[i]) for i, n in enumerate(("hyper", "iou"))], f"heads {case}")


@pytest.mark.parametrize("name", R.TOK_ATTN_SPECIAL)
def test_two_terms_sit_inside_the_limits_of_the_special_tok_attn_inputs(name):
    d, skips, names = R.tok_attn_special(name)
    for skip_pe in skips:
        D, D1, D2 = (R.tok_attn(*R.tok_attn_args(d, skip_pe, 0, r)) for r in (R.ident, R.bf1, R.bf2))
        if name == "constant_row":         # queries' = ln_b exactly in every arithmetic (the GPU file asserts equality there, no limit)
            assert all(float((x[0] - d["ln_b"].double()).abs().max()) == 0.0 for x in (D, D1, D2))
        _two_term_inside([(n, D[i], D1[i], D2[i]) for i, n in enumerate(("queries", "q_t2i")) if n in names], f"tok_attn {name} skip_pe={skip_pe}")


@pytest.mark.parametrize("name", R.TOK_MLP_SPECIAL)
def test_two_terms_sit_inside_the_limits_of_the_special_tok_mlp_inputs(name):
    """null operands; the dead hidden layer (every ReLU output zero: D1's error has no MLP share, the limit shrinks with it)"""
    d = R.tok_mlp_special(name)
    for do_mlp in (1, 0) if name == "nulls" else (1,):
        D, D1, D2 = (R.tok_mlp(*R.tok_mlp_args(d, do_mlp, r)) for r in (R.ident, R.bf1, R.bf2))
        names = ("queries", "k", "v") if do_mlp else ("queries",)
        _two_term_inside([(n, D[i], D1[i], D2[i]) for i, n in enumerate(names)], f"tok_mlp {name} do_mlp={do_mlp}")


@pytest.mark.parametrize("chain", R.HEADS_NULL_CHAINS)
def test_two_terms_sit_inside_the_limits_of_the_heads_with_null_biases(chain):
    hs, chains = R.heads_null_case(chain)
    D, D1, D2 = (R.heads(hs, chains, 0, 4, 4, r) for r in (R.ident, R.bf1, R.bf2))
    _two_term_inside([(n, D[i], D1[i], D2[i]) for i, n in enumerate(("hyper", "iou"))], f"heads null biases of chain {chain}")


def _i2t_inside(d, T, what):
    """rms(D2 - D) <= rms(D1 - D) / 16 (the GPU limit is / 8) and every element of D2 within half of the written-out bound -> (D, rms limit of the GPU file)"""
    D, D1, D2 = (R.i2t(*R.i2t_args(d, r)) for r in (R.ident, R.bf1, R.bf2))
    (m1, r1), (m2, r2) = R.err(D1, D), R.err(D2, D)
    worst = float(((D2 - D).abs() / R.i2t_bound(d)).max())
    print(f"i2t {what}: D1 max {m1:.2e} rms {r1:.2e}; D2 max {m2:.2e} rms {r2:.2e}; D2 rms / limit {r2 / max(r1 / 8, 1e-300):.3f}, worst err / bound {worst:.3f}")
    if T == 1:
        assert m1 == 0.0 and m2 == 0.0
    else:
        assert r2 <= r1 / 16, (r1, r2)
    assert worst <= 0.5
    return D, r1 / 8


@pytest.mark.parametrize("case", R.I2T_CASES)
def test_two_terms_sit_inside_the_image_to_token_limits(case):
    """with T = 1 every arithmetic gives the definition exactly (softmax = 1, a = v ... up to the two-term value of v: its cast to bf16 is the same).  The
    cases with hundreds of prompts are evaluated on their first 8 prompts (same inputs, N, T and weights: the error statistics do not depend on P)."""
    P, N, T, shared = case
    _i2t_inside(R.i2t_prompts(R.i2t_case(P, N, T, shared), 8), T, str(case))


@pytest.mark.parametrize("name", sorted(R.I2T_SPECIAL))
def test_two_terms_sit_inside_the_limits_of_the_special_image_to_token_inputs(name):
    """null operands and the residual offsets; at offset 200 a ONE-pass fp32 variance in norm4, even with the best summation order, breaks the GPU file's rms
    limit (so that input enforces the two-pass form), while at 50 it would still fit."""
    d = R.i2t_special(name)
    D, limit = _i2t_inside(d, R.I2T_SPECIAL[name][2], name)
    if name.startswith("offset"):
        y = R.i2t(*R.i2t_args(d, R.ident, True, True))[3]
        _, bad = R.err(R.norm4_one_pass_fp32(y, d["lnw"], d["lnb"], d["eps"]), D)
        print(f"i2t {name}: one-pass fp32 norm4 rms {bad:.2e}, limit {limit:.2e}: {bad / limit:.2f}")
        if name == "offset200":
            assert bad > 2 * limit


@pytest.mark.parametrize("T", [1, 5, 16])
def test_selection_inputs_select(T):
    """the exact-selection inputs of the GPU file: the winning logit leads by > 100 in every (row, head) (e^-100: the softmax is one-hot to 4e-44, so the attention
    output is the winner's bf16 value in ANY arithmetic), logits stay small (|.| < 256: fp32 keeps 1e-5 of them), winners as drawn and spread over all tokens,
    rows and heads; D1 and D2 then equal D exactly."""
    P, N = 2, 200
    d, win = R.i2t_selection_case(P, N, T)
    D, D1, D2 = (R.i2t(*R.i2t_args(d, r)) for r in (R.ident, R.bf1, R.bf2))
    if T > 1:
        lead, top, idx = R.selection_margin(d)
        print(f"T={T}: smallest lead {lead:.2f}, largest logit {top:.2f}")
        assert lead > 100.0 and abs(top) < 256.0
        assert torch.equal(idx, win) and len(torch.unique(win)) == T
        assert all(len(torch.unique(win[p, n])) > 1 for p in range(P) for n in range(0, N, 37))       # heads of a row differ
        if T < 16:
            assert top < -50.0             # an unmasked token >= T (zero key: logit 0) would win every softmax
    assert float((D1 - D).abs().max()) <= 1e-12 and float((D2 - D).abs().max()) <= 1e-12
