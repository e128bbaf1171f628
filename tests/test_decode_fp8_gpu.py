"""Weight-only fp8 (OCP e4m3, one power-of-two scale per output channel) for the LLM's decode steps, on the GPU: the quantiser against its
definition bit for bit, each e4m3-weight decode kernel against float64 and against the bf16 kernel on the dequantised weights, the model-level
definition ("the bf16 decode run on W' = dequant(quant(W))") at the 7B shape, accuracy against the reference (printed), and the switch's hygiene.

The bounds of the kernel tests are those tests/test_kernels_gpu.py uses for the bf16 forms (same `err`, same shapes): 2e-3 for fp32 outputs,
2e-2 / 3e-2 for bf16 outputs -- the arithmetic is the same fp32 accumulation of exact bf16 x bf16 products."""
import math

import numpy as np
import pytest
import torch

from tests import util as U
from tests.test_decode_fp8_cpu import dequant_ref, quant_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def T(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype).contiguous()


def NP(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as o
    return o


def _quant(ops, w):
    """-> (e4m3 bytes, scales, W' = q * scale as bf16 -- exact --, W' as float64 on the GPU)"""
    q, sc = ops.rows_fp8_pow2(w)
    wd = q.view(torch.float8_e4m3fn).float() * sc[:, None]
    assert torch.equal(wd.to(torch.bfloat16).float(), wd)
    return q, sc, wd.to(torch.bfloat16).contiguous(), wd.double()


def _same(tag, a, b):
    same = torch.equal(a, b)
    print(f"    {tag}: {'bit-equal to' if same else 'NOT bit-equal to (max |d| %.3e)' % float((a.double() - b.double()).abs().max())} the bf16 kernel on the dequantised weights")
    return same


# ---- 1. the quantiser against its definition ------------------------------------------------------------------------------------------
def _quantiser_cases():
    g = torch.Generator().manual_seed(11)
    a = (torch.randn(517, 4096, generator=g) * 0.02).to(torch.bfloat16)
    a[0] = 0                                   # an all-zero row
    a[1, 77] = 448.0 * 2.0 ** -3               # amax an exact power of two times 448
    a[2, 9] = -448.0 * 2.0 ** -7
    a[3, 4000] = 1000.0                        # one outlier
    a[4] *= 2.0 ** -100                        # tiny rows
    a[5] *= 2.0 ** 60
    b = (torch.randn(92553, 256, generator=g) * 0.02).to(torch.bfloat16)       # N a multiple of nothing
    c = (torch.randn(33, 14336, generator=g) * 0.01).to(torch.bfloat16)        # w2's row length
    return {"517x4096": a, "92553x256": b, "33x14336": c}


def test_quantiser_equals_its_definition_bit_for_bit(ops):
    for tag, w in _quantiser_cases().items():
        q_ref, sc_ref = quant_ref(w)
        q, sc = ops.rows_fp8_pow2(w.to(DEV))
        torch.cuda.synchronize()
        q, sc = q.cpu(), sc.cpu()
        assert torch.equal(sc, sc_ref), (tag, int((sc != sc_ref).sum()))
        assert torch.equal(q, q_ref), (tag, int((q != q_ref).sum()))
        f, _ = torch.frexp(sc)
        assert bool((f == 0.5).all()), tag                                     # every scale a power of two
        amax = w.float().abs().amax(1)
        nz = amax > 0
        assert bool((amax[nz] / sc[nz] <= 448).all()) and bool((amax[nz] / (sc[nz] / 2) > 448).all()), tag     # ... and the smallest that fits
        wd = dequant_ref(q, sc)
        assert torch.equal(wd.to(torch.bfloat16).float(), wd), tag             # q * scale survives bf16 unchanged
        q2, sc2 = ops.rows_fp8_pow2(wd.to(torch.bfloat16).to(DEV))             # a fixed point: the scale may halve (largest code exactly 224), the values may not move
        assert torch.equal(dequant_ref(q2, sc2), wd), tag
        assert bool(((sc2.cpu() == sc) | (sc2.cpu() * 2 == sc)).all()), tag
        if tag == "517x4096":
            assert float(sc[0]) == 1.0 and int(q[0].max()) == 0 and float(sc[1]) == 2.0 ** -3 and int(q[1, 77]) == 0x7E and int(q[2, 9]) == 0xFE
    # fp32 rows take the same rule
    w32 = _quantiser_cases()["517x4096"].float() * 1.2345
    q_ref, sc_ref = quant_ref(w32)
    q, sc = ops.rows_fp8_pow2(w32.to(DEV))
    assert torch.equal(sc.cpu(), sc_ref) and torch.equal(q.cpu(), q_ref)


def test_entries_return_errors_for_shapes_they_do_not_take(ops):
    from ullsam_amd import _lib
    w = torch.zeros((64, 1000), dtype=torch.bfloat16, device=DEV)
    q, sc = ops.rows_fp8_pow2(w)
    with pytest.raises(_lib.UllsamError):      # K % 512
        ops.gemm_w8(torch.zeros((2, 1000), dtype=torch.bfloat16, device=DEV), q, sc)
    w = torch.zeros((64, 1024), dtype=torch.bfloat16, device=DEV)
    q, sc = ops.rows_fp8_pow2(w)
    with pytest.raises(_lib.UllsamError):      # M > 8
        ops.gemm_w8(torch.zeros((9, 1024), dtype=torch.bfloat16, device=DEV), q, sc)
    with pytest.raises(_lib.UllsamError):      # the prologue needs K % 2048 == 0
        ops.gemm_w8(torch.zeros((2, 1024), dtype=torch.float32, device=DEV), q, sc, norm_w=torch.ones(1024, device=DEV), eps=1e-5)
    with pytest.raises(TypeError):
        ops.gemm_w8(torch.zeros((2, 1024), dtype=torch.bfloat16, device=DEV), w, sc)
    torch.cuda.synchronize()


# ---- 2. each kernel against float64 and against the bf16 kernel on W' -----------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
def test_gemm_w8_decode_rows(ops, M):
    """The shapes of test_gemm_decode_rows (narrow k-split, ragged N, k-split at K = 14336, the plain kernel, SwiGLU through the persistent kernel) + the LM head's
    92553 rows: plain, bias + GELU, fp32 residual in place, SwiGLU on packed w13."""
    from ullsam_amd.packing import pack_w13
    rng = np.random.default_rng(M)
    shapes = [(4096, 4096), (1003, 512), (2048, 14336 if M <= 4 else 1536), (17923, 1024), (18432, 2048)] + ([(92553, 4096)] if M <= 4 else [])
    all_same = True
    for N, K in shapes:
        print(f"  M={M} N={N} K={K}")
        a = T(rng.standard_normal((M, K), dtype=np.float32), torch.bfloat16)
        w = T((rng.standard_normal((N, K), dtype=np.float32) / math.sqrt(K)).astype(np.float32), torch.bfloat16)
        w[min(7, N - 1)] *= 1.0 / 37.0        # rows of very different scales next to each other
        bias, res = T(rng.standard_normal(N, dtype=np.float32)), T(rng.standard_normal((M, N), dtype=np.float32))
        q, sc, wd, wd64 = _quant(ops, w)
        ref = NP(a.double() @ wd64.T)
        y = ops.gemm_w8(a, q, sc, out_f32=True)
        assert err(NP(y), ref) < 2e-3
        yb = ops.gemm(a, wd, out_f32=True)
        assert err(NP(y), NP(yb)) < 2e-3
        all_same &= _same("plain", y, yb)
        y = ops.gemm_w8(a, q, sc, bias=bias, act=ops.ACT_GELU)
        from oracle import ullsam_oracle as O
        assert err(NP(y), O.gelu(ref + NP(bias))) < 2e-2
        yb = ops.gemm(a, wd, bias=bias, act=ops.ACT_GELU)
        assert err(NP(y), NP(yb)) < 2e-2
        all_same &= _same("bias + GELU", y, yb)
        y, yb = res.clone(), res.clone()
        ops.gemm_w8(a, q, sc, bias=bias, residual=y, out_f32=True, out=y)
        ops.gemm(a, wd, bias=bias, residual=yb, out_f32=True, out=yb)
        assert err(NP(y), ref + NP(bias) + NP(res)) < 2e-3 and err(NP(y), NP(yb)) < 2e-3
        all_same &= _same("bias + residual in place", y, yb)
        if N % 256 == 0:
            h = N // 2
            w13 = pack_w13(w[:h].contiguous(), w[h:].contiguous())
            q13, s13, wd13, wd13_64 = _quant(ops, w13)            # quantised AFTER packing: gate and up rows keep their own scales
            s = ops.gemm_w8(a, q13, s13, act=ops.ACT_SWIGLU, out_f32=True)
            g, u = ref[:, :h], ref[:, h:]
            assert err(NP(s), g / (1 + np.exp(-g)) * u) < 2e-3
            sb = ops.gemm(a, wd13, act=ops.ACT_SWIGLU, out_f32=True)
            assert err(NP(s), NP(sb)) < 2e-3
            all_same &= _same("SwiGLU", s, sb)
    print(f"  M={M}: every result bit-equal to the bf16 kernel's: {all_same}")


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [2048, 4096])
def test_gemm_w8_with_rmsnorm_prologue(ops, M, K):
    """The RMSNorm prologue in front of e4m3 weights: packed w13 with SwiGLU (K = 4096: the persistent kernel), a narrow plain matrix (k-split), a wide plain matrix and the
    LM head's 92553 rows behind the norm (the persistent kernel's general epilogue)."""
    from ullsam_amd.packing import pack_w13
    rng = np.random.default_rng(100 * M + K)
    x = T(rng.standard_normal((M, K), dtype=np.float32) * 3)
    nw = T(1 + 0.1 * rng.standard_normal(K, dtype=np.float32))
    F = 1024 if K == 2048 else 9216
    w13 = pack_w13(T(rng.standard_normal((F, K), dtype=np.float32) / math.sqrt(K), torch.bfloat16), T(rng.standard_normal((F, K), dtype=np.float32) / math.sqrt(K), torch.bfloat16))
    xn = ops.norm(x, nw, None, 1e-5, torch.bfloat16, rms=True)          # the staged row is the one ullsam_norm writes (test_decode_gemm_with_rmsnorm_prologue_equals_norm_then_gemm)
    q13, s13, wd13, wd13_64 = _quant(ops, w13)
    a = ops.gemm_w8(x, q13, s13, act=ops.ACT_SWIGLU, norm_w=nw, eps=1e-5)
    r = NP(xn.double() @ wd13_64.T).reshape(M, -1, 2, 64)
    g, u = r[:, :, 0].reshape(M, -1), r[:, :, 1].reshape(M, -1)
    assert err(NP(a), g / (1 + np.exp(-g)) * u) < 3e-2
    b = ops.gemm_rmsnorm(x, nw, 1e-5, wd13, act=ops.ACT_SWIGLU)
    assert err(NP(a), NP(b)) < 3e-2
    _same(f"M={M} K={K} norm + w13 + SwiGLU", a, b)
    for N in (1536,) + ((17412, 92553) if K == 4096 else ()):
        w = T(rng.standard_normal((N, K), dtype=np.float32) / math.sqrt(K), torch.bfloat16)
        q, sc, wd, wd64 = _quant(ops, w)
        a = ops.gemm_w8(x, q, sc, norm_w=nw, eps=1e-5)
        assert err(NP(a), NP(xn.double() @ wd64.T)) < 3e-2
        b = ops.gemm_rmsnorm(x, nw, 1e-5, wd)
        assert err(NP(a), NP(b)) < 3e-2
        _same(f"M={M} K={K} norm + plain N={N}", a, b)


@pytest.mark.parametrize("B,KVH,G,past", [(4, 8, 4, 1081), (1, 2, 4, 0), (3, 4, 2, 17), (2, 8, 4, 5)])
@pytest.mark.parametrize("normed", [False, True])
def test_decode_qkv_rope_w8(ops, B, KVH, G, past, normed):
    """wqkv on e4m3 weights + head split + RoPE + KV-cache append in one launch, against the exact rotation of the float64 products and against the bf16 launch on W'."""
    hd, K, cap = 128, 2048 if B != 2 else 4096, past + 8
    rng = np.random.default_rng(B * 100 + KVH)
    N = KVH * (G + 2) * hd
    x = T(rng.standard_normal((B, K), dtype=np.float32))
    nw = T(1 + 0.1 * rng.standard_normal(K, dtype=np.float32))
    w = T(rng.standard_normal((N, K), dtype=np.float32) / math.sqrt(K), torch.bfloat16)
    bias = T(0.1 * rng.standard_normal(N, dtype=np.float32))
    pos = T(rng.integers(0, past + 1, size=(B, 1)).astype(np.int32), torch.int32)
    inv = 1.0 / (10000.0 ** (np.arange(0, hd, 2, dtype=np.float32) / hd))
    fr = np.arange(past + 4, dtype=np.float32)[:, None] * inv[None]
    emb = np.concatenate([fr, fr], -1)
    cos, sin = T(np.cos(emb).astype(np.float32)), T(np.sin(emb).astype(np.float32))
    xn = ops.norm(x, nw, None, 1e-5, torch.bfloat16, rms=True) if normed else x.to(torch.bfloat16)
    q8, sc, wd, wd64 = _quant(ops, w)
    fill = lambda: (torch.full((B, KVH, cap, hd), 7.0, dtype=torch.bfloat16, device=DEV), torch.full((B, KVH, cap, hd), -3.0, dtype=torch.bfloat16, device=DEV))
    k0, v0 = fill()
    q0 = ops.decode_qkv_rope(x if normed else xn, nw if normed else None, 1e-5, wd, bias, k0, v0, pos, cos, sin, B, KVH, G, past)
    k1, v1 = fill()
    q1 = ops.decode_qkv_rope_w8(x if normed else xn, nw if normed else None, 1e-5, q8, sc, bias, k1, v1, pos, cos, sin, B, KVH, G, past)
    untouched = torch.ones(cap, dtype=torch.bool, device=DEV); untouched[past] = False
    assert bool((k1[:, :, untouched] == 7.0).all()) and bool((v1[:, :, untouched] == -3.0).all())
    qkv = (NP(xn.double() @ wd64.T) + NP(bias)).reshape(B, KVH, G + 2, hd)
    p = pos.cpu().numpy()[:, 0]
    c, s_ = np.cos(emb)[p][:, None, None, :], np.sin(emb)[p][:, None, None, :]
    rot = np.concatenate([-qkv[..., hd // 2:], qkv[..., :hd // 2]], -1)
    ro = qkv * c + rot * s_
    assert err(NP(q1).reshape(B, KVH, G, hd), ro[:, :, :G]) < 2e-2       # one rounding of the result
    assert err(NP(k1[:, :, past]), ro[:, :, G]) < 2e-2
    assert err(NP(v1[:, :, past]), qkv[:, :, G + 1]) < 2e-2
    assert err(NP(q1), NP(q0)) < 2e-2 and err(NP(k1), NP(k0)) < 2e-2 and err(NP(v1), NP(v0)) < 2e-2
    _same(f"B={B} normed={normed} q", q1, q0); _same("k", k1, k0); _same("v", v1, v0)


# ---- 5. switch hygiene ----------------------------------------------------------------------------------------------------------------
def _small_lm(seed=0):
    """Two layers at a shape the fused decode step takes (hidden 2048, head_dim 128) with a w2 the decode kernels take too (K = 1024)."""
    from ullsam_amd.modeling.configuration_internlm2 import InternLM2Config
    from ullsam_amd.modeling.modeling_internlm2 import InternLM2ForCausalLM
    cfg = InternLM2Config(vocab_size=3001, hidden_size=2048, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=4,
                          bias=False, max_position_embeddings=2048, rope_theta=10000.0, rms_norm_eps=1e-5)
    torch.manual_seed(seed)
    lm = InternLM2ForCausalLM(cfg)
    torch.nn.init.normal_(lm.model.tok_embeddings.weight, std=1.0)
    return lm.to(DEV).to(torch.bfloat16).eval()


def _steps(lm, ids, n=3):
    """Prefill + n decode steps through InternLM2ForCausalLM.forward -> (prefill logits of the last position, [n] decode logits)."""
    B, S = ids.shape
    cache = lm.model.new_cache(B, S + n + 1, ids.device)
    out = lm(input_ids=ids, past_key_values=cache, use_cache=True)
    pre = out.logits[:, -1].clone()
    rows = []
    for s in range(n):
        tok = torch.full((B, 1), 5 + s, device=ids.device, dtype=torch.long)
        rows.append(lm(input_ids=tok, past_key_values=cache, use_cache=True).logits[:, -1].clone())
    return pre, torch.stack(rows, 1)


def test_switch_off_makes_the_parent_calls_and_on_makes_the_w8_calls(monkeypatch):
    from ullsam_amd import _lib
    lm = _small_lm()
    ids = torch.randint(0, 3000, (2, 9), device=DEV)
    real, names = _lib.call, []
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def decode_step_calls():
        cache = lm.model.new_cache(2, 16, DEV)
        lm(input_ids=ids, past_key_values=cache, use_cache=True)
        del names[:]
        lm(input_ids=ids[:, :1].contiguous(), past_key_values=cache, use_cache=True)
        return list(names)

    assert lm.fp8_decode is False
    off = decode_step_calls()
    del lm.fp8_decode
    gone = decode_step_calls()
    assert off == gone and not any("w8" in n or "fp8" in n for n in off), off
    assert off.count("ullsam_decode_qkv_rope") == 2 and off.count("ullsam_gemm_rmsnorm") == 2 and off.count("ullsam_gemm") == 5
    lm.fp8_decode = True
    on = decode_step_calls()
    swap = {"ullsam_decode_qkv_rope": "ullsam_decode_qkv_rope_w8", "ullsam_gemm_rmsnorm": "ullsam_gemm_w8", "ullsam_gemm": "ullsam_gemm_w8"}
    assert [n for n in on if n != "ullsam_rows_fp8_pow2"] == [swap.get(n, n) for n in off], (on, off)     # same launches, e4m3 forms (+ the quantiser on first use)
    assert on.count("ullsam_rows_fp8_pow2") == 2 * 4 + 1
    again = decode_step_calls()
    assert "ullsam_rows_fp8_pow2" not in again                                                            # packs are cached
    # prefill never reads them
    del names[:]
    lm(input_ids=ids, use_cache=True)
    assert not any("w8" in n for n in names), names
    lm.model.fuse_decode = False                                                                          # the unfused decode path has no e4m3 form: bf16, silently
    assert not any("w8" in n for n in decode_step_calls())
    lm.model.fuse_decode = True


def test_fp32_model_ignores_the_switch():
    lm = _small_lm().float()
    ids = torch.randint(0, 3000, (2, 9), device=DEV)
    pre0, dec0 = _steps(lm, ids)
    lm.fp8_decode = True
    pre1, dec1 = _steps(lm, ids)
    assert torch.equal(pre0, pre1) and torch.equal(dec0, dec1)


def test_small_model_fp8_decode_is_the_bf16_decode_on_dequantised_weights(ops):
    """The model-level definition at a small shape (the 7B shape: test_decode_7b_fp8_model_level_definition): overwrite every LLM linear with W' = dequant(quant(W));
    then switch on and switch off compute the same function, and prefill is the same code."""
    lm = _small_lm(1)
    with torch.no_grad():
        for n_, p in lm.named_parameters():
            if p.dim() == 2 and "tok_embeddings" not in n_:
                q, sc = ops.rows_fp8_pow2(p.detach().contiguous())
                p.copy_((q.view(torch.float8_e4m3fn).float() * sc[:, None]).to(torch.bfloat16))
    ids = torch.randint(0, 3000, (4, 33), device=DEV)
    pre_b, dec_b = _steps(lm, ids, 6)
    lm.fp8_decode = True
    pre_a, dec_a = _steps(lm, ids, 6)
    assert torch.equal(pre_a, pre_b)
    d = (dec_a - dec_b).abs()
    print(f"small model, fp8 decode vs bf16 decode on W': bit-equal {torch.equal(dec_a, dec_b)}, max |d logit| {float(d.max()):.3e}")
    lm.fp8_decode = False
    lm.model.fuse_decode = False
    _, dec_u = _steps(lm, ids, 6)
    lm.model.fuse_decode = True
    du = (dec_u - dec_b).abs().mean((0, 2))
    assert bool((d.mean((0, 2)) <= du).all()), (d.mean((0, 2)), du)
    # generate: same ids either way
    g0 = lm.generate(input_ids=ids, max_new_tokens=8, eos_token_id=-1)
    lm.fp8_decode = True
    g1 = lm.generate(input_ids=ids, max_new_tokens=8, eos_token_id=-1)
    if torch.equal(dec_a, dec_b):
        assert torch.equal(g0, g1)


def test_packs_are_rebuilt_after_an_in_place_weight_update():
    from ullsam_amd.checkpoint import prepack
    lm = _small_lm(2)
    lm.fp8_decode = True
    assert prepack(lm, fp8_decode=True) - prepack(lm) == 2 * 4 + 1
    ids = torch.randint(0, 3000, (2, 17), device=DEV)
    _, dec0 = _steps(lm, ids)
    g0 = lm.generate(input_ids=ids, max_new_tokens=6, eos_token_id=-1)
    with torch.no_grad():     # an AdamW-style in-place step on one weight: decay, then the update
        w = lm.model.layers[1].attention.wo.weight
        torch.manual_seed(9)
        w.mul_(1 - 0.01).add_(torch.randn_like(w), alpha=0.05)
    _, dec1 = _steps(lm, ids)
    g1 = lm.generate(input_ids=ids, max_new_tokens=6, eos_token_id=-1)
    fresh = _small_lm(3)
    fresh.load_state_dict(lm.state_dict())
    fresh.fp8_decode = True
    _, dec2 = _steps(fresh, ids)
    g2 = fresh.generate(input_ids=ids, max_new_tokens=6, eos_token_id=-1)
    assert not torch.equal(dec0, dec1)            # the update is seen ...
    assert torch.equal(dec1, dec2) and torch.equal(g1, g2)     # ... and what is computed is what a fresh model computes from the same weights


# ---- 3 + 4. the model-level definition at the 7B shape, accuracy against the reference ---------------------------------------------------
def _prefill_logits(m, x, ids, mask):
    from ullsam_amd import ops
    lm = m.language_model
    B, S = ids.shape
    vit = m._mlp1_tokens(m.vision_model.forward_tokens(x), x.shape[0])
    rank, _ = ops.scan_image_tokens(ids.contiguous(), m.img_context_token_id)
    emb = ops.embed_tokens(lm.model.tok_embeddings.weight.detach(), ids.contiguous(), rank, vit).reshape(B, S, -1)
    mk = mask.long()
    pos = (mk.cumsum(-1) - 1).masked_fill(mk == 0, 1)
    cache = lm.model.new_cache(B, S + 2, ids.device)
    out = lm.model(inputs_embeds=emb, attention_mask=mk, position_ids=pos, past_key_values=cache, use_cache=True)
    return lm.lm_head(out.last_hidden_state[:, -1], prefill=True)     # what generate does with the prompt's last position


def test_decode_7b_fp8_model_level_definition():
    """The `decode_7b_forced.npz` protocol of tests/test_model_gpu.py (7B shape, batch 4, S = 1081, 16 teacher-forced steps per prompt = 64 steps, none skipped).
      P  = the fixture's bf16 weights W, switch on (the product configuration: prefill on W, decode on quant(W));
      A  = the LLM's linears and head overwritten with W' = dequant(quant(W)), switch on;   B = the same weights, switch off: the parent's code computing the same function.
    Asserted: prefill logits of A == B bit for bit; mean |logit A - logit B(fused)| <= d[step] = mean |logit B(fused) - logit B(unfused)| at every step (two decode
    implementations the parent ships: A makes no rounding B-fused does not make); top-1 of A == top-1 of B wherever B's top-2 margin exceeds 2 x dmax (their largest
    difference).  Printed, not bounded (item 4): mean |logits - the reference's fp32 logits| per step for P, A, B and the bf16 mode next to the reference's own autocast error,
    and the count of steps whose top-1 is the reference's.  Seeded random weights: the logits are nearly tied; real checkpoints are not available here."""
    import bench
    from tests.test_model_gpu import _fill_model_from_rule, _forced_decode, decode_7b_prompts
    from ullsam_amd import ops
    from ullsam_amd.utils.synthetic import microscopy_batch
    g = U.gold("decode_7b_forced")
    ids_np, mask_np = decode_7b_prompts()
    assert np.array_equal(ids_np, g["ids"]) and np.array_equal(mask_np, g["mask"])
    x_np, _ = microscopy_batch([int(s) for s in g["tile_seeds"]])
    ids, mask = torch.from_numpy(ids_np).to(DEV), torch.from_numpy(mask_np).to(DEV)
    forced = torch.from_numpy(g["forced_ids"]).to(DEV)
    B, n = g["forced_ids"].shape
    ref_s, top1, acm = g["logits_sample"].astype(np.float64), g["top1_ids"], g["ac_mean_err"].astype(np.float64)
    m = _fill_model_from_rule(bench.build_model("h", "7b", torch.bfloat16, DEV, init=False), int(g["weight_seed"]))   # (the filler's fp32 values rounded to bf16 once, as .to(bfloat16) of an fp32 model does)
    lm = m.language_model
    x = torch.from_numpy(x_np).to(DEV).bfloat16()

    def run(fp8, fuse=True):
        lm.fp8_decode, lm.model.fuse_decode = fp8, fuse
        try:
            return _forced_decode(m, x, ids, mask, forced)
        finally:
            lm.fp8_decode, lm.model.fuse_decode = False, True

    def vs_ref(lg):
        return np.abs(lg[:, :, ::97].double().cpu().numpy() - ref_s).mean(-1), int((lg.argmax(-1).cpu().numpy() == top1).sum())

    lg16, lgP = run(False), run(True)
    assert not torch.equal(lg16, lgP)                       # the switch is on: the decode steps read other weights
    with torch.no_grad():
        for n_, p in lm.named_parameters():
            if p.dim() == 2 and "tok_embeddings" not in n_:
                q, sc = ops.rows_fp8_pow2(p.detach().contiguous())
                wd = q.view(torch.float8_e4m3fn).float() * sc[:, None]
                assert torch.equal(wd.to(torch.bfloat16).float(), wd)
                p.copy_(wd.to(torch.bfloat16))
                del q, sc, wd
    lgB, lgBu, lgA = run(False), run(False, fuse=False), run(True)
    lm.fp8_decode = True
    preA = _prefill_logits(m, x, ids, mask)
    lm.fp8_decode = False
    preB = _prefill_logits(m, x, ids, mask)
    assert torch.equal(preA, preB)
    d = (lgBu - lgB).abs()
    dstep, dmax = d.mean(-1).cpu().numpy(), float(d.max())
    dA = (lgA - lgB).abs().mean(-1).cpu().numpy()
    print(f"\nA (fp8 decode on W') against B (bf16 decode on W', fused): bit-equal {torch.equal(lgA, lgB)}; mean |d logit| per step {float(dA.min()):.3e} .. {float(dA.max()):.3e}; "
          f"yardstick B fused vs B unfused: mean per step {float(dstep.min()):.3e} .. {float(dstep.max()):.3e}, largest {dmax:.4f}")
    for b in range(B):
        print(f"  prompt {b}: A-B per step " + " ".join(f"{v:.1e}" for v in dA[b]) + "\n            d[step]    " + " ".join(f"{v:.1e}" for v in dstep[b]))
    eP, tP = vs_ref(lgP); eA, tA = vs_ref(lgA); eB, tB = vs_ref(lgB); e16, t16 = vs_ref(lg16)
    print("mean |logits - the reference's fp32 logits| per step (min .. max over the 64 steps; mean), and steps whose top-1 is the reference's fp32 top-1:")
    for tag, e, t in (("bf16 mode (switch off, W)", e16, t16), ("P: prefill W, decode quant(W)", eP, tP), ("A: fp8 decode on W'", eA, tA), ("B: bf16 decode on W'", eB, tB)):
        print(f"  {tag:32s} {float(e.min()):.4f} .. {float(e.max()):.4f}; mean {float(e.mean()):.4f} = {float(e.mean() / acm.mean()):.2f} x the reference's autocast error; top-1 {t} of {B * n}")
    print(f"  the reference's own autocast: {float(acm.min()):.4f} .. {float(acm.max()):.4f}; mean {float(acm.mean()):.4f}; top-1 {int((g['ac_top1_ids'] == top1).sum())} of {B * n}")
    assert (dA <= dstep).all(), float((dA - dstep).max())
    assert (np.abs(eA - eB) <= dstep).all()
    top2 = lgB.topk(2, -1).values
    marginB = (top2[..., 0] - top2[..., 1]).cpu().numpy()
    argA, argB = lgA.argmax(-1).cpu().numpy(), lgB.argmax(-1).cpu().numpy()
    print(f"greedy ids: A == B at {int((argA == argB).sum())} of {B * n} steps; B's margin exceeds 2 x dmax at {int((marginB > 2 * dmax).sum())} steps")
    assert ((argA == argB) | (marginB <= 2 * dmax)).all()
