"""Training the language model itself: the caption trainer's SFT stage (train.py:284-318 with --freeze_vision only, train.py:400-480) and the joint
trainer's --trainable_modules language_model (train_joint_v2.py:1334-1351).  Gradients of the token embeddings, every decoder layer, the final norm and the
LM head against the reference's own autograd (tests/golden/train_sft_step*.npz, train_step_llm.npz, made by tools/gen_golden_train_llm.py), and the two
kernels behind them (ullsam_train_embedding_bwd, ullsam_train_cross_entropy_bwd_bf16) against their definitions."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import util as U

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLM_LINEARS = ("attention.wqkv", "attention.wo", "feed_forward.w1", "feed_forward.w3", "feed_forward.w2")


def _t(a):
    return torch.from_numpy(a).to(DEV)


def _sft_model(dtype, real=False):
    if real:
        from tests.test_train_gpu import _ullsam_real_dims
        m = _ullsam_real_dims(dtype)
    else:
        from tests.test_model_gpu import _ullsam_tiny
        m = _ullsam_tiny(dtype)
    for n, p in m.named_parameters():
        p.requires_grad_(not n.startswith("vision_model."))                  # --freeze_vision (train.py:400-480)
    return m


def _sft_step(m, g, dtype):
    """train.py:284-318 (accumulation_steps = 1): model.train(); outputs = model(...labels...); outputs.loss.backward()."""
    x = _t(U.rand_image((1, 3, 1024, 1024), seed=int(g["image_seed"]))).to(dtype)
    ids = _t(g["ids"]).long()
    m.train()
    out = m(pixel_values=x, input_ids=ids, attention_mask=_t(g["attention_mask"]).long(), image_flags=(ids == 92546)[..., None].long(),
            labels=_t(g["labels"]).long(), return_dict=True, use_cache=False)
    loss = out.loss / 1
    loss.backward()
    torch.cuda.synchronize()
    return loss


def _check_against_reference(m, g, tol=1e-3, none_or_zero=()):
    params = dict(m.named_parameters())
    names = [str(v) for v in g["names"]]
    worst = (0.0, "")
    for n in names:
        assert params[n].grad is not None, n
        ref = g["g:" + n].astype(np.float64)
        full = params[n].grad.float().cpu().numpy().reshape(-1).astype(np.float64)
        got = full[::max(1, full.size // 512)]
        scale, diff = np.abs(ref).max(), np.abs(got - ref).max()
        assert diff < tol * scale + 1e-7, (n, diff, scale)
        if scale > 1e-6:
            worst = max(worst, (diff / scale, n))
        nref = float(g["n:" + n])
        assert abs(np.sqrt((full ** 2).sum()) - nref) < tol * nref + 1e-6, (n, np.sqrt((full ** 2).sum()), nref)
    for n in g["no_grad_names"]:
        p = params[str(n)]
        if str(n).startswith(none_or_zero):      # (the prompt encoder's point-embedding table is one Function input: its unused rows get zeros, not None)
            assert p.grad is None or not bool(p.grad.any()), n
        else:
            assert p.grad is None, n
    emb = params["language_model.model.tok_embeddings.weight"].grad
    for rid, ref in zip(g["row_ids"], g["emb_rows"]):
        got = emb[int(rid)].float().cpu().numpy()
        if not ref.any():
            assert not got.any(), (int(rid), float(np.abs(got).max()))          # padding id, <IMG_CONTEXT>, an id that does not occur: exactly zero
        else:
            assert np.abs(got - ref).max() < tol * np.abs(ref).max(), int(rid)
    return names, worst


def _llm_grads_all_present(m):
    lm = {n: p for n, p in m.named_parameters() if n.startswith("language_model.")}
    for n, p in lm.items():
        assert p.grad is not None and p.grad.dtype == p.dtype, n
    for part in LLM_LINEARS + ("attention_norm", "ffn_norm"):
        assert any(part in n and float(p.grad.abs().max()) > 0 for n, p in lm.items()), part
    assert float(lm["language_model.model.norm.weight"].grad.abs().max()) > 0
    assert float(lm["language_model.output.weight"].grad.abs().max()) > 0


@pytest.mark.gpu
def test_sft_step_gradients_equal_the_reference_autograd():
    """The SFT step on the tiny composite, fp32 (fixture train_sft_step.npz): the loss within 1e-5 relative; the gradient of every trainable parameter
    (mlp1, token embeddings, both decoder layers, final norm, LM head) within 1e-3 of its tensor's largest entry and its norm within 1e-3; the stored
    embedding rows the reference leaves at zero (padding id 0, <IMG_CONTEXT>, an absent id) are exactly zero; mlp2 / prompt encoder / mask decoder get none."""
    g = U.gold("train_sft_step")
    m = _sft_model(torch.float32)
    loss = _sft_step(m, g, torch.float32)
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    names, worst = _check_against_reference(m, g)
    assert {n.split(".")[0] for n in names} == {"mlp1", "language_model"}
    assert {str(n).split(".")[0] for n in g["no_grad_names"]} == {"mlp2", "prompt_encoder", "mask_decoder"}
    _llm_grads_all_present(m)
    print(len(names), "gradients; worst relative error", worst)


def _graph_nodes(loss):
    seen, stack, kinds = set(), [loss.grad_fn], []
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        kinds.append(f)
        stack.extend(nf for nf, _ in f.next_functions)
    return kinds


@pytest.mark.gpu
def test_sft_step_of_a_bf16_model_runs_the_llm_on_bf16_gemms():
    """bf16 model, SFT step: the bf16-GEMM route (training.BF16_LINEAR) against the fp32-arithmetic route on the same bf16 weights, with the bounds of
    test_bf16_model_runs_its_large_linears_on_bf16_gemms; the graph shows the head (LMLossFn on its bf16 route), the token embeddings (EmbeddingFn) and the
    layer linears (LinearBf16Fn, no FrozenLinearBf16Fn) as trainable nodes."""
    from ullsam_amd import training
    g = U.gold("train_sft_step")
    res = []
    old = training.BF16_LINEAR
    try:
        for on in (True, False):
            training.BF16_LINEAR = on
            m = _sft_model(torch.bfloat16)
            x = _t(U.rand_image((1, 3, 1024, 1024), seed=int(g["image_seed"]))).to(torch.bfloat16)
            ids = _t(g["ids"]).long()
            m.train()
            loss = m(pixel_values=x, input_ids=ids, attention_mask=_t(g["attention_mask"]).long(), labels=_t(g["labels"]).long(), return_dict=True,
                     use_cache=False).loss
            if on:
                nodes = _graph_nodes(loss)
                kinds = [type(f).__name__ for f in nodes]
                head = [f for f in nodes if "LMLossFn" in type(f).__name__]
                assert len(head) == 1 and head[0].train_w and head[0].bf16_w
                assert sum("EmbeddingFn" in k for k in kinds) == 1
                assert sum("LinearBf16Fn" in k and "Frozen" not in k for k in kinds) >= 2 * len(LLM_LINEARS) + 2, kinds
                assert not any("FrozenLinearBf16Fn" in k for k in kinds)
            loss.backward()
            torch.cuda.synchronize()
            _llm_grads_all_present(m)
            res.append((float(loss.detach()), {n: p.grad.float() for n, p in m.named_parameters() if p.grad is not None}))
            del m
    finally:
        training.BF16_LINEAR = old
    (lb, gb), (lf, gf) = res
    assert abs(lb - lf) < 2e-3 * abs(lf), (lb, lf)
    assert set(gb) == set(gf)
    worst, worst_cos = (0.0, ""), (1.0, "")
    for n in gf:
        scale = float(gf[n].abs().max())
        if scale < 1e-6:
            continue
        e = float((gb[n] - gf[n]).abs().max()) / scale
        cos = float((gb[n] * gf[n]).sum() / (gb[n].norm() * gf[n].norm()))
        worst, worst_cos = max(worst, (e, n)), min(worst_cos, (cos, n))
        assert e < 0.25 and cos > 0.995, (n, e, cos)
    print("SFT bf16-GEMM route vs fp32-arithmetic route: loss", lb, lf, "worst relative difference", worst, "worst cosine", worst_cos)


@pytest.mark.gpu
def test_segmentation_step_with_every_module_trainable_equals_the_reference():
    """train_joint_v2.py's segmentation step with --trainable_modules vision_model mlp1 language_model mlp2 prompt_encoder mask_decoder (fixture
    train_step_llm.npz): loss = 0 * outputs.loss + seg_loss; the LLM's gradients come from the segmentation loss alone, within 1e-3, and the LM head's
    gradient is a tensor of zeros (not None), as the reference's autograd leaves it."""
    import torch.nn.functional as F
    from tests.test_model_gpu import _ullsam_tiny
    from tests.test_train_gpu import _trainer_losses
    g = U.gold("train_step_llm")
    m = _ullsam_tiny(torch.float32)
    for p in m.parameters():
        p.requires_grad_(True)
    x = _t(U.rand_image((1, 3, 1024, 1024), seed=int(g["seed"])))
    ids = _t(g["ids"]).long()
    points, point_labels = _t(g["pts"]), _t(g["lbl"])
    yy, xx = np.mgrid[0:1024, 0:1024].astype(np.float32)
    masks = _t(np.stack([((xx - 300) ** 2 + (yy - 340) ** 2 < 150 ** 2), ((xx - 700) ** 2 + (yy - 610) ** 2 < 220 ** 2)]).astype(np.float32)[:, None])
    m.train()
    outputs = m(pixel_values=x, input_ids=ids, attention_mask=torch.ones_like(ids), image_flags=(ids == 92546)[..., None].long(), labels=_t(g["labels"]).long(),
                return_dict=True, use_cache=False, output_hidden_states=True)
    assert abs(outputs.loss.item() - float(g["lm_loss"])) < 1e-5 * float(g["lm_loss"])
    image_embeddings = m.vision_model(x)
    sparse, dense = m.prompt_encoder(points=(points, point_labels), boxes=None, masks=None, llm_hidden_states=outputs.hidden_states.repeat(points.shape[0], 1, 1, 1))
    low, _ = m.mask_decoder(image_embeddings=image_embeddings, image_pe=m.prompt_encoder.get_dense_pe(), sparse_prompt_embeddings=sparse,
                            dense_prompt_embeddings=dense, multimask_output=False)
    seg, _, _ = _trainer_losses(F.interpolate(low, (1024, 1024), mode="bilinear", align_corners=False), masks)
    loss = 0 * outputs.loss + seg
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(g["loss"])) < 2e-5 * float(g["loss"]), (loss.item(), float(g["loss"]))
    names, worst = _check_against_reference(m, g, none_or_zero=("prompt_encoder.point_embeddings.",))
    assert {n.split(".")[0] for n in names} == {"vision_model", "mlp1", "language_model", "mlp2", "prompt_encoder", "mask_decoder"}
    hg = m.language_model.output.weight.grad
    assert hg is not None and hg.shape == m.language_model.output.weight.shape and float(hg.abs().max()) == 0.0
    assert float(m.language_model.model.tok_embeddings.weight.grad.abs().max()) > 0
    print(len(names), "gradients; worst relative error", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sft_step_at_real_llm_geometry(dtype):
    """The SFT step with one 7B-shaped InternLM2 layer (hidden 4096, 32 / 8 heads, vocab 92553; S = 1081, so the head sees 1080 rows, not a multiple of 64)
    behind the ViT-B-width SAM (fixture train_sft_step_real.npz).  fp32: the loss within 5e-5, every gradient within 1e-3 of its tensor's largest entry.
    bf16 model (bf16 GEMMs with fp32 accumulation, bf16 gradients): the loss within 1e-2 and every gradient's direction (cosine > 0.99) and norm (2 %)."""
    g = U.gold("train_sft_step_real")
    m = _sft_model(dtype, real=True)
    torch.cuda.synchronize(); t0 = __import__("time").perf_counter()
    loss = _sft_step(m, g, dtype)
    print(f"SFT step at real LLM geometry ({dtype}): {__import__('time').perf_counter() - t0:.3f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    ref_loss = float(g["loss"])
    if dtype == torch.float32:
        assert abs(loss.item() - ref_loss) < 5e-5 * abs(ref_loss), (loss.item(), ref_loss)
        _check_against_reference(m, g)
        _llm_grads_all_present(m)
        return
    assert abs(loss.item() - ref_loss) < 1e-2 * abs(ref_loss), (loss.item(), ref_loss)
    params = dict(m.named_parameters())
    worst = (1.0, "")
    for n in [str(v) for v in g["names"]]:
        full = params[n].grad.float().cpu().numpy().reshape(-1).astype(np.float64)
        ref = g["g:" + n].astype(np.float64)
        got = full[::max(1, full.size // 512)]
        nref = float(g["n:" + n])
        assert abs(np.sqrt((full ** 2).sum()) - nref) < 2e-2 * nref + 1e-6, (n, np.sqrt((full ** 2).sum()), nref)
        if np.abs(ref).max() > 0:
            cos = float((got * ref).sum() / (np.linalg.norm(got) * np.linalg.norm(ref) + 1e-30))
            worst = min(worst, (cos, n))
            assert cos > 0.99, (n, cos)
    for n in g["no_grad_names"]:
        assert params[str(n)].grad is None, n
    emb = params["language_model.model.tok_embeddings.weight"].grad
    for rid, ref in zip(g["row_ids"], g["emb_rows"]):
        if not ref.any():
            assert float(emb[int(rid)].abs().max()) == 0.0, int(rid)
    print("bf16 SFT step at real geometry: worst cosine", worst)


def _embedding_bwd(dy, ids, skip, V, padding_idx, dtype):
    from ullsam_amd import _lib
    from ullsam_amd.training import _s
    R, D = dy.shape
    sid, order = torch.sort(ids.to(torch.int32), stable=True)
    order = order.to(torch.int32)
    out = torch.full((V, D), float("nan"), dtype=dtype, device=DEV)                         # every row must be written
    _lib.call("ullsam_train_embedding_bwd", dy.data_ptr(), D, sid.data_ptr(), order.data_ptr(), 0 if skip is None else skip.data_ptr(), R, D, V, padding_idx,
              out.data_ptr(), 1 if dtype == torch.bfloat16 else 0, _s())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("D", [256, 2048, 4096, 6144])
def test_embedding_backward_kernel_against_a_float64_index_add(D):
    """ullsam_train_embedding_bwd against numpy's float64 index-add: duplicates (one id 600 times), ids 0 and V - 1, the padding id skipped, masked rows
    skipped, every other row exactly zero; bf16 output = the fp32 output rounded; two launches bit-equal."""
    V, R = 92553, 1100
    rng = np.random.default_rng(D)
    ids = rng.integers(0, V, R)
    ids[rng.choice(R, 600, replace=False)] = 4242
    ids[[3, 700]] = 0
    ids[[5, 900, 901]] = V - 1
    ids[[10, 11]] = 77
    skip = np.zeros(R, np.int32)
    skip[rng.choice(R, 150, replace=False)] = 1
    skip[[10, 11]] = 1                                                                        # id 77: every row masked -> zero
    skip[[5, 3]] = 0
    dy = rng.standard_normal((R, D)).astype(np.float32)
    pad = 0
    ref = {}
    for r in range(R):
        if ids[r] == pad or skip[r]:
            continue
        ref.setdefault(int(ids[r]), np.zeros(D, np.float64))
        ref[int(ids[r])] += dy[r].astype(np.float64)
    dyt, idt, skt = _t(dy), _t(ids), _t(skip)
    out = _embedding_bwd(dyt, idt, skt, V, pad, torch.float32)
    out2 = _embedding_bwd(dyt, idt, skt, V, pad, torch.float32)
    outb = _embedding_bwd(dyt, idt, skt, V, pad, torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    assert torch.equal(outb, out.bfloat16())
    named = torch.tensor(sorted(ref), dtype=torch.long, device=DEV)
    got = out[named].double().cpu().numpy()
    want = np.stack([ref[k] for k in sorted(ref)])
    assert np.abs(got - want).max() < 1e-5 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    assert 4242 in ref and V - 1 in ref and 0 not in ref and 77 not in ref
    zero = torch.ones(V, dtype=torch.bool, device=DEV)
    zero[named] = False
    assert zero[0] and zero[77]
    assert int(torch.count_nonzero(out[zero])) == 0 and int(torch.count_nonzero(outb[zero])) == 0
    # no mask at all: only the padding id is skipped
    out3 = _embedding_bwd(dyt, idt, None, V, -1, torch.float32)
    r0 = dy[ids == 0].astype(np.float64).sum(0)
    assert np.abs(out3[0].double().cpu().numpy() - r0).max() < 1e-5 * max(1.0, np.abs(r0).max())


@pytest.mark.gpu
@pytest.mark.parametrize("R,V", [(1080, 92553), (37, 1000)])
def test_cross_entropy_backward_bf16_layouts_equal_the_rounded_fp32_kernel(R, V):
    """ullsam_train_cross_entropy_bwd_bf16: every element of the row-major [R, Vp] and the transposed [Vp, Rp] output is the bf16 rounding of what
    ullsam_train_cross_entropy_bwd writes; the pads are zero; either layout may be skipped."""
    from ullsam_amd import _lib
    from ullsam_amd.training import _s
    Vp, Rp = -(-V // 64) * 64, -(-R // 64) * 64
    gen = torch.Generator(device=DEV); gen.manual_seed(R)
    logits = torch.randn((R, V), device=DEV, generator=gen) * 4.0
    labels = torch.randint(0, V, (R,), device=DEV, generator=gen)
    labels[::7] = -100
    lse, rows, out2 = torch.empty(R, device=DEV), torch.empty(R, device=DEV), torch.empty(2, device=DEV)
    _lib.call("ullsam_train_cross_entropy", logits.data_ptr(), V, labels.data_ptr(), lse.data_ptr(), rows.data_ptr(), out2.data_ptr(), R, V, _s())
    g = torch.full((1,), 0.75, device=DEV)
    ref = torch.empty((R, Vp), device=DEV)
    _lib.call("ullsam_train_cross_entropy_bwd", logits.data_ptr(), V, labels.data_ptr(), lse.data_ptr(), out2.data_ptr(), g.data_ptr(), ref.data_ptr(), Vp, R, V, _s())
    bf = torch.bfloat16

    def run(rm, tr):
        d = torch.full((R, Vp), float("nan"), dtype=bf, device=DEV) if rm else None
        dt = torch.full((Vp, Rp), float("nan"), dtype=bf, device=DEV) if tr else None
        _lib.call("ullsam_train_cross_entropy_bwd_bf16", logits.data_ptr(), V, labels.data_ptr(), lse.data_ptr(), out2.data_ptr(), g.data_ptr(),
                  0 if d is None else d.data_ptr(), Vp, 0 if dt is None else dt.data_ptr(), Rp, R, V, _s())
        return d, dt

    d, dt = run(True, True)
    torch.cuda.synchronize()
    want = ref.bfloat16()
    assert torch.equal(d, want)                                                              # columns V .. Vp - 1: the fp32 kernel's zeros, rounded
    assert int(torch.count_nonzero(d[:, V:])) == 0
    assert torch.equal(dt[:V, :R], want[:, :V].t())
    assert int(torch.count_nonzero(dt[V:])) == 0 and int(torch.count_nonzero(dt[:, R:])) == 0
    assert float(want.float().abs().max()) > 0
    d1, n1 = run(True, False)
    n2, dt2 = run(False, True)
    torch.cuda.synchronize()
    assert n1 is None and n2 is None and torch.equal(d1, d) and torch.equal(dt2, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_sft_steps_are_bit_equal(dtype):
    """The SFT step has no scheduling-dependent sum (the embedding gradient sums each id's rows in position order, the head's dlog is one pass): two runs
    give the same loss and the same bits in every gradient."""
    g = U.gold("train_sft_step")
    m = _sft_model(dtype)
    runs = []
    for _ in range(2):
        for p in m.parameters():
            p.grad = None
        loss = _sft_step(m, g, dtype)
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1)
    assert set(g0) == set(g1) and len(g0) >= 17
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_then_infer_matches_a_fresh_model_with_the_updated_weights(dtype):
    """Inference first (fills the inference path's weight packs), one SFT step and one torch.optim.AdamW step (in-place updates of every LLM weight), then
    eval() forward and greedy generate: logits and token ids bit-equal to a fresh model loaded with load_state_dict(model.state_dict()) -- the PackCache
    re-layouts (w13 ...), the W^T cache and the widened copies follow the optimizer's in-place updates."""
    from tests.test_model_gpu import _ullsam_tiny
    g = U.gold("train_sft_step")
    x = _t(U.rand_image((1, 3, 1024, 1024), seed=int(g["image_seed"]))).to(dtype)
    ids = _t(g["ids"]).long()[:, :1070]
    amask = torch.ones_like(ids)

    def infer(model):
        model.eval()
        with torch.no_grad():
            out = model(pixel_values=x, input_ids=ids, attention_mask=amask, return_dict=True, use_cache=False)
            logits = out.logits.float().clone()
            toks = model.generate(pixel_values=x, input_ids=ids, attention_mask=amask, max_new_tokens=6)
        torch.cuda.synchronize()
        return logits, toks.clone()

    m = _sft_model(dtype)
    before, _ = infer(m)
    _sft_step(m, g, dtype)
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.05)
    opt.step()
    torch.cuda.synchronize()
    after, toks = infer(m)
    assert not torch.equal(before, after)                                                    # the step moved the model
    fresh = _ullsam_tiny(dtype)
    fresh.load_state_dict(m.state_dict())
    ref, ref_toks = infer(fresh)
    assert torch.equal(after, ref), float((after - ref).abs().max())
    assert torch.equal(toks, ref_toks), (toks.tolist(), ref_toks.tolist())


def test_llm_training_kernels_compile_without_spills():
    """ullsam_train_embedding_bwd's two kernels and ullsam_train_cross_entropy_bwd_bf16's: no spilled register and no scratch, read from the built library."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels()
    found = {n: r for n, r in ks.items() if re.search(r"ce_bwd_bf16_kernel|embedding_bwd_kernel|zero_fill16_kernel", n)}
    assert len(found) == 10, sorted(found)                                                     # (embedding_bwd_kernel: fp32 / bf16 x four row widths)
    bad = {n: r for n, r in found.items() if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)}
    assert not bad, bad
