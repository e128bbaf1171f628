"""CPU half of the prefill attention tests: the float64 definitions of tests/attention_ref.py against the numpy oracle, the probe round trip,
what the bf16 format alone costs, the conditions every case of the tables must meet so that no bound is ever decided by a floor, the old
rel_h indexing of the global table pass shown wrong on paper, and the refusal of unaligned bases (made before any launch, so it is called
here with dummy addresses that are never dereferenced)."""
import math

import numpy as np
import pytest
import torch

from oracle import ullsam_oracle as O
from tests import attention_ref as R

ALL_CAUSAL = [(fam, name) for fam, cases in R.CAUSAL_FAMILIES.items() for name in cases]
ALL_VIT = [(fam, name) for fam, cases in R.VIT_FAMILIES.items() for name in cases]


# ---------------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("B,Sq,past,H,KVH,mask", [(2, 9, 0, 4, 2, ("left", 3)), (2, 7, 5, 2, 1, ("holes", [0, 6])), (1, 12, 0, 2, 2, ("tail", 4)),
                                                  (2, 5, 3, 4, 1, ("left", 5))])
def test_causal_ref_agrees_with_the_oracle(B, Sq, past, H, KVH, mask):
    hd, G, Sk = 16, H // KVH, past + Sq
    c = dict(Sq=Sq, q_pos0=past, B=B, H=H, KVH=KVH, mask=mask)
    t = R.build_causal(f"oracle{Sq}_{past}", c, torch.float32, hd)
    out, P, defined = R.causal_ref(t["q"], t["k"], t["v"], t["mask"], past)
    q = t["q"].numpy().transpose(0, 2, 1, 3)
    k, v = np.repeat(t["k"].numpy(), G, 1), np.repeat(t["v"].numpy(), G, 1)
    a = np.matmul(q, k.transpose(0, 1, 3, 2)) / np.float32(math.sqrt(hd)) + O.decoder_mask(t["mask"].numpy().astype(np.int64), Sq, past)
    Po = O.softmax(a.astype(np.float32))
    oo = np.matmul(Po, v).transpose(0, 2, 1, 3)
    # every row, the undefined ones too: the literal masks give the reference's uniform rows there
    assert np.abs(P.numpy() - Po).max() < 1e-6 and np.abs(out.numpy() - oo).max() < 1e-5
    ok = R.causal_unmasked(t["mask"], B, Sq, Sk, past)
    assert torch.equal(defined, ok.any(-1)) and bool(defined.all()) == (mask[0] != "left")
    assert bool((P.permute(0, 2, 1, 3)[defined][~ok[defined][:, None].expand(-1, H, -1)] == 0).all())          # masked keys of defined rows: exactly 0


@pytest.mark.parametrize("gh,gw,window,heads,hd", [(5, 5, 0, 2, 16), (4, 7, 0, 2, 16), (7, 3, 0, 1, 16), (10, 10, 7, 2, 16), (9, 5, 4, 2, 16), (3, 6, 4, 1, 16)])
def test_vit_ref_agrees_with_the_oracle(gh, gw, window, heads, hd):
    B, D = 2, heads * hd
    rng = np.random.default_rng(gh * 100 + gw)
    xn = rng.standard_normal((B, gh, gw, D), dtype=np.float32)
    nh_, nw_ = (window, window) if window > 0 else (gh, gw)
    P = {"qkv.weight": (rng.standard_normal((3 * D, D), dtype=np.float32) / math.sqrt(D)).astype(np.float32),
         "qkv.bias": rng.standard_normal(3 * D, dtype=np.float32) * 0.3,
         "rel_pos_h": rng.standard_normal((2 * nh_ - 1, hd), dtype=np.float32) * 0.1,
         "rel_pos_w": rng.standard_normal((2 * nw_ - 1, hd), dtype=np.float32) * 0.1,
         "proj.weight": np.eye(D, dtype=np.float32), "proj.bias": np.zeros(D, np.float32)}
    if window > 0:
        xw, pad_hw = O.window_partition(xn, window)
        ref = O.window_unpartition(O.vit_attention(xw, P, "", heads), window, pad_hw, (gh, gw))
    else:
        ref = O.vit_attention(xn, P, "", heads)
    qkv = O.linear(xn.reshape(-1, D), P["qkv.weight"], P["qkv.bias"])                       # the UNPADDED tokens
    out, Pm = R.vit_ref(torch.from_numpy(qkv), torch.from_numpy(P["rel_pos_h"]), torch.from_numpy(P["rel_pos_w"]), torch.from_numpy(P["qkv.bias"]),
                        B, heads, hd, gh, gw, window)
    assert np.abs(out.numpy().reshape(ref.shape) - ref).max() < 2e-6 * max(1.0, float(np.abs(ref).max()))
    assert float((Pm.sum(-1) - 1).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- probes
@pytest.mark.parametrize("n_keys,hd", [(1, 64), (64, 64), (65, 64), (196, 80), (197, 80), (390, 64), (1089, 80)])
def test_probe_and_recover_round_trip_exactly(n_keys, hd):
    g = torch.Generator(); g.manual_seed(n_keys)
    P = torch.softmax(torch.randn(7, n_keys, generator=g, dtype=torch.float64) * 3, -1)
    runs = R.n_runs(n_keys, hd)
    outs = [P @ R.probe_v(n_keys, hd, r, torch.float64) for r in range(runs)]               # an exact "kernel"
    assert all(o.shape == (7, hd) for o in outs) and runs <= R.MAX_RUNS
    assert torch.equal(R.recover_p(outs, n_keys), P)


@pytest.mark.parametrize("name", ["win14_29x29", "win14_16x30", "win8_9x17", "glob_8x9_hd64"])
def test_vit_probe_operands_round_trip_exactly(name):
    """The packed probe operands through the float64 definition give back its own probability matrix in the kernel's output layout: the live keys
    entry by entry, the pad keys as their sum."""
    c = next(cs[name] for cs in R.VIT_FAMILIES.values() if name in cs)
    t = R.build_vit(name, c, torch.float32)
    args = (c["B"], c["heads"], c["hd"], c["gh"], c["gw"], c["window"])
    _, P = R.vit_ref(t["qkv"], t["rel_h"], t["rel_w"], t["bias"], *args)
    tok = R.window_layout(c["gh"], c["gw"], c["window"])[0] if c["window"] else torch.arange(c["gh"] * c["gw"])[None]
    N = tok.shape[1]
    outs = []
    for run in range(R.vit_probe_runs(c)):
        qkv, bias = R.vit_probe_qkv(t["qkv"], t["bias"], c, run)
        outs.append(R.vit_ref(qkv, t["rel_h"], t["rel_w"], bias, *args)[0].reshape(c["B"], -1, c["heads"], c["hd"]))
    got = torch.cat(outs, -1)
    want = R.vit_token_p(P, tok, c["gh"], c["gw"])
    keys = R.vit_token_keys(tok, c["gh"], c["gw"])
    n = min(got.shape[-1], N + 1)
    keep = keys[None, :, None, :n].expand(c["B"], -1, c["heads"], -1)
    live_slots = keep.clone(); live_slots[..., N:] = False
    assert torch.equal(got[..., :n][live_slots], want[..., :n][live_slots])                  # a live key's entry comes back exactly
    assert float((got[..., :n] - want[..., :n]).abs()[keep].max()) < 1e-14                   # the pad slot is a sum taken in another order
    assert bool(keys[:, :N].any(-1).all()) and int(keys.sum()) == sum(int((tok[w] >= 0).sum()) * (int((tok[w] >= 0).sum()) + int((tok[w] < 0).any()))
                                                                       for w in range(tok.shape[0]))      # 100 % of the live entries + one pad slot
    assert float((want.sum(-1) - 1).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- conditions on the tables
def _check_logits(x, ok, what):
    """x [..., rows, keys] float64 logits, ok the same shape: True where the entry is compared."""
    big = torch.where(ok, x, torch.full_like(x, -math.inf))
    small = torch.where(ok, x, torch.full_like(x, math.inf))
    rows = ok.any(-1)
    assert bool(rows.any()), what
    assert float(x.abs()[ok].max()) < R.MAX_LOGIT, (what, float(x.abs()[ok].max()))
    span = (big.max(-1).values - small.min(-1).values)[rows]
    assert float(span.max()) <= R.MAX_SPAN, (what, float(span.max()))
    return span


@pytest.mark.parametrize("fam,name", ALL_CAUSAL)
@pytest.mark.parametrize("hd", [128, 64])
def test_causal_cases_meet_the_conditions_and_the_bf16_format_fits_the_bound(fam, name, hd):
    c = R.CAUSAL_FAMILIES[fam][name]
    t = R.build_causal(name, c, torch.bfloat16, hd)
    B, H, Sq, Sk, p0 = t["B"], t["H"], t["Sq"], t["Sk"], t["q_pos0"]
    out, P, defined = R.causal_ref(t["q"], t["k"], t["v"], t["mask"], p0)
    ok = R.causal_unmasked(t["mask"], B, Sq, Sk, p0)[:, None].expand(B, H, Sq, Sk)
    assert bool(defined.any(-1).all()), "a batch row without a defined query"
    assert torch.equal(defined[:, None].expand(B, H, Sq), ok.any(-1))
    assert R.n_runs(Sk, hd) <= R.MAX_RUNS
    G = H // t["KVH"]
    x = t["q"].double().permute(0, 2, 1, 3) @ t["k"].double().repeat_interleave(G, 1).transpose(-1, -2) / math.sqrt(hd)
    _check_logits(x, ok, name)
    assert float(P[ok].min()) >= R.MIN_P, float(P[ok].min())
    assert bool((P[~ok & ok.any(-1, keepdim=True)] == 0).all())
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    if c.get("logits") == "rising":                                                          # the maximum moves in every 32-key block of a late row
        assert bool((x[0, 0, -1].reshape(-1)[31::32].diff() > 0).all())
    if c.get("logits") == "falling":                                                         # and never after key 0
        assert bool((x[0, 0, -1] <= x[0, 0, -1, 0]).all())
    for Pm in R.bf16_model(torch.where(ok, x, torch.full_like(x, -math.inf))[ok.any(-1)]):
        e = R.rel_err(Pm, P[ok.any(-1)], ok[ok.any(-1)])
        assert e <= R.FORMAT_TOL, e


def _vit_case(fam, name):
    c = R.VIT_FAMILIES[fam][name]
    t = R.build_vit(name, c, torch.bfloat16)
    args = (c["B"], c["heads"], c["hd"], c["gh"], c["gw"], c["window"])
    return c, t, args


@pytest.mark.parametrize("fam,name", ALL_VIT)
def test_vit_cases_meet_the_conditions_and_the_bf16_format_fits_the_bound(fam, name):
    c, t, args = _vit_case(fam, name)
    x, _, tok = R.vit_logits(t["qkv"], t["rel_h"], t["rel_w"], t["bias"], *args)
    live_q = (tok >= 0)[None, :, None, :, None].expand_as(x)                                 # cropped query rows are not compared; every key is live
    span = _check_logits(x, live_q, name)
    P = torch.softmax(x, -1)
    assert float(P[live_q].min()) >= R.MIN_P
    assert R.vit_probe_runs(c) <= R.MAX_RUNS or (c["gh"], c["gw"]) == (64, 64) and c["window"] == 0 and c["hd"] >= 64   # 64 x 64 global: the two marginals
    if c["logits"] == "rel":                                                                 # the bias alone picks the key: the argmax without the q.k term
        xb = x - (R.vit_logits(t["qkv"], t["rel_h"] * 0, t["rel_w"] * 0, t["bias"], *args)[0])
        assert float((xb.argmax(-1) == x.argmax(-1)).double().mean()) > 0.5
    if c["logits"] == "bias":                                                                # pad tokens carry most of the weight where there are any
        padw = (tok < 0).any(-1)
        mass = (P * (tok < 0)[None, :, None, None, :]).sum(-1)[:, padw]
        assert float(mass.mean()) > 0.5
    rows = (tok >= 0)[None, :, None, :].expand(x.shape[:-1])
    if x.shape[-1] <= 1200:
        for Pm in R.bf16_model(x[rows]):
            e = R.rel_err(Pm, P[rows], torch.ones_like(P[rows], dtype=torch.bool))
            assert e <= R.FORMAT_TOL, e
    else:                                                                                    # 4096 keys: one head's rows are enough for the format
        for Pm in R.bf16_model(x[0, 0, 0]):
            e = R.rel_err(Pm, P[0, 0, 0], torch.ones_like(P[0, 0, 0], dtype=torch.bool))
            assert e <= R.FORMAT_TOL, e
    del span


# ---------------------------------------------------------------------------------------------------------------- the old indexing, on paper
@pytest.mark.parametrize("gh,gw", R.GLOBAL_NONSQUARE_GRIDS)
@pytest.mark.parametrize("hd", [64, 80])
def test_the_old_rel_h_indexing_fails_the_bound_on_non_square_grids(gh, gw, hd):
    """flash_attn_kernel's global table pass used 2*grid_w - 1 rows and the offset grid_w - 1 for BOTH tables.  Emulated in float64 (rows that do
    not exist or were never written counted as 0), every rel_h term is shifted by grid_w - grid_h and the probabilities leave the bound the GPU
    test sets -- shown here without launching that code on a grid where it read beyond rel_h.  On a square grid the old indexing is the new one."""
    name = f"glob_{gh}x{gw}_hd{hd}"
    c, t, args = _vit_case("global_small", name)
    _, P = R.vit_ref(t["qkv"], t["rel_h"], t["rel_w"], t["bias"], *args)
    _, Pold = R.vit_ref(t["qkv"], t["rel_h"], t["rel_w"], t["bias"], *args, parent_indexing=True)
    e = R.rel_err(Pold, P, torch.ones_like(P, dtype=torch.bool))
    print(f"{name}: old indexing, largest relative error of a probability {e:.3f}")
    assert e > 4 * R.BF16_TOL
    cs, ts, args_s = _vit_case("global_small", "glob_7x7_hd64")
    assert torch.equal(R.vit_ref(ts["qkv"], ts["rel_h"], ts["rel_w"], ts["bias"], *args_s)[1],
                       R.vit_ref(ts["qkv"], ts["rel_h"], ts["rel_w"], ts["bias"], *args_s, parent_indexing=True)[1])


# ---------------------------------------------------------------------------------------------------------------- the checks fire
def test_the_checks_fire_on_three_wrong_kernels():
    """Three wrong "kernels", built from the float64 definition: one drops a 32-key block for the late rows, one weights one masked key, one puts
    rel_h on the neighbouring key row.  The per-entry check of the probabilities, the exact zero of masked entries and the row-normalised output
    check do not let them through (the masked key's 2^-10 moves no output by more than 2^-10 max|V|, an eighth of the older tests' 4e-2: an absolute bound on outputs never sees it)."""
    name = "hole40"
    c = R.CAUSAL_MASKS[name]
    t = R.build_causal(name, c, torch.bfloat16, 128)
    B, H, Sq, Sk = t["B"], t["H"], t["Sq"], t["Sk"]
    out, P, defined = R.causal_ref(t["q"], t["k"], t["v"], t["mask"], 0)
    ok = R.causal_unmasked(t["mask"], B, Sq, Sk, 0)[:, None].expand(B, H, Sq, Sk)
    vf = t["v"].double().repeat_interleave(H // t["KVH"], 1)
    rows = defined[:, :, None].expand(B, Sq, H)
    R.check_entries(P, P, ok, R.BF16_TOL, "exact")                                           # the definition itself passes
    dropped = P.clone()
    dropped[:, :, 150:, 64:96] = 0                                                           # a 32-key block, for the late rows
    dropped = dropped / dropped.sum(-1, keepdim=True)
    o2 = (dropped @ vf).permute(0, 2, 1, 3)
    with pytest.raises(AssertionError):
        R.check_entries(dropped, P, ok, R.BF16_TOL, "dropped block")
    with pytest.raises(AssertionError):
        R.check_outputs(o2, out, rows, R.BF16_TOL, "dropped block")
    leaky = P.clone()
    leaky[-1, :, 100:, 40] = 2.0 ** -10                                                      # the padded key 40, seen by the rows behind it
    assert float(((leaky @ vf).permute(0, 2, 1, 3) - out).abs().max()) <= 2.0 ** -10 * float(vf.abs().max()) < 4e-2 / 8
    masked = defined[:, None, :, None].expand_as(ok) & ~ok
    assert bool((P[masked] == 0).all()) and not bool((leaky[masked] == 0).all())
    cv, tv, args = _vit_case("global_small", "glob_33x33_hd80")
    Pv = R.vit_ref(tv["qkv"], tv["rel_h"], tv["rel_w"], tv["bias"], *args)[1]
    shifted = torch.cat([tv["rel_h"][1:], tv["rel_h"][:1]])                                  # every rel_h term taken one key row off
    P3 = R.vit_ref(tv["qkv"], shifted, tv["rel_w"], tv["bias"], *args)[1]
    with pytest.raises(AssertionError):
        R.check_entries(P3, Pv, torch.ones_like(Pv, dtype=torch.bool), R.BF16_TOL, "shifted rel_h")


# ---------------------------------------------------------------------------------------------------------------- refusals, no launch
@pytest.fixture(scope="module")
def lib():
    from ullsam_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


BASE = 0x7F0000000000           # dummy addresses: the alignment check precedes the first HIP call of both entry points


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("off", [2, 4, 8])
def test_causal_attention_refuses_an_unaligned_base_before_any_launch(lib, dtype, which, off):
    """The LDS-DMA kernel used to fall back to the tiled kernel on such a base -- which reads q / k / v 16 bytes at a time itself."""
    from ullsam_amd import _lib
    ptrs = [BASE + 0x100000 * i + (off if i == which else 0) for i in range(4)]
    with pytest.raises(_lib.UllsamError, match="16-byte aligned"):
        _lib.call("ullsam_causal_attention", dtype, *ptrs, None, 1, 4, 2, 128, 64, 64, 64, 0, None)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("window,grid", [(14, 64), (0, 64), (7, 10), (0, 12)])
@pytest.mark.parametrize("which", range(5))
def test_vit_attention_refuses_an_unaligned_base_before_any_launch(lib, dtype, window, grid, which):
    """win14r / vitglob used to fall back to win14_attn_kernel / the 8-wave tiled kernel on such a base -- which read 16 bytes at a time themselves."""
    from ullsam_amd import _lib
    ptrs = [BASE + 0x1000000 * i + (8 if i == which else 0) for i in range(5)]
    with pytest.raises(_lib.UllsamError, match="16-byte aligned"):
        _lib.call("ullsam_vit_attention", dtype, *ptrs, 1, 2, 80, grid, grid, window, None)
