"""Greedy decode throughput of the InternLM2-7B-shaped LLM (app.py:431-495 caption path): prefill S tokens, then n new tokens.
usage: python tools/decode_bench.py [batch] [prompt_len] [new_tokens] [fp8]
fp8: the weight-only e4m3 decode (InternLM2ForCausalLM.fp8_decode) against the bf16 decode in ONE process, three alternating runs each (bf16, fp8, bf16, fp8, ...);
one JSON line per run with the weight bytes a step really streams and the fraction of 8 TB/s that is, then a summary line with the ratio and the bf16 runs' spread."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import build_model
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1081
n = int(sys.argv[3]) if len(sys.argv) > 3 else 64
fp8 = len(sys.argv) > 4 and sys.argv[4] == "fp8"
if os.environ.get("ULLSAM_GEMM_VARIANT"):
    from ullsam_amd import _lib
    _lib.load().ullsam_set_gemm_variant(int(os.environ["ULLSAM_GEMM_VARIANT"]))
m = build_model("b", "7b", torch.bfloat16, "cuda:0")
lm = m.language_model
ids = torch.randint(0, 90000, (B, S), device="cuda")
def run(k):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = lm.generate(input_ids=ids, max_new_tokens=k, eos_token_id=-1)
    torch.cuda.synchronize(); return time.perf_counter() - t0, out
def measure():
    run(4)
    t1, _ = run(1)
    tn, out = run(n)
    return t1, (tn - t1) / (n - 1)
if not fp8:
    t1, per = measure()
    print(json.dumps({"workload": f"greedy decode, InternLM2-7B-shaped, bf16, batch {B}, prompt {S}", "prefill_plus_first_token_ms": round(t1 * 1e3, 1),
                      "ms_per_decode_step": round(per * 1e3, 3), "tokens_per_s": round(B / per, 1),
                      "weight_bytes_per_step_GB": 15.5, "hbm_floor_ms": round(15.5e9 / 5e12 * 1e3, 2)}))
    sys.exit(0)
# the linears a decode step streams: every layer's wqkv / wo / w1 / w3 / w2 and the LM head (the token embedding is a row gather)
lin = [p for k, p in lm.named_parameters() if k.endswith(".weight") and p.dim() == 2 and "tok_embeddings" not in k]
n_w, n_rows = sum(p.numel() for p in lin), sum(p.shape[0] for p in lin)
from ullsam_amd.checkpoint import prepack
prepack(lm, fp8_decode=True)
runs = {"bf16": [], "fp8": []}
for rep in range(3):
    for mode in ("bf16", "fp8"):
        lm.fp8_decode = mode == "fp8"
        t1, per = measure()
        gb = (n_w * 2 if mode == "bf16" else n_w + n_rows * 4) / 1e9   # (fp8: one byte per weight + the rows' fp32 scales)
        runs[mode].append(per)
        print(json.dumps({"workload": f"greedy decode, InternLM2-7B-shaped, {mode} weights, batch {B}, prompt {S}", "run": rep, "prefill_plus_first_token_ms": round(t1 * 1e3, 1),
                          "ms_per_decode_step": round(per * 1e3, 3), "tokens_per_s": round(B / per, 1), "weight_bytes_per_step_GB": round(gb, 2),
                          "fraction_of_8TBps": round(gb * 1e9 / per / 8e12, 3)}), flush=True)
lm.fp8_decode = False
mb, mf = sorted(runs["bf16"])[1], sorted(runs["fp8"])[1]
spread = max(runs["bf16"]) - min(runs["bf16"])
print(json.dumps({"summary": "fp8 decode against bf16 decode, medians of 3 alternating runs", "bf16_ms_per_step": round(mb * 1e3, 3), "fp8_ms_per_step": round(mf * 1e3, 3),
                  "bf16_over_fp8": round(mb / mf, 3), "bf16_spread_ms": round(spread * 1e3, 3), "gain_ms": round((mb - mf) * 1e3, 3),
                  "faster_by_more_than_3_spreads": bool(mb - mf > 3 * spread)}))
