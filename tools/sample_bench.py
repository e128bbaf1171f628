"""Sampled decode of the InternLM2-7B-shaped LLM with the caption path's policy (app.py:469-477: T 0.7, top_k 50, top_p 0.9) against greedy decode.
usage: python tools/sample_bench.py [batch] [prompt_len] [new_tokens]
Three alternating runs each of greedy, the host sampler (do_sample without seed: torch ops on the global generator, a blocking stop test every step) and
the fused sampler (do_sample with seed: one ullsam_sample_topk_topp launch a step, pipelined stop test), bf16, eos_token_id=-1, in ONE process.
One JSON line per run, then a summary with the medians, each sampled route's surplus over greedy and the greedy runs' spread."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import build_model
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1081
n = int(sys.argv[3]) if len(sys.argv) > 3 else 64
m = build_model("b", "7b", torch.bfloat16, "cuda:0")
lm = m.language_model
ids = torch.randint(0, 90000, (B, S), device="cuda")
POLICY = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
MODES = {"greedy": {}, "host_sampler": POLICY, "fused_sampler": dict(POLICY, seed=1234)}
def run(k, kw):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = lm.generate(input_ids=ids, max_new_tokens=k, eos_token_id=-1, **kw)
    torch.cuda.synchronize(); return time.perf_counter() - t0, out
def measure(kw):
    run(4, kw)
    t1, _ = run(1, kw)
    tn, out = run(n, kw)
    return t1, (tn - t1) / (n - 1)
runs = {k: [] for k in MODES}
for rep in range(3):
    for mode, kw in MODES.items():
        t1, per = measure(kw)
        runs[mode].append(per)
        print(json.dumps({"workload": f"{mode} decode, InternLM2-7B-shaped, bf16, batch {B}, prompt {S}" + (", T 0.7 / top_k 50 / top_p 0.9" if kw else ""), "run": rep,
                          "prefill_plus_first_token_ms": round(t1 * 1e3, 1), "ms_per_decode_step": round(per * 1e3, 3), "tokens_per_s": round(B / per, 1)}), flush=True)
med = {k: sorted(v)[1] for k, v in runs.items()}
spread = max(runs["greedy"]) - min(runs["greedy"])
gain = med["host_sampler"] - med["fused_sampler"]
print(json.dumps({"summary": "sampled decode against greedy decode, medians of 3 alternating runs", "greedy_ms_per_step": round(med["greedy"] * 1e3, 3),
                  "host_sampler_ms_per_step": round(med["host_sampler"] * 1e3, 3), "fused_sampler_ms_per_step": round(med["fused_sampler"] * 1e3, 3),
                  "host_surplus_over_greedy_ms": round((med["host_sampler"] - med["greedy"]) * 1e3, 3),
                  "fused_surplus_over_greedy_ms": round((med["fused_sampler"] - med["greedy"]) * 1e3, 3), "greedy_spread_ms": round(spread * 1e3, 3),
                  "gain_ms": round(gain * 1e3, 3), "faster_by_more_than_3_spreads": bool(gain > 3 * spread)}))
