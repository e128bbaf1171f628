"""Wall time of one SFT step with the LLM trainable (train.py:284-318 with --freeze_vision: model(..., labels=...).loss.backward() through mlp1, the token
embeddings, every decoder layer, the final norm and the LM head) at the shapes of the models the reference ships (SAM ViT-B + InternLM2-1.8B-shaped) or the
bench's (ViT-H + 7B-shaped).  Correctness of the step is gated by tests/test_train_llm_gpu.py; this only times it.  One JSON line per run.
    usage: python tools/train_llm_step_bench.py [b|h] [2b|7b] [fp32|bf16] [steps]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from ullsam_amd.utils.synthetic import microscopy_batch

vit = sys.argv[1] if len(sys.argv) > 1 else "b"
llm = sys.argv[2] if len(sys.argv) > 2 else "2b"
dt = torch.bfloat16 if (len(sys.argv) > 3 and sys.argv[3] == "bf16") else torch.float32
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
dev = "cuda:0"
m = bench.build_model(vit, llm, dt, dev)
for n, p in m.named_parameters():
    p.requires_grad_(not n.startswith("vision_model."))
imgs, _ = microscopy_batch([3])
x = torch.from_numpy(imgs).to(dev).to(dt)
ids = torch.from_numpy(bench.make_input_ids(20, 34, seed=1)).to(dev)
labels = ids.clone()
labels[:, :1050] = -100                      # the loss over the answer turn only, as the SFT dataset masks the prompt
m.train()
times = []
for it in range(steps):
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize(); t0 = time.perf_counter()
    loss = m(pixel_values=x, input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels, return_dict=True, use_cache=False).loss
    torch.cuda.synchronize(); t1 = time.perf_counter()
    loss.backward()
    torch.cuda.synchronize(); t2 = time.perf_counter()
    times.append((t1 - t0, t2 - t1))
fw, bw = times[-1]
print(json.dumps({"workload": f"SFT step, ViT-{vit.upper()} (frozen) + InternLM2-{llm}-shaped (trainable) + mlp1, {'bf16' if dt == torch.bfloat16 else 'fp32'} model, S = {ids.shape[1]}",
                  "step_ms": round(1e3 * (fw + bw), 1), "forward_ms": round(1e3 * fw, 1), "backward_ms": round(1e3 * bw, 1), "loss": round(float(loss.detach()), 4),
                  "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                  "params_with_grad": sum(p.grad is not None for p in m.parameters())}))
