"""Latency of the interactive loop (ullsam_amd/interactive.py) at batch 1 against the route the model API alone gives, in one process on one GPU:

  (a) InteractiveSegmenter.set_image      preprocess + ViT + projector + LLM prefill + mlp2, once per image
  (b) InteractiveSegmenter.click          prompt encoder + mask decoder + the finish kernel, on a 1024^2 display
  (c) one click without the session       the full forward + prompt encoder + mask decoder + ops.resize_bilinear(threshold=0) (the call sequence
                                          of app.py:580-645), then the host tail below
  (d) the finish launch alone (mask, statistics, overlay with the highlight) against the host tail of (c): the download of the mask, PIL's
      Image.NEAREST (postprocess_mask, app.py:283-287) and the numpy overlay of visualize_masks (app.py:748-772) over the canvas
  (e) InteractiveSegmenter.predict_instances at P = 16 and 64 prompts

for the model the reference ships (ViT-B + a 2B-shaped LLM) and for ViT-H + a 7B-shaped LLM, bf16, seeded random weights.  One warm-up per
measurement, then --reps runs of each in turn (a, b, c, ..., a, b, c, ...), torch.cuda.synchronize() before and after each, time.perf_counter()
around; medians, spread = max - min.  "A click is cheaper than a forward" is written only when (c) - (b) exceeds three times the larger spread.

    python tools/interactive_bench.py [--configs b2b,h7b] [--reps 3] [--out profiles/r14_interactive.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_model, make_input_ids  # noqa: E402
from ullsam_amd import ops  # noqa: E402
from ullsam_amd.interactive import InteractiveSegmenter  # noqa: E402
from ullsam_amd.utils.imageprep import preprocess_image  # noqa: E402
from ullsam_amd.utils.interactive import default_palette, frame_coords  # noqa: E402
from ullsam_amd.utils.synthetic import microscopy_tile  # noqa: E402

try:
    import PIL
    from PIL import Image
except ImportError:
    Image = None

CONFIGS = {"b2b": ("b", "2b", "ViT-B + 2B-shaped LLM (the model the reference ships)"), "h7b": ("h", "7b", "ViT-H + 7B-shaped LLM")}
DEV = "cuda:0"


def seeded_weights_(model, seed=0):
    """Seeded random weights generated on the device (the values do not enter a latency): matrices N(0, 0.02^2), biases 0, other vectors 1."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g, device=DEV, dtype=torch.float32) * 0.02)
            elif name.endswith("bias"):
                p.zero_()
            else:
                p.fill_(1.0)


def host_tail(mask_dev, image, canvas, colors):
    """What the app does with the thresholded frame mask of one click: download, postprocess_mask, visualize_masks with the current mask."""
    mask = mask_dev.cpu().numpy()
    mask_image = Image.fromarray(mask.astype(np.uint8)).resize((image.shape[1], image.shape[0]), Image.NEAREST)      # app.py:283-287
    current_mask = np.array(mask_image) > 0
    overlay = image.copy()                                                                                            # app.py:743-772
    if np.max(canvas) > 0:
        for instance_id in range(1, np.max(canvas) + 1):
            instance_mask = (canvas == instance_id)
            if np.any(instance_mask):
                color = colors[(instance_id - 1) % len(colors)]
                overlay[instance_mask] = ((1 - 0.5) * overlay[instance_mask] + 0.5 * np.array(color)).astype(np.uint8)
    if np.any(current_mask):
        overlay[current_mask] = ((1 - 0.7) * overlay[current_mask] + 0.7 * np.array((0, 255, 0))).astype(np.uint8)
    return current_mask, overlay


def run_config(key, reps, lines):
    vit, llm, what = CONFIGS[key]
    model = build_model(vit, llm, torch.bfloat16, DEV, init=False)
    seeded_weights_(model)
    ids = torch.from_numpy(make_input_ids(20, 34, seed=1)).to(DEV)
    am, flags = torch.ones_like(ids), (ids == 92546)[..., None].long()
    tile, centres = microscopy_tile(7)
    image = np.ascontiguousarray((np.clip(tile, 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0))
    image_dev = torch.from_numpy(image).to(DEV)
    colors = [tuple(int(c) for c in row) for row in default_palette()]
    saved = [[float(x), float(y)] for x, y in centres[:3]]
    click = [[float(centres[3][0]), float(centres[3][1])]]
    rng = np.random.default_rng(0)
    many = {P: rng.integers(16, 1008, (P, 1, 2)).astype(np.float32) for P in (16, 64)}
    seg = InteractiveSegmenter(model, ids)
    pe, md = model.prompt_encoder, model.mask_decoder
    state = {}

    def a_set_image():
        seg.set_image(image_dev)

    def prepare():                                            # three saved instances on the canvas, as after three rounds of the app
        seg.reset_instances()
        for p in saved:
            seg.click([p], [1])
            seg.save_instance()
        state["canvas"] = seg.labels.cpu().numpy()

    def b_click():
        state["click"] = seg.click(click, [1])

    def c_forward_route():
        x = state["x"]
        out = model(pixel_values=x, input_ids=ids, attention_mask=am, image_flags=flags, return_dict=True, use_cache=False, output_hidden_states=True)
        pts = torch.from_numpy(frame_coords([click], 1024, 1024)).to(DEV)                 # int(x * img_size / width), app.py:536-537
        sp, de = pe(points=(pts, torch.ones((1, 1), dtype=torch.int32, device=DEV)), boxes=None, masks=None, llm_hidden_states=out.hidden_states)
        low, _ = md(image_embeddings=out.image_embeddings, image_pe=pe.get_dense_pe(), sparse_prompt_embeddings=sp, dense_prompt_embeddings=de,
                    multimask_output=False)
        _, mk = ops.resize_bilinear(low.float().contiguous(), (1024, 1024), want_float=False, threshold=0.0)
        state["frame_mask"] = mk[0, 0]
        if Image is not None:
            state["host"] = host_tail(mk[0, 0], image, state["canvas"], colors)

    def d_finish():
        r = state["click"]
        state["finish"] = seg._finish(r.low[:, 0].contiguous(), highlight=True, want_overlay=True)

    def d_host_tail():
        state["host"] = host_tail(state["frame_mask"], image, state["canvas"], colors)

    def e_instances(P):
        def run():
            seg.count = 3                                     # over the same three saved instances every time (ids 4 .. 3 + P are repainted)
            seg.predict_instances(many[P], np.ones((P, 1), np.int32))
        return run

    a_set_image()
    state["x"] = preprocess_image(image_dev, device=DEV).to(torch.bfloat16)
    prepare()
    work = [("(a) set_image", a_set_image), ("(b) click", b_click), ("(c) forward route + host tail" if Image is not None else "(c) forward route, NO host tail (PIL absent)",
                                                                       c_forward_route),
            ("(d) finish launch alone", d_finish)]
    if Image is not None:
        work.append(("(d) host tail alone", d_host_tail))
    work += [("(e) predict_instances P=16", e_instances(16)), ("(e) predict_instances P=64", e_instances(64))]
    times = {name: [] for name, _ in work}
    for name, fn in work:                                     # warm-up, in order: (b) needs the image of (a), (d) the results of (b) and (c)
        fn()
    a_set_image()
    prepare()
    for _ in range(reps):
        for name, fn in work:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); times[name].append(time.perf_counter() - t0)
            if name.startswith("(a)"):                        # set_image resets the canvas: put the three instances back, outside the timing
                prepare()
    med, spread = statistics.median, (lambda t: max(t) - min(t))
    lines.append(f"{key}: {what}, bf16, batch 1, prompt of {ids.shape[1]} tokens, 1024^2 uint8 RGB image resident on the device, three saved instances on the canvas")
    for name, _ in work:
        t = times[name]
        lines.append(f"  {name:48s} runs {', '.join(f'{1e3 * x:.3f}' for x in t)} ms, median {1e3 * med(t):.3f} ms, spread {1e3 * spread(t):.3f} ms")
    b, c = times["(b) click"], times[work[2][0]]
    gain, bound = med(c) - med(b), 3 * max(spread(b), spread(c))
    lines.append(f"  (c) - (b) = {1e3 * gain:.3f} ms against 3 x the larger spread = {1e3 * bound:.3f} ms: "
                 + ("a click is cheaper than a forward" if gain > bound else "NO claim: the difference does not exceed three spreads")
                 + f"; (c) / (b) = {med(c) / med(b):.1f}x")
    if Image is not None:
        f, h = times["(d) finish launch alone"], times["(d) host tail alone"]
        lines.append(f"  (d) host tail / finish launch = {med(h) / med(f):.1f}x ({1e3 * (med(h) - med(f)):.3f} ms against 3 x the larger spread = {1e3 * 3 * max(spread(f), spread(h)):.3f} ms)")
        r = state["click"]
        same = bool(np.array_equal(r.mask.cpu().numpy().astype(bool), state["host"][0])) and bool(np.array_equal(r.overlay.cpu().numpy(), state["host"][1]))
        lines.append(f"  the session's mask and overlay equal the host tail's on this click: {same}")
    del seg, model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="b2b,h7b")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"tools/interactive_bench.py --configs {a.configs} --reps {a.reps} on {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} host cores available"
             + (f", PIL {PIL.__version__}" if Image is not None else ", PIL ABSENT: no host tail"),
             f"how: one process; one warm-up per measurement, then {a.reps} runs of each in turn, torch.cuda.synchronize() before and after, time.perf_counter() around; "
             "medians and spread = max - min"]
    for key in a.configs.split(","):
        run_config(key, a.reps, lines)
        print("\n".join(lines[-12:]), flush=True)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
