"""Time image preprocessing of one 2048^2 x 3 uint8 microscopy tile (utils.synthetic.microscopy_tile) to float32 [1, 3, 1024, 1024], in one
process, the measurements alternating:

  (a) device: upload the uint8 tile (12 MiB, pageable memory) and run utils.imageprep.preprocess_image on it; also with the tile already resident;
  (b) host:   what the reference does -- PIL's Image.resize(BILINEAR), ToTensor's permute / float / div(255) -- then the upload of the float tensor
      (12 MiB).  Without PIL on the machine (a) is reported alone, and the output says so.

Then the two kernels on their own (HIP events, 20 launches each), and SamAutomaticMaskGenerator.generate on the real-size tile (ViT-H, 64 x 64 points,
the thresholds of tools/amg_bench.py) under image_resize="bilinear" and "pil".

    python tools/imageprep_bench.py [--reps 3] [--no-amg] [--out profiles/r13_imageprep.txt]
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
from ullsam_amd import _lib, ops  # noqa: E402
from ullsam_amd.utils.imageprep import preprocess_image  # noqa: E402
from ullsam_amd.utils.synthetic import microscopy_tile  # noqa: E402

try:
    import PIL
    from PIL import Image
except ImportError:
    Image = None

S = 1024


def host_route(tile):
    x = torch.from_numpy(np.array(Image.fromarray(tile).resize((S, S), Image.BILINEAR)))      # (a copy, as ToTensor makes)
    return x.permute(2, 0, 1).contiguous().float().div(255)[None].cuda()


def kernel_times(dev_tile, n=20):
    """(horizontal, vertical) device times in ms, medians over n launches, each between two HIP events."""
    H, W, C = dev_tile.shape
    bh, ch, kh = ops._aa_tables_dev(W, S, "bilinear", True, dev_tile.device)
    bv, cv, kv = ops._aa_tables_dev(H, S, "bilinear", False, dev_tile.device)
    row0, rows = ops.aa_row_span(H, S, "bilinear")
    tmp = torch.empty((rows, S, C), dtype=torch.uint8, device=dev_tile.device)
    out = torch.empty((3, S, S), dtype=torch.float32, device=dev_tile.device)
    lut = (torch.arange(256, dtype=torch.float32) / 255).repeat(3, 1).contiguous().cuda()
    st = torch.cuda.current_stream().cuda_stream

    def h():
        _lib.call("ullsam_resize_u8_aa_h", dev_tile.data_ptr(), *dev_tile.stride(), H, W, C, 0, 0, H, W, row0, rows, bh.data_ptr(), ch.data_ptr(), kh, S,
                  tmp.data_ptr(), st)

    def v():
        _lib.call("ullsam_resize_u8_aa_v", tmp.data_ptr(), row0, rows, S, C, bv.data_ptr(), cv.data_ptr(), kv, S, None, lut.data_ptr(), out.data_ptr(),
                  out.stride(0), out.stride(1), st)

    res = []
    for fn in (h, v):
        fn()
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res.append(ts)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-amg", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    med = statistics.median
    spread = lambda t: max(t) - min(t)
    fmt = lambda t: ", ".join(f"{1e3 * x:.3f}" for x in t)
    line = lambda name, t: f"  {name} runs {fmt(t)} ms, median {1e3 * med(t):.3f} ms, spread {1e3 * spread(t):.3f} ms"
    tile_f, _ = microscopy_tile(7, size=2048, n_cells=40, r_range=(90.0, 260.0))
    tile = np.ascontiguousarray((np.clip(tile_f, 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0))
    lines = [f"tools/imageprep_bench.py --reps {a.reps} on {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} host cores available",
             f"how: one process; one warm-up call per route, then {a.reps} runs of each route in turn, torch.cuda.synchronize() before and after, "
             "time.perf_counter() around; medians and spread = max - min",
             f"tile: uint8 {tile.shape} -> float32 [1, 3, {S}, {S}] (mean 0, std 1: the app's transform)"]
    resident = torch.from_numpy(tile).cuda()
    want = preprocess_image(resident, img_size=S)                                   # warm-up: tables, allocator, code objects
    if Image is not None:
        same = torch.equal(host_route(tile), want)
    torch.cuda.synchronize()
    ta, tr, tb = [], [], []
    for _ in range(a.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        preprocess_image(torch.from_numpy(tile).cuda(), img_size=S)
        torch.cuda.synchronize(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        preprocess_image(resident, img_size=S)
        torch.cuda.synchronize(); tr.append(time.perf_counter() - t0)
        if Image is not None:
            t0 = time.perf_counter()
            host_route(tile)
            torch.cuda.synchronize(); tb.append(time.perf_counter() - t0)
    lines += [line("(a) device, upload of the uint8 tile + preprocess_image:", ta), line("(a) device, tile resident, preprocess_image alone:   ", tr)]
    if Image is not None:
        lines += [line(f"(b) host, PIL {PIL.__version__} resize + ToTensor ops + upload of the floats:", tb),
                  f"  (a) and (b) give the same tensor: {same}; (b) / (a) = {med(tb) / med(ta):.1f}x with the upload, {med(tb) / med(tr):.1f}x against the resident tile"]
    else:
        lines.append("  PIL is ABSENT on this machine: route (b) was not measured")
    th, tv = kernel_times(resident)
    lines += ["the two launches on their own (HIP events around one launch, 20 launches each):",
              f"  horizontal pass 2048 x 2048 x 3 -> 2048 x 1024 x 3 uint8:            median {med(th):.4f} ms, spread {spread(th):.4f} ms",
              f"  vertical pass + table -> float32 [3, 1024, 1024] (reads 6 MiB back):   median {med(tv):.4f} ms, spread {spread(tv):.4f} ms"]
    if not a.no_amg:
        from bench import build_model
        from ullsam_amd.automatic_mask_generator import SamAutomaticMaskGenerator
        from ullsam_amd.utils.synthetic import blob_decoder_init
        sam = blob_decoder_init(build_model("h", "none", torch.bfloat16, "cuda:0"))
        kw = dict(points_per_side=64, points_per_batch=64, pred_iou_thresh=0.90, stability_score_thresh=0.92, stability_score_offset=1.0, box_nms_thresh=0.7,
                  output_mode="uncompressed_rle")
        planar = torch.from_numpy(np.ascontiguousarray(tile.transpose(2, 0, 1))).cuda()
        gens = {m: SamAutomaticMaskGenerator(sam, image_resize=m, **kw) for m in ("bilinear", "pil")}
        times, kept = {m: [] for m in gens}, {}
        for m, g in gens.items():
            kept[m] = len(g.generate(planar))                                       # warm-up
        for _ in range(a.reps):
            for m, g in gens.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                g.generate(planar)
                torch.cuda.synchronize(); times[m].append(time.perf_counter() - t0)
        lines.append("SamAutomaticMaskGenerator.generate, ViT-H bf16, 64 x 64 points on the 2048^2 uint8 tile (resident, planar), thresholds of tools/amg_bench.py:")
        for m in gens:
            lines.append(line(f"image_resize={m!r:11s} ({kept[m]} records):", times[m]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
