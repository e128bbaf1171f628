"""Time utils.raster.rasterize_polygons on the outline rings of the synthetic label frame of tools/distance_bench.py and of one adversarial frame,
a single spiral corridor whose one loop has long edges with many crossings each, in one process, the routes alternating:

  (a) the host form: the numpy definition, rings in host memory, after one warm-up call;
  (b) the device route (csrc/raster.hip): rings resident on the GPU as label_outlines left them, torch.cuda.synchronize() before and after, after
      one warm-up call -- once per paint form ("waves": one wave per span; "pixels": one lane per pixel), the A/B of the paint stage: the two
      forms in alternating order, after one untimed device call that follows the host form (the device idles while numpy runs);
  (c) timing only, where Pillow is installed: one ImageDraw.polygon per ring on the host (holes painted 0).  Pillow's rule is its own: no equality
      is claimed against it.

    python tools/raster_bench.py [--size 2048] [--cells 400] [--reps 3] [--stages] [--no-host] [--out profiles/r21_raster.txt]

Prints every run, the medians and the spread (max - min), whether (a) and (b) give identical outputs and the round trip returns the label image, the
rings / vertices / crossings / spans of each frame, and with --stages the device route stage by stage (device events); --out appends the lines
to a file.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from outline_bench import spiral  # noqa: E402
from ullsam_amd.utils import outline as OL  # noqa: E402
from ullsam_amd.utils import raster as RA  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)
FORMS = ("waves", "pixels")


def verdict(ta, tb, a, b) -> str:
    gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
    return (f"{a} - {b} = {gap:.6f} s against 3 x the larger spread {3 * worse:.6f} s -> "
            f"{b + ' is faster' if gap > 3 * worse else a + ' is faster' if -gap > 3 * worse else 'no claim'}")


def stages(out, h, w, k, reps, say):
    """The device route stage by stage through ops, each between two device events; the paint stage in both forms."""
    from ullsam_amd import ops
    dev = out.vertices.device
    q = (out.vertices.long() * RA.SUB).to(torch.int32).contiguous()
    times = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        return res

    for _ in range(reps + 1):                             # (the first round is the warm-up)
        flags = torch.zeros((ops.RASTER_FLAGS,), dtype=torch.int32, device=dev)
        row0, cnt, nxt, elab, off, _ = timed("edges: rows, counts + their scan", lambda: ops.raster_edges(q, out.start, out.label, h, w, k, flags))
        c = timed("read-back: status, C", lambda: flags.cpu().tolist())[1]
        keys, _ = timed("keys: one work item per crossing", lambda: ops.raster_keys(q, row0, cnt, nxt, elab, off, c, h, w, k, flags))
        keys = timed("sort of the C keys (torch)", lambda: torch.sort(keys).values)
        covered, length, _ = timed("covered per label, span lengths", lambda: ops.raster_covered(keys, h, w, k, flags))
        rank = timed("ranks by area (torch, K rows)", lambda: torch.empty((k,), dtype=torch.int32, device=dev).index_put_(
            (torch.sort(-covered.long(), stable=True).indices,), torch.arange(k, dtype=torch.int32, device=dev)))
        raw, _ = timed("paint, waves: one wave per span", lambda: ops.raster_paint(keys, rank, h, w, "waves", None, flags))
        timed("paint, pixels: scan of the lengths + one lane per pixel", lambda: ops.raster_paint(keys, rank, h, w, "pixels", length, flags))
        label_of = torch.zeros((k + 1,), dtype=torch.int32, device=dev)
        label_of[(rank + 1).long()] = torch.arange(1, k + 1, dtype=torch.int32, device=dev)
        timed("finish: rank -> label, area, box", lambda: ops.raster_finish(raw, label_of, flags))
    for name, t in times.items():
        say(f"    stage {name:<56s} {med(t[1:]) * 1e3:10.1f} us (spread {spread(t[1:]) * 1e3:8.1f})")
    tw, tp = ([x * 1e-3 for x in times[n][1:]] for n in ("paint, waves: one wave per span", "paint, pixels: scan of the lengths + one lane per pixel"))
    say("    paint stage alone: " + verdict(tw, tp, "waves", "pixels"))


def pillow(verts, start, label, area2, h, w):
    from PIL import Image, ImageDraw
    img = Image.new("I", (w, h), 0)
    draw = ImageDraw.Draw(img)
    for i in range(len(label)):
        draw.polygon([tuple(p) for p in verts[start[i]:start[i + 1]].tolist()], fill=int(label[i]) if area2[i] > 0 else 0)
    return img


def measure(name, lab, a, say) -> bool:
    h, w = lab.shape
    k = int(lab.max())
    lab_d = torch.from_numpy(lab).cuda()
    out = OL.label_outlines(lab_d, 8, num=k)              # the rings, resident on the device
    host = [t.cpu().numpy() for t in (out.vertices, out.start, out.label)]
    area2 = out.area2.cpu().numpy()
    call_d = lambda form: RA.rasterize_polygons(out.vertices, out.start, out.label, (h, w), "area", k, paint=form)
    call_h = lambda: RA.rasterize_polygons(*host, (h, w), "area", k, device="cpu")
    dev = {f: call_d(f) for f in FORMS}                   # warm-up: allocator, code objects
    torch.cuda.synchronize()
    if not a.no_host:
        call_h()                                          # and one of the host form: first-touch pages of its arrays
    lengths = np.diff(host[1])
    say(f"{name}: {h} x {w}, {k} ids; {len(host[2])} rings, {len(host[0])} vertices, the longest ring {int(lengths.max())} vertices; "
        f"{int(dev['waves'].covered.sum())} covered pixels; order=\"area\"")
    ta, tc, tb, res_h = [], [], {f: [] for f in FORMS}, None
    try:
        import PIL  # noqa: F401
        have_pillow = not a.no_host
    except ImportError:
        have_pillow = False
    for rep in range(a.reps):
        if not a.no_host:
            t0 = time.perf_counter()
            res_h = call_h()
            ta.append(time.perf_counter() - t0)
            call_d(RA.PAINT)                              # (not timed: the device idled during the host form, the first call after it pays for that)
        for f in (FORMS if rep % 2 == 0 else FORMS[::-1]):   # the two paint forms in alternating order
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev[f] = call_d(f)
            torch.cuda.synchronize()
            tb[f].append(time.perf_counter() - t0)
        if have_pillow:
            t0 = time.perf_counter()
            pillow(*host, area2, h, w)
            tc.append(time.perf_counter() - t0)
    ok = all(torch.equal(x, y) for x, y in zip(dev["waves"], dev["pixels"])) and torch.equal(dev[RA.PAINT].labels, lab_d)
    for f in FORMS:
        say(f"  (b) device, paint={f:<7s} rings resident, synchronised: runs {fmt(tb[f])} s, median {med(tb[f]):.6f} s, spread {spread(tb[f]):.6f} s")
    say(f"      the two forms give {'IDENTICAL' if ok else 'DIFFERENT'} outputs and the round trip {'returns' if ok else 'DOES NOT return'} the label image; "
        + verdict(tb["waves"], tb["pixels"], "waves", "pixels"))
    if ta:
        same = all(d.dtype == x.dtype and torch.equal(d.cpu(), x) for d, x in zip(dev[RA.PAINT], res_h))
        ok = ok and same
        say(f"  (a) host form  numpy definition:                       runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
        say(f"      outputs {'IDENTICAL' if same else 'DIFFERENT'}; (a) / (b) = {med(ta) / med(tb[RA.PAINT]):.1f}x; " + verdict(ta, tb[RA.PAINT], "(a)", "(b)"))
    else:
        say("  (a) host form  not measured")
    if tc:
        say(f"  (c) Pillow     one ImageDraw.polygon per ring (timing only): runs {fmt(tc)} s, median {med(tc):.6f} s, spread {spread(tc):.6f} s; "
            f"(c) / (b) = {med(tc) / med(tb[RA.PAINT]):.1f}x")
    else:
        say("  (c) Pillow     not measured")
    if a.stages:
        stages(out, h, w, k, a.reps, say)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--rmin", type=float, default=20.0)
    ap.add_argument("--rmax", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form and Pillow (the device route alone)")
    ap.add_argument("--stages", action="store_true", help="also time the device route stage by stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = measure(f"label_frame, {a.cells} cells of radius {a.rmin}..{a.rmax}", S.label_frame(1, a.size, a.size, a.cells, (a.rmin, a.rmax)), a, say)
    ok = measure("one spiral corridor", spiral(a.size), a, say) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
