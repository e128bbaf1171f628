"""Time utils.split.split_labels on a synthetic label frame in which pairs of touching cells were fused into one id, in one process, the routes
alternating:

  (a) the host form: the numpy definition, labels in host memory;
  (b) the device route (csrc/split.hip): labels resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call;
  (c) where scikit-image is installed: peak_local_max + skimage.segmentation.watershed of the same distance map, for time only (its parts are not
      these parts, and no equality is claimed).

    python tools/split_bench.py [--size 2048] [--cells 400] [--depth 2] [--reps 3] [--stages] [--no-host] [--out profiles/r19_split.txt]

Prints every run, the medians and the spread (max - min), whether the two routes give identical outputs, the basins / pairs / rounds / parts of the
frame, and with --stages the device route stage by stage (device events) with the LDS / global A/B of the ascent; --out appends the lines to a file.
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
from ullsam_amd.utils import split as SP  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


def fuse_pairs(lab: np.ndarray):
    """Cells that touch along a row are fused two by two (every cell in at most one pair): the smaller id takes the larger one's pixels."""
    a, b = lab[:, :-1], lab[:, 1:]
    m = (a > 0) & (b > 0) & (a != b)
    pairs = np.unique(np.stack([np.minimum(a[m], b[m]), np.maximum(a[m], b[m])], 1), axis=0)
    to = np.arange(int(lab.max()) + 1)
    used = set()
    for x, y in pairs.tolist():
        if x not in used and y not in used:
            used.update((x, y))
            to[y] = x
    return to[lab].astype(np.int32), len(used) // 2


def skimage_route(lab, d2):
    from skimage.feature import peak_local_max
    from skimage.segmentation import watershed
    d = np.sqrt(d2.astype(np.float64))
    peaks = peak_local_max(d, labels=lab, min_distance=3)
    seeds = np.zeros(lab.shape, np.int32)
    seeds[tuple(peaks.T)] = np.arange(1, len(peaks) + 1)
    return watershed(-d, seeds, mask=lab > 0)


def stages(lab_d, depth, reps, say):
    """The device route stage by stage through ops, each between two device events."""
    from ullsam_amd import ops
    h, w = lab_d.shape
    n = h * w
    k = int(lab_d.max())
    times = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        return out

    for rep in range(reps + 1):                          # (the first round is the warm-up)
        g, _, _ = timed("distance columns", lambda: ops.distance_columns(lab_d, False, False, num=k))
        d2, _ = timed("distance rows -> D2", lambda: ops.distance_rows(lab_d, g, None, "inner", num=k))
        order = ("lds", "global") if rep % 2 else ("global", "lds")      # the A/B alternates
        for route in order:
            up, flags = timed(f"ascent, {route}", lambda: ops.split_ascent(lab_d, d2, k, route))
        timed("flatten (after the ascent)", lambda: ops.split_flatten(up, flags=flags))
        keys, vals, _ = timed("passes (table zeroed, atomicMax inserts)", lambda: ops.split_passes(lab_d, d2, up, 1 << 20, k, flags))
        best = timed("best words zeroed (8 B a pixel, once)", lambda: torch.zeros((n,), dtype=torch.int64, device=lab_d.device))
        changed = torch.zeros((64,), dtype=torch.int32, device=lab_d.device)
        for r in range(64):
            timed(f"round {r + 1}: best + decide", lambda: ops.split_round(keys, vals, lab_d, d2, up, depth, best, changed[r:r + 1], k, flags))
            if not int(changed[r].cpu()):
                break
            timed(f"round {r + 1}: flatten", lambda: ops.split_flatten(up, flags=flags))
        timed("collect: count", lambda: ops.split_collect(lab_d, up, None, k, flags))
        parts = int(flags.cpu()[4])
        lst, _ = timed("collect: list", lambda: ops.split_collect(lab_d, up, parts, k, flags))
        lst = timed("sort of the K' keys (torch)", lambda: torch.sort(lst).values)
        timed("tables + relabel", lambda: ops.split_relabel(lst, lab_d, d2, up, k, flags))
    total = 0.0
    for name, t in times.items():
        ms = med(t[1:])
        total += 0.0 if name == "ascent, global" else ms
        say(f"    stage {name:<44s} {ms * 1e3:10.1f} us (spread {spread(t[1:]) * 1e3:8.1f})")
    say(f"    the stages' medians sum to {total * 1e3:.1f} us (the global ascent left out)")
    a, b = times["ascent, lds"][1:], times["ascent, global"][1:]
    gap, worse = med(b) - med(a), max(spread(a), spread(b))
    say(f"    ascent A/B: lds {med(a) * 1e3:.1f} us, global {med(b) * 1e3:.1f} us; global - lds = {gap * 1e3:.1f} us against 3 x the larger spread "
        f"{3 * worse * 1e3:.1f} us -> {'lds is faster' if gap > 3 * worse else 'global is faster' if -gap > 3 * worse else 'no claim'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--rmin", type=float, default=20.0)
    ap.add_argument("--rmax", type=float, default=60.0)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form and scikit-image (the device route alone)")
    ap.add_argument("--stages", action="store_true", help="also time the device route stage by stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lab, fused = fuse_pairs(S.label_frame(1, a.size, a.size, a.cells, (a.rmin, a.rmax)))
    say(f"label_frame {a.size}^2, {a.cells} cells of radius {a.rmin}..{a.rmax}, {fused} pairs of touching cells fused: {len(np.unique(lab[lab > 0]))} ids, "
        f"{100 * (lab > 0).mean():.1f} % of the pixels labelled; min_depth = {a.depth}")
    try:
        import skimage  # noqa: F401
        ski = not a.no_host
    except ImportError:
        ski = False
    say("scikit-image: " + ("installed" if ski else "skipped" if a.no_host else "not installed, its route is not measured"))
    lab_d = torch.from_numpy(lab).cuda()
    k = int(lab.max())
    call = lambda x, kw: SP.split_labels(x, a.depth, num=k, **kw)
    st = {}
    dev = SP.split_labels(lab_d, a.depth, num=k, stats=st)      # warm-up: allocator, code objects
    torch.cuda.synchronize()
    say(f"basins {st['basins']}, pairs of touching basins {st['pairs']}, rounds {st['rounds']}, parts {st['parts']}")
    ta, tb, tc, host = [], [], [], None
    for _ in range(a.reps):
        if not a.no_host:
            t0 = time.perf_counter()
            host = call(lab, {"device": "cpu"})
            ta.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = call(lab_d, {})
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t0)
        if ski:
            from ullsam_amd.utils import distance as D
            d2 = D.inner_distance(lab).numpy()
            t0 = time.perf_counter()
            skimage_route(lab, d2)
            tc.append(time.perf_counter() - t0)
    ok = True
    say(f"split_labels(min_depth={a.depth})")
    say(f"  (b) device     labels resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s")
    if ta:
        ok = all(torch.equal(d.cpu(), h) for d, h in zip(dev, host))
        gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
        say(f"  (a) host form  numpy definition:              runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
        say(f"      outputs {'IDENTICAL' if ok else 'DIFFERENT'}; (a) / (b) = {med(ta) / med(tb):.1f}x; (a) - (b) = {gap:.6f} s against 3 x the larger spread "
            f"{3 * worse:.6f} s -> {'(b) is faster' if gap > 3 * worse else '(a) is faster' if -gap > 3 * worse else 'no claim'}")
    else:
        say("  (a) host form  not measured")
    if tc:
        gap, worse = med(tc) - med(tb), max(spread(tc), spread(tb))
        say(f"  (c) scikit-image peak_local_max + watershed (time only, the distance map given): runs {fmt(tc)} s, median {med(tc):.6f} s, spread {spread(tc):.6f} s; "
            f"(c) - (b) = {gap:.6f} s against {3 * worse:.6f} s -> {'(b) is faster' if gap > 3 * worse else '(c) is faster' if -gap > 3 * worse else 'no claim'}")
    else:
        say("  (c) scikit-image not measured")
    if a.stages:
        stages(lab_d, a.depth, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
