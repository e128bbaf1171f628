"""Time utils.skeleton on two synthetic 2048^2 label frames -- the cells of the distance bench and a frame of branched filaments -- in one process, the
routes alternating:

  (a) the host form: the numpy definition, labels in host memory;
  (b) the device route (csrc/skeleton.hip) in every route it has: labels resident on the GPU, torch.cuda.synchronize() before and after, after one
      warm-up call.

    python tools/skeleton_bench.py [--size 2048] [--cells 400] [--filaments 300] [--reps 3] [--stages] [--no-host] [--out profiles/r27_skeleton.txt]

Prints every run, the medians and the spread (max - min), whether the routes give identical outputs, the instances / skeleton pixels / sub-iterations
of each frame, the A/B of the device routes by the rule "a difference counts beyond 3 x the larger spread", measure_skeletons on its own, and with
--stages the kernels one by one (device events) against the time of their bytes at 8 TB/s; --out appends the lines to a file.
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
from ullsam_amd.utils import distance as D  # noqa: E402
from ullsam_amd.utils import skeleton as SK  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)
HBM = 8e12                                                # bytes / s


def verdict(ta, tb, a, b):
    gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
    return (f"{a} - {b} = {gap:.6f} s against 3 x the larger spread {3 * worse:.6f} s -> "
            + (f"{b} is faster, {med(ta) / med(tb):.2f}x" if gap > 3 * worse else f"{a} is faster, {med(tb) / med(ta):.2f}x" if -gap > 3 * worse else "no claim"))


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stages(lab_d, sk_d, subiterations, reps, say):
    """The kernels one by one through ops, each launch between two device events."""
    from ullsam_amd import ops
    h, w = lab_d.shape
    n = h * w
    times = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1) * 1e-3)
        return out

    flags = torch.zeros((ops.SKEL_FLAGS,), dtype=torch.int32, device=lab_d.device)
    bufs = [torch.empty_like(lab_d), torch.empty_like(lab_d)]
    steps = -(-max(subiterations, 1) // ops.SKEL_TILE_STEPS) * ops.SKEL_TILE_STEPS
    counts = torch.zeros((steps,), dtype=torch.int32, device=lab_d.device)
    has_lds = "lds" in SK.ROUTES
    for rep in range(reps + 1):                           # (the first round is the warm-up)
        cur = lab_d
        for i in range(steps):
            cur = timed("skel_step, one sub-iteration", lambda: ops.skel_step(cur, bufs[i & 1], i, counts=counts[i:i + 1], flags=flags))[0]
        if has_lds:
            cur = lab_d
            for j, i in enumerate(range(0, steps, ops.SKEL_TILE_STEPS)):
                cur = timed("skel_tile, one launch", lambda: ops.skel_tile(cur, bufs[j & 1], i, counts=counts[i:i + ops.SKEL_TILE_STEPS], flags=flags))[0]
        timed("skel_measure, tables", lambda: ops.skel_measure(sk_d, int(lab_d.max()), None))
        timed("skel_measure, node image", lambda: ops.skel_measure(sk_d, None, None, nodes=True))
    per = {"skel_step, one sub-iteration": (1, 8 * n), "skel_measure, tables": (1, 4 * n), "skel_measure, node image": (1, 5 * n)}
    if has_lds:
        (ch, cw), s = ops.SKEL_TILE, ops.SKEL_TILE_STEPS
        per["skel_tile, one launch"] = (s, int(4 * n * (1 + (ch + 2 * s) * (cw + 2 * s) / (ch * cw))))
    launches = len(times["skel_step, one sub-iteration"]) // (reps + 1)
    for name, t in times.items():
        k = len(t) // (reps + 1)
        runs = [med(t[r * k:(r + 1) * k]) for r in range(1, reps + 1)]        # the median launch of every timed round
        subs, nbytes = per[name]
        say(f"    stage {name:<30s} {med(runs) * 1e6:9.1f} us a launch (spread of the rounds' medians {spread(runs) * 1e6:6.1f}), {med(runs) / subs * 1e6:8.1f} us a "
            f"sub-iteration; its {nbytes / 1e6:.1f} MB take {nbytes / HBM * 1e6:.1f} us at 8 TB/s: {med(runs) / (nbytes / HBM):.1f}x that")
    say(f"    ({launches} launches of skel_step a round" + (f", {launches // ops.SKEL_TILE_STEPS} of skel_tile" if has_lds else "") + ")")


def bench(name, lab, a, say):
    lab_d = torch.from_numpy(lab).cuda()
    routes = [r for r in SK.ROUTES if r != "auto"]
    dev = {r: SK.skeletonize_labels(lab_d, route=r) for r in routes}           # warm-up: allocator, code objects
    torch.cuda.synchronize()
    first = dev[routes[0]]
    say(f"{name}: {len(np.unique(lab[lab > 0]))} instances, {100 * (lab > 0).mean():.1f} % of the pixels labelled, {int((first.labels > 0).sum())} skeleton pixels, "
        f"subiterations {first.subiterations}")
    th, td, host = [], {r: [] for r in routes}, None
    for rep in range(a.reps):
        if not a.no_host:
            t0 = time.perf_counter()
            host = SK.skeletonize_labels(lab)
            th.append(time.perf_counter() - t0)
        for r in (routes if rep % 2 == 0 else routes[::-1]):                    # the A/B alternates
            dev[r], t = sync_time(lambda: SK.skeletonize_labels(lab_d, route=r))
            td[r].append(t)
    ok = all(torch.equal(dev[r].labels, first.labels) and dev[r].subiterations == first.subiterations for r in routes)
    for r in routes:
        say(f"  (b) device, route {r:<7s} labels resident, synchronised: runs {fmt(td[r])} s, median {med(td[r]):.6f} s, spread {spread(td[r]):.6f} s")
    if len(routes) == 2:
        say(f"      route A/B (outputs {'IDENTICAL' if ok else 'DIFFERENT'}): " + verdict(td[routes[0]], td[routes[1]], routes[0], routes[1]))
    best = SK.AUTO_ROUTE if len(routes) > 1 else routes[0]
    if th:
        same = torch.equal(first.labels.cpu(), host.labels) and first.subiterations == host.subiterations
        ok = ok and same
        say(f"  (a) host form  numpy definition:                      runs {fmt(th)} s, median {med(th):.6f} s, spread {spread(th):.6f} s")
        say(f"      outputs {'IDENTICAL' if same else 'DIFFERENT'}; against route {best}: " + verdict(th, td[best], "(a)", "(b)"))
    else:
        say("  (a) host form  not measured")
    sk_d = first.labels
    d2_d = D.inner_distance(lab_d)
    k = int(lab.max())
    SK.measure_skeletons(sk_d, num_ids=k, d2=d2_d)
    tm, tmh, mh = [], [], None
    sk_h, d2_h = sk_d.cpu(), d2_d.cpu()
    for _ in range(a.reps):
        if not a.no_host:
            t0 = time.perf_counter()
            mh = SK.measure_skeletons(sk_h, num_ids=k, d2=d2_h)
            tmh.append(time.perf_counter() - t0)
        md, t = sync_time(lambda: SK.measure_skeletons(sk_d, num_ids=k, d2=d2_d))
        tm.append(t)
    say(f"  measure_skeletons with d2, device: runs {fmt(tm)} s, median {med(tm):.6f} s, spread {spread(tm):.6f} s; end points {int(md.end_points.sum())}, "
        f"junctions {int(md.junctions.sum())}, links {int(md.links_orth.sum())} + {int(md.links_diag.sum())} diagonal")
    if tmh:
        same = all(torch.equal(x.cpu(), y) for x, y in zip(md, mh))
        ok = ok and same
        say(f"  measure_skeletons with d2, host:   runs {fmt(tmh)} s, median {med(tmh):.6f} s, spread {spread(tmh):.6f} s; tables {'IDENTICAL' if same else 'DIFFERENT'}; "
            + verdict(tmh, tm, "host", "device"))
    if a.stages:
        stages(lab_d, sk_d, first.subiterations, a.reps, say)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--rmin", type=float, default=20.0)
    ap.add_argument("--rmax", type=float, default=60.0)
    ap.add_argument("--filaments", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form (the device routes alone)")
    ap.add_argument("--stages", action="store_true", help="also time the kernels one by one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"skeletonize_labels: routes {[r for r in SK.ROUTES if r != 'auto']}, auto = {SK.AUTO_ROUTE if 'lds' in SK.ROUTES else 'global'}; {a.reps} alternating rounds after one warm-up call")
    ok = bench(f"label_frame {a.size}^2, {a.cells} cells of radius {a.rmin}..{a.rmax}", S.label_frame(1, a.size, a.size, a.cells, (a.rmin, a.rmax)), a, say)
    ok = bench(f"filament_frame {a.size}^2, {a.filaments} branched filaments", S.filament_frame(1, a.size, a.size, a.filaments), a, say) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
