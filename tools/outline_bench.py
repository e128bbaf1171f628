"""Time utils.outline.label_outlines on the synthetic label frame of tools/distance_bench.py and on one adversarial frame, a single spiral corridor
whose one loop holds nearly all the edges, in one process, the routes alternating:

  (a) the host form: the numpy definition, labels in host memory, after one warm-up call;
  (b) the device route (csrc/outline.hip): labels resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call.

    python tools/outline_bench.py [--size 2048] [--cells 400] [--connectivity 8] [--reps 3] [--stages] [--no-host] [--out profiles/r20_outline.txt]

Prints every run, the medians and the spread (max - min), whether the two routes give identical outputs, the edges / loops / vertices / longest loop
of each frame, and with --stages the device route stage by stage (device events); --out appends the lines to a file.
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
from ullsam_amd.utils import outline as OL  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


def spiral(n: int) -> np.ndarray:
    """One instance: a corridor one pixel wide that winds inwards with one-pixel walls (row and column arithmetic only)."""
    lab = np.zeros((n, n), np.int32)
    for lo in range(1, n // 2, 2):                        # every second ring of the square ...
        hi = n - 1 - lo
        if hi - lo < 2:
            break
        lab[lo, lo:hi + 1] = 1
        lab[hi, lo:hi + 1] = 1
        lab[lo:hi + 1, lo] = 1
        lab[lo:hi + 1, hi] = 1
        if lo > 1:
            lab[lo - 1, lo - 2] = 0                       # ... the ring outside it cut open below its top-left corner
            lab[lo, lo - 1] = 1                           # and its loose end led inwards, onto this ring's corner
    return lab


def stages(lab_d, conn, reps, say):
    """The device route stage by stage through ops, each between two device events."""
    from ullsam_amd import ops
    h, w = lab_d.shape
    k = int(lab_d.max())
    dev = lab_d.device
    times = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        return out

    for _ in range(reps + 1):                             # (the first round is the warm-up)
        flags = torch.zeros((ops.OUTLINE_FLAGS,), dtype=torch.int32, device=dev)
        mask, off, _ = timed("side masks + scan of the counts", lambda: ops.outline_sides(lab_d, k, flags))
        e = timed("read-back: status, E", lambda: flags.cpu().tolist())[1]
        eid, succ, pdir, _ = timed("successors (+ the direction scattered)", lambda: ops.outline_successors(lab_d, mask, off, e, conn, flags))
        leader, rank, _ = timed(f"leader and rank: {max(e - 1, 0).bit_length()} rounds of doubling", lambda: ops.outline_rank(succ, eid, pdir, flags))
        lst, _ = timed("collect the leaders", lambda: ops.outline_collect(lab_d, eid, leader, e // 4 + 1, flags))
        fl = timed("read-back: L, N", lambda: flags.cpu().tolist())

        def tables():
            keys = torch.sort(lst[:fl[3]]).values
            lead = (keys & 0xFFFFFFFF).to(torch.int32)
            loop_of = torch.empty((e,), dtype=torch.int32, device=dev)
            loop_of[lead.long()] = torch.arange(fl[3], dtype=torch.int32, device=dev)
            return keys, lead, loop_of
        keys, lead, loop_of = timed("sort of the L keys, loop_of (torch)", tables)
        edges, area2, _ = timed("edges and area2 per loop (atomics)", lambda: ops.outline_loops(eid, leader, loop_of, fl[3], w, flags))
        estart = timed("offsets of the loops (torch cumsum)", lambda: (torch.cumsum(edges, 0) - edges).to(torch.int32))
        reid, corner, _ = timed("rank-ordered copy", lambda: ops.outline_order(eid, pdir, leader, rank, loop_of, estart, flags))
        coff, _ = timed("scan of the corner flags", lambda: ops.outline_scan(corner))
        timed("vertices (ordered compaction)", lambda: ops.outline_vertices(reid, corner, coff, fl[2], w))
        timed("parents", lambda: ops.outline_parents(lab_d, mask, off, eid, leader, loop_of, lead, area2, flags))
    total = 0.0
    for name, t in times.items():
        ms = med(t[1:])
        total += ms
        say(f"    stage {name:<44s} {ms * 1e3:10.1f} us (spread {spread(t[1:]) * 1e3:8.1f})")
    say(f"    the stages' medians sum to {total * 1e3:.1f} us")


def measure(name, lab, a, say) -> bool:
    lab_d = torch.from_numpy(lab).cuda()
    k = int(lab.max())
    call = lambda x, kw: OL.label_outlines(x, a.connectivity, num=k, **kw)
    dev = call(lab_d, {})                                 # warm-up: allocator, code objects
    torch.cuda.synchronize()
    if not a.no_host:
        call(lab, {"device": "cpu"})                      # and one of the host form: first-touch pages of its arrays
    say(f"{name}: {lab.shape[0]} x {lab.shape[1]}, {len(np.unique(lab[lab > 0]))} ids, {100 * (lab > 0).mean():.1f} % of the pixels labelled; "
        f"connectivity {a.connectivity}: {int(dev.edges.sum())} edges, {dev.label.numel()} loops ({int((dev.area2 < 0).sum())} holes), "
        f"{dev.vertices.shape[0]} vertices, the longest loop {int(dev.edges.max())} edges")
    ta, tb, host = [], [], None
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
    ok = True
    say(f"  (b) device     labels resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s")
    if ta:
        ok = all(d.dtype == h.dtype and torch.equal(d.cpu(), h) for d, h in zip(dev, host))
        gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
        say(f"  (a) host form  numpy definition:              runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
        say(f"      outputs {'IDENTICAL' if ok else 'DIFFERENT'}; (a) / (b) = {med(ta) / med(tb):.1f}x; (a) - (b) = {gap:.6f} s against 3 x the larger spread "
            f"{3 * worse:.6f} s -> {'(b) is faster' if gap > 3 * worse else '(a) is faster' if -gap > 3 * worse else 'no claim'}")
    else:
        say("  (a) host form  not measured")
    if a.stages:
        stages(lab_d, a.connectivity, a.reps, say)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--rmin", type=float, default=20.0)
    ap.add_argument("--rmax", type=float, default=60.0)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form (the device route alone)")
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
