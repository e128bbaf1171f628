"""Time utils.simplify.simplify_outlines on the synthetic label frame of tools/distance_bench.py and on the spiral corridor of tools/outline_bench.py,
at tolerances of 0.5 and 2 pixels, in one process, the routes alternating:

  (a) the host form: the numpy definition, labels in host memory, after one warm-up call;
  (b) the device route (csrc/simplify.hip): labels resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call.

    python tools/simplify_bench.py [--size 2048] [--cells 400] [--connectivity 8] [--reps 3] [--stages] [--no-host] [--out profiles/r22_simplify.txt]

Prints every run, the medians and the spread (max - min), whether the routes give identical outputs, the vertices before and after and the rounds
taken, and with --stages the device route stage by stage (device events); --out appends the lines to a file.
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
from ullsam_amd.utils import simplify as SM  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)
TOLERANCES = (0.5, 2.0)


def stages(lab_d, conn, tol, reps, say):
    """The device route stage by stage through ops, each between two device events (label_outlines' stages as one)."""
    from ullsam_amd import ops
    h, w = lab_d.shape
    k, t, dev = int(lab_d.max()), SM._tolerance(tol), lab_d.device
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
        src, reid, corner, estart, _ = timed("label_outlines' stages up to the rank-ordered copy, parents", lambda: SM._ordered_device(lab_d, k, conn))
        flags = torch.zeros((ops.SIMPLIFY_FLAGS,), dtype=torch.int32, device=dev)
        cand, _ = timed("fixed-point and candidate flags", lambda: ops.simplify_flags(lab_d, reid, corner, flags))
        coff, total = timed("scan of the candidate flags", lambda: ops.outline_scan(cand))
        cstart = timed("offsets of the loops' candidates (torch)", lambda: torch.cat([coff[estart.long()], total]))
        n_cand = timed("read-back: C", lambda: int(total.cpu()))
        cxy, cloop, kept, nfixed, _ = timed("candidates (compaction, loop search)", lambda: ops.simplify_candidates(reid, cand, coff, estart, n_cand, h, w, flags))
        timed("anchors (64-bit atomics per loop)", lambda: ops.simplify_anchors(cxy, cloop, nfixed, kept, flags))
        pa, pb, _ = timed("segments (scan of kept, neighbours)", lambda: ops.simplify_segments(kept, cloop, cstart, flags))

        def rounds():
            block, n = SM.ROUND_BLOCK, 0
            while True:
                got = ops.simplify_rounds(cxy, cloop, cstart, t, block, pa, pb, kept, flags)[0].cpu().tolist()
                n += sum(1 for v in got if v)
                if got[-1] == 0:
                    return n
                block = min(2 * block, SM.ROUND_BLOCK_MAX)
        n_rounds = timed("the rounds (with their read-backs)", rounds)
        voff, total = timed("scan of the kept flags", lambda: ops.outline_scan(kept))
        n_vert = timed("read-back: N", lambda: int(total.cpu()))
        out = timed("rings (vertices, count and area2 per loop)", lambda: ops.simplify_rings(cxy, cloop, kept, voff, total, cstart, n_vert, flags))
        timed("surviving loops, re-indexed tables (torch)", lambda: SM._finish(src, out[0], cloop[kept.bool()], out[1], out[2], k))
    total_ms = 0.0
    for name, ts in times.items():
        ms = med(ts[1:])
        total_ms += ms
        say(f"    stage {name:<60s} {ms * 1e3:10.1f} us (spread {spread(ts[1:]) * 1e3:8.1f})")
    say(f"    the stages' medians sum to {total_ms * 1e3:.1f} us; {n_rounds} rounds")


def measure(name, lab, tol, a, say) -> bool:
    lab_d = torch.from_numpy(lab).cuda()
    k = int(lab.max())
    call = lambda x, kw: SM._run(x, tol, a.connectivity, num=k, **kw)
    dev, info = call(lab_d, {})                           # warm-up: allocator, code objects
    torch.cuda.synchronize()
    if not a.no_host:
        call(lab, {"device": "cpu"})                      # and one of the host form: first-touch pages of its arrays
    say(f"{name}: {lab.shape[0]} x {lab.shape[1]}, {len(np.unique(lab[lab > 0]))} ids; connectivity {a.connectivity}, tolerance {tol} px: "
        f"{info['vertices']} vertices in {info['loops']} loops before, {info['candidates']} candidates, {dev.outlines.vertices.shape[0]} vertices in "
        f"{dev.source.numel()} loops after, {info['rounds']} rounds")
    ta, tb, host = [], [], None
    for _ in range(a.reps):
        if not a.no_host:
            t0 = time.perf_counter()
            host = call(lab, {"device": "cpu"})[0]
            ta.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = call(lab_d, {})[0]
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t0)
    ok = True
    say(f"  (b) device     labels resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s")
    if ta:
        ok = all(x.dtype == y.dtype and torch.equal(x.cpu(), y) for x, y in zip(list(dev.outlines) + [dev.source], list(host.outlines) + [host.source]))
        gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
        say(f"  (a) host form  numpy definition:              runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
        say(f"      outputs {'IDENTICAL' if ok else 'DIFFERENT'}; (a) / (b) = {med(ta) / med(tb):.1f}x; (a) - (b) = {gap:.6f} s against 3 x the larger spread "
            f"{3 * worse:.6f} s -> {'(b) is faster' if gap > 3 * worse else '(a) is faster' if -gap > 3 * worse else 'no claim'}")
    else:
        say("  (a) host form  not measured")
    if a.stages:
        stages(lab_d, a.connectivity, tol, a.reps, say)
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

    ok = True
    cells = S.label_frame(1, a.size, a.size, a.cells, (a.rmin, a.rmax))
    for tol in TOLERANCES:
        ok = measure(f"label_frame, {a.cells} cells of radius {a.rmin}..{a.rmax}", cells, tol, a, say) and ok
    for tol in TOLERANCES:
        ok = measure("one spiral corridor", spiral(a.size), tol, a, say) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
