"""Time the stack linking (utils.stack.link_label_stack) on a synthetic sphere stack, in one process, the two routes alternating:

  (a) the host form: the numpy definition, planes in host memory;
  (b) the device route (csrc/stack.hip): planes resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call.

The stack is utils.synthetic.label_stack: spheres cut by planes, every plane numbering the cells it sees by a permutation of its own (default 32
planes of 2048^2 = 134 M voxels) -- what 32 generate_label_map calls would leave behind.

    python tools/stack_bench.py [--planes 32] [--size 2048] [--cells 6000] [--reps 3] [--mode mutual] [--max-pairs 1048576] [--stages] [--out profiles/r17_stack.txt]

Prints every run, the medians and the spread (max - min), and whether the two routes give identical outputs; --out also writes the lines to a file.
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
from ullsam_amd.utils import stack as K  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402


def stages(planes_d, counts, iou, mode, reps, max_pairs):
    """The device route stage by stage through ops, each between two device events: ([(name, median milliseconds)], distinct pairs in the table)."""
    from ullsam_amd import ops
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    g = int(base[-1])
    base_d = torch.from_numpy(base).cuda()
    times = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        return out

    for _ in range(reps + 1):                            # (the first round is the warm-up)
        keys, cnt, areas, flags = timed("pairs (zero-fill + one pass)", lambda: ops.stack_pairs(planes_d, base_d, g, max_pairs))
        if mode == "mutual":
            succ, pred, _ = timed("best partner", lambda: ops.stack_best(keys, cnt, areas, g, iou))
            parent, _ = timed("link (chain walk)", lambda: ops.stack_link(g, succ=succ, pred=pred))
        else:
            parent, _ = timed("link (union-find)", lambda: ops.stack_link(g, keys=keys, counts=cnt, areas=areas, iou=iou))
        vox, zr, bx, _ = timed("stats", lambda: ops.stack_stats(planes_d, base_d, g, parent))
        log = timed("compact", lambda: ops.stack_compact(vox, zr, bx, parent))[0]
        timed("relabel", lambda: ops.stack_relabel(planes_d, base_d, g, log))
    return [(name, statistics.median(t[1:])) for name, t in times.items()], int(flags[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=6000, help="spheres drawn in the stack's volume")
    ap.add_argument("--rmin", type=float, default=12.0)
    ap.add_argument("--rmax", type=float, default=40.0)
    ap.add_argument("--dz", type=float, default=4.0, help="plane spacing in pixels")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", default="mutual", choices=K.MODES)
    ap.add_argument("--iou", type=int, nargs=2, default=(1, 4))
    ap.add_argument("--max-pairs", type=int, default=1 << 20, help="the pair table takes this many distinct pairs (its slots: the power of two >= twice that)")
    ap.add_argument("--stages", action="store_true", help="also time the device route stage by stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    planes, counts = S.label_stack(1, a.planes, a.size, a.size, a.cells, (a.rmin, a.rmax), a.dz)
    say(f"{a.planes} planes of {a.size}^2 ({planes.size / 1e6:.1f} M voxels), {a.cells} spheres of radius {a.rmin}..{a.rmax}, planes {a.dz} pixels apart: "
        f"{sum(counts)} per-plane labels in all (built in {time.perf_counter() - t0:.1f} s); iou = {tuple(a.iou)}, mode = {a.mode}, max_pairs = {a.max_pairs}")
    kw = dict(iou=tuple(a.iou), mode=a.mode, max_pairs=a.max_pairs)
    planes_d = torch.from_numpy(planes).cuda()
    dev = K.link_label_stack(planes_d, counts, device="cuda", **kw)                # warm-up: allocator, code objects
    torch.cuda.synchronize()
    ta, tb = [], []
    host = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        host = K.link_label_stack(planes, counts, device="cpu", **kw)
        ta.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = K.link_label_stack(planes_d, counts, device="cuda", **kw)
        torch.cuda.synchronize()
        tb.append(time.perf_counter() - t0)
    same = [bool(torch.equal(d.cpu(), h)) for d, h in zip(dev, host)]
    med = lambda t: statistics.median(t)
    spread = lambda t: max(t) - min(t)
    fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)
    say(f"{len(dev[2])} objects in the volume; the longest spans {int((dev[3][:, 1] - dev[3][:, 0]).max()) + 1 if len(dev[3]) else 0} planes")
    say(f"(a) host form    numpy definition, planes in host memory:         runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
    say(f"(b) device       link_label_stack, planes resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s")
    say(f"identical outputs (volume, label_of_global, voxels, zrange, boxes): {same} -> {'IDENTICAL' if all(same) else 'DIFFERENT'}")
    say(f"(a) / (b) = {med(ta) / med(tb):.1f}x; (a) - (b) = {med(ta) - med(tb):.4f} s against (a)'s spread {spread(ta):.4f} s")
    vox = planes.size
    nbytes = 8 * vox + 4 * vox + 8 * vox
    say(f"algorithmic bytes of (b): 8 B x voxels (pairs: every plane read as z and as z + 1) + 4 B x voxels (stats) + 8 B x voxels (relabel read + write) "
        f"= {nbytes / 1e6:.0f} MB = {nbytes / 8e12 * 1e6:.0f} us at 8 TB/s; measured {med(tb) * 1e6:.0f} us (upload of the bases, launches and the read-back included)")
    if a.stages:
        per_stage, npairs = stages(planes_d, counts, tuple(a.iou), a.mode, a.reps, a.max_pairs)
        say(f"    {npairs} distinct pairs in a table of {2 * a.max_pairs if a.max_pairs & (a.max_pairs - 1) == 0 else '>= ' + str(2 * a.max_pairs)} slots")
        for name, ms in per_stage:
            say(f"    stage {name:<34s} {ms * 1e3:9.1f} us (median of {a.reps}, device events around the launches of the stage)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(same) else 1


if __name__ == "__main__":
    sys.exit(main())
