"""Time the per-instance measurements (utils.measure.measure_instances / label_contacts) on synthetic label frames, in one process, the routes
alternating:

  (a) the host form: the numpy route of the same module, labels and image in host memory;
  (b) the device route (csrc/measure.hip) with lds_slots = 0: every run of equal labels straight to the global tables;
  (c) the device route as utils.measure runs it: the per-workgroup LDS table in front (ops.MEASURE_LDS_SLOTS entries).  (b) against (c) is the
      A/B that decided the default.

For (b) and (c) the labels and the image are resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call.  A device
call takes well under a millisecond, and the first one after the host form has kept the GPU idle for seconds was seen to take 0.2 - 0.3 ms
longer whichever route it was: so a timed device run is --calls back-to-back calls (each with its own read-back of the status word), reported
per call, one discarded call stands between the host form and the timed device runs, and (b) and (c) swap their order from round to round.
The frames are utils.synthetic.label_frame: 2048^2 with a uint8 x 3 image, and the mosaic bench's 7424^2 frame (labels only).  Reads nothing
outside the repository.

    python tools/measure_bench.py [--reps 3] [--calls 20] [--small 2048] [--large 7424] [--cells-per-mpx 14]

Prints every run, the medians and the spread (max - min); the outputs of the three routes are asserted identical before any time is printed.
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
from ullsam_amd import ops  # noqa: E402
from ullsam_amd.utils import measure as M  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


def _timed(fn, calls):
    """calls = 0: a host route, once.  Otherwise `calls` back-to-back device calls between two synchronisations, seconds per call."""
    if calls:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(max(calls, 1)):
        out = fn()
    if calls:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / max(calls, 1), out


def _tensors(t):
    return [x for x in t if x is not None] if isinstance(t, tuple) else [t]


def _line(tag, what, t):
    print(f"({tag}) {what}: runs {fmt(t)} s, median {med(t):.6f} s, spread {spread(t):.6f} s", flush=True)


def _verdict(name_a, ta, name_b, tb):
    """The rule of profiles/r14_interactive.txt: a difference counts only where it exceeds three times the larger spread."""
    diff, bar = med(ta) - med(tb), 3 * max(spread(ta), spread(tb))
    if abs(diff) > bar:
        fast, slow = (name_b, name_a) if diff > 0 else (name_a, name_b)
        return f"{fast} is faster than {slow}: {max(med(ta), med(tb)) / min(med(ta), med(tb)):.2f}x (difference {abs(diff):.6f} s > 3 x the larger spread = {bar:.6f} s)"
    return f"no difference between {name_a} and {name_b} by the rule (difference {abs(diff):.6f} s <= 3 x the larger spread = {bar:.6f} s)"


def run(side: int, n_cells: int, channels: int, reps: int, calls: int):
    t0 = time.perf_counter()
    lab = S.label_frame(1, side, side, n_cells)
    k = int(lab.max())
    img = None
    if channels:
        img = np.random.default_rng(7).integers(0, 256, (side, side, channels)).astype(np.uint8)
    print(f"--- {side}^2 frame ({side * side / 1e6:.1f} M pixels), {n_cells} discs drawn, K = {k}, {(lab > 0).mean() * 100:.0f} % foreground, "
          f"image {'none' if img is None else f'uint8 x {channels}'} (built in {time.perf_counter() - t0:.1f} s)", flush=True)
    lab_d = torch.from_numpy(lab).cuda()
    img_d = None if img is None else torch.from_numpy(img).cuda()
    routes = {
        "a": (lambda: M.measure_instances(lab, img, num=k), 0),
        "b": (lambda: M.measure_instances(lab_d, img_d, num=k, device="cuda", lds_slots=0), calls),
        "c": (lambda: M.measure_instances(lab_d, img_d, num=k, device="cuda", lds_slots=ops.MEASURE_LDS_SLOTS), calls),
        "pa": (lambda: M.label_contacts(lab, num=k), 0),
        "pb": (lambda: M.label_contacts(lab_d, num=k, device="cuda"), calls),
    }
    for name in ("b", "c", "pb"):                                                    # warm-up: allocator, code objects
        routes[name][0]()
    times = {n: [] for n in routes}
    outs = {}
    for r in range(reps):
        order = ("a", "pa", None, "b", "c", "pb") if r % 2 == 0 else ("a", "pa", None, "c", "b", "pb")
        for name in order:
            if name is None:                                                         # the GPU sat idle during the host form: one discarded call
                routes["b"][0]()
                continue
            dt, outs[name] = _timed(*routes[name])
            times[name].append(dt)
        print(f"    round {r + 1} of {reps} done ({' '.join(n for n in order if n)})", flush=True)
    for dev_name in ("b", "c"):
        for g, w_ in zip(_tensors(outs[dev_name]), _tensors(outs["a"])):
            assert g.dtype == w_.dtype and torch.equal(g.cpu(), w_), f"route ({dev_name}) differs from the host form"
    assert torch.equal(outs["pb"].cpu(), outs["pa"]), "the device contact list differs from the host form"
    print("identical outputs: (a) == (b) == (c) for every table, contact list (host) == (device): IDENTICAL")
    _line("a", "measure_instances, host form (numpy), host memory        ", times["a"])
    _line("b", f"measure_instances, device, lds_slots = 0 (direct), resident, per call of {calls}", times["b"])
    _line("c", f"measure_instances, device, LDS table of {ops.MEASURE_LDS_SLOTS} slots, resident, per call of {calls}", times["c"])
    print("    " + _verdict("(a) host", times["a"], "(c) device", times["c"]))
    print("    LDS table A/B: " + _verdict("(b) direct", times["b"], "(c) LDS table", times["c"]))
    _line("pa", f"label_contacts, host form (numpy), {len(outs['pa'])} pairs             ", times["pa"])
    _line("pb", f"label_contacts, device (its own launch), resident, per call of {calls}", times["pb"])
    print("    " + _verdict("(pa) host", times["pa"], "(pb) device", times["pb"]))
    px = side * side
    nbytes = 4 * px * 3 + (0 if img is None else int((lab > 0).sum()) * channels)
    print(f"    algorithmic bytes of (c): 4 B x H*W x 3 (the row and its two neighbour rows; the neighbours mostly hit in cache) + {channels} B per foreground pixel "
          f"= at most {nbytes / 1e6:.0f} MB = {nbytes / 8e12 * 1e6:.0f} us at 8 TB/s; measured {med(times['c']) * 1e6:.0f} us (allocation of the tables, init launch and the read-back of the status word included)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed device run (reported per call)")
    ap.add_argument("--small", type=int, default=2048)
    ap.add_argument("--large", type=int, default=7424, help="the mosaic bench's frame: 4 x 4 tiles of 2048^2, overlap 256")
    ap.add_argument("--cells-per-mpx", type=float, default=14.0, help="discs per 2^20 pixels (label_tile's default density on a 1024^2 tile)")
    a = ap.parse_args()
    for side, channels in ((a.small, 3), (a.large, 0)):
        if side > 0:
            run(side, int(round(a.cells_per_mpx * side * side / 2 ** 20)), channels, a.reps, max(a.calls, 1))


if __name__ == "__main__":
    main()
