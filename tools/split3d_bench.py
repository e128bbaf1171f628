"""Time utils.split3d.split_labels3d on the volume of tools/distance3d_bench.py -- a synthetic sphere stack (utils.synthetic.label_stack, default
32 x 2048^2, dz = 2.5, spacing (5, 2, 2)) linked ON THE DEVICE by utils.stack.link_label_stack(mode="all"), which fuses spheres that overlap from
plane to plane: the objects the split exists for --, in one process, the routes alternating:

  (a) the host form: the numpy definition, on a SUB-VOLUME (--host-sub planes side; the first planes, the top-left corner) small enough to finish,
      against the device route on the same sub-volume, identical outputs asserted;
  (b) the device route on the whole volume: resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call, once per
      route of the ascent ("auto", "lds", "global"), the routes alternating within every round.

    python tools/split3d_bench.py [--planes 32] [--size 2048] [--cells 6000] [--depth 2] [--reps 3] [--stages] [--no-host] [--out profiles/r24_split3d.txt]

Prints every run, the medians and the spread (max - min), the basins / pairs / rounds / parts of the volume, how many objects the linking fused and
how many the split cut, the peak device memory of a call, and with --stages the device route stage by stage (device events) with the LDS / global
A/B of the ascent and the bytes the ascent and the passes have to move at 8 TB/s; --out appends the lines to a file.  A difference is claimed only
above 3 x the larger spread.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ullsam_amd import _lib  # noqa: E402
from ullsam_amd.utils import split3d as SP  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402
from ullsam_amd.utils.stack import link_label_stack  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


def _claim(ta, tb, a, b):
    gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
    verdict = f"{b} is faster" if gap > 3 * worse else f"{a} is faster" if -gap > 3 * worse else "no claim"
    return f"{a} / {b} = {med(ta) / med(tb):.2f}x; {a} - {b} = {gap:.6f} against 3 x the larger spread {3 * worse:.6f} -> {verdict}"


def stages(vol_d, s, depth, max_pairs, reps, say):
    """The device route stage by stage through ops, each between two device events (milliseconds); the first round is the warm-up."""
    from ullsam_amd import ops
    n = vol_d.numel()
    k = int(vol_d.max())
    e = (False, False, False)
    times = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        return out

    def distance():
        g, _, _ = ops.distance3d_z(vol_d, False, False, num=k)
        hy, _ = ops.distance3d_y(vol_d, g, None, s, e)
        return ops.distance3d_x(vol_d, hy, None, "inner", s, e, num=k)[0]

    def merge(keys, vals, d2, up, best):
        rounds = 0
        while True:
            changed = torch.zeros((1,), dtype=torch.int32, device=vol_d.device)
            ops.split_round(keys, vals, vol_d, d2, up, depth, best, changed, k)
            if not int(changed.cpu()):
                return rounds
            ops.split_flatten(up)
            rounds += 1

    def collect(up):
        parts = int(ops.split_collect(vol_d, up, None, k)[4].cpu())
        return torch.sort(ops.split_collect(vol_d, up, parts, k)[0]).values

    for rep in range(reps + 1):
        d2 = timed("distance (z, y, x passes, inner)", distance)
        for route in (("lds", "global") if rep % 2 == 0 else ("global", "lds")):      # alternating
            up = timed(f"ascent, {route}", lambda: ops.split3d_ascent(vol_d, d2, k, route)[0])
        timed("first flatten", lambda: ops.split_flatten(up))
        keys, vals, _ = timed("passes (13 forward neighbours, pair table)", lambda: ops.split3d_passes(vol_d, d2, up, max_pairs, k))
        best = torch.zeros((n,), dtype=torch.int64, device=vol_d.device)
        timed("rounds until rest (best + decide, one read-back, flatten)", lambda: merge(keys, vals, d2, up, best))
        del best
        lst = timed("collect (count, read-back, list, sort)", lambda: collect(up))
        timed("relabel (tables + every voxel)", lambda: ops.split3d_relabel(lst, vol_d, d2, up, k))
        del d2, up, keys, vals, lst
    for name, t in times.items():
        say(f"    stage {name:<62s} {med(t[1:]):9.3f} ms (spread {spread(t[1:]):7.3f}); runs {', '.join(f'{x:.3f}' for x in t[1:])}")
    tl, tg = times["ascent, lds"][1:], times["ascent, global"][1:]
    say(f"    ascent A/B (ms): {_claim(tg, tl, 'global', 'lds')}")
    for name in ("ascent, lds", "ascent, global", "passes (13 forward neighbours, pair table)"):
        ms, nbytes = med(times[name][1:]), 12 * n          # labels, D2 read, up written / labels, D2, up read: 12 bytes a voxel, neighbours from the caches
        say(f"    {name}: {nbytes / 1e6:.1f} MB = {nbytes / 8e12 * 1e3:.3f} ms at 8 TB/s: x{ms * 1e-3 / (nbytes / 8e12):.1f}")
    dearest = max(times, key=lambda m: med(times[m][1:]))
    say(f"    the dearest stage: {dearest}, {med(times[dearest][1:]):.3f} ms of {sum(med(t[1:]) for m, t in times.items() if m != 'ascent, global'):.3f} ms "
        f"(all stages, the ascent counted once)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=6000, help="spheres drawn in the stack's volume")
    ap.add_argument("--rmin", type=float, default=12.0)
    ap.add_argument("--rmax", type=float, default=40.0)
    ap.add_argument("--dz", type=float, default=2.5, help="plane spacing in pixels")
    ap.add_argument("--spacing", type=int, nargs=3, default=(5, 2, 2), help="(sz, sy, sx): integers in the ratio dz : 1 : 1")
    ap.add_argument("--depth", type=int, default=2, help="min_depth, in spacing units (2 = one pixel of xy at the default spacing)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sub", type=int, nargs=2, default=(8, 384), help="planes and side of the sub-volume the numpy host form runs on")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form (the device route alone)")
    ap.add_argument("--stages", action="store_true", help="also time the device route stage by stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = tuple(a.spacing)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    planes, counts = S.label_stack(1, a.planes, a.size, a.size, a.cells, (a.rmin, a.rmax), a.dz)
    planes_d = torch.from_numpy(planes).cuda()
    del planes
    mutual = link_label_stack(planes_d, counts, device="cuda")[0]
    present = lambda v: int((torch.bincount(v.reshape(-1))[1:] > 0).sum())
    n_mutual = present(mutual)
    del mutual
    vol_d = link_label_stack(planes_d, counts, mode="all", device="cuda")[0]
    del planes_d
    n = vol_d.numel()
    k = int(vol_d.max())
    n_all = present(vol_d)
    say(f"label_stack {a.planes} x {a.size}^2, {a.cells} spheres of radius {a.rmin}..{a.rmax}, dz = {a.dz}, linked on the device with mode=\"all\": "
        f"{n_all} objects ({n_mutual} under mode=\"mutual\": the linking fused {n_mutual - n_all} more), {100 * float((vol_d > 0).float().mean()):.1f} % of the {n} "
        f"voxels labelled; spacing {s}, min_depth {a.depth}")

    max_pairs = 1 << 20
    while True:                                           # (the default capacity, doubled until the volume's pairs fit; said below)
        try:
            st = {}
            parts = SP.split_labels3d(vol_d, a.depth, s, num=k, max_pairs=max_pairs, stats=st)
            break
        except _lib.UllsamError as err:
            if "max_pairs" not in str(err) or max_pairs >= 1 << 30:
                raise
            max_pairs *= 2
    cut = int((parts.parts_of > 1).sum())
    say(f"stats: basins {st['basins']}, pairs {st['pairs']}, rounds {st['rounds']}, parts {st['parts']}; {cut} of the {n_all} objects are cut into "
        f"{int(parts.parts_of[parts.parts_of > 1].sum())} parts; max_pairs = {max_pairs}"
        f"{' (the default holds the pairs)' if max_pairs == 1 << 20 else ' (the default 1 << 20 does NOT hold the pairs)'}")
    del parts
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    SP.split_labels3d(vol_d, a.depth, s, num=k, max_pairs=max_pairs)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    say(f"peak device memory of one call, beyond the resident volume: {peak / 1e6:.1f} MB = {peak / n:.1f} bytes a voxel "
        f"({(peak + 4 * n) / n:.1f} with the volume's own 4)")

    routes = ("auto", "lds", "global")
    t = {r: [] for r in routes}
    for rep in range(a.reps):
        for r in (routes if rep % 2 == 0 else routes[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            SP.split_labels3d(vol_d, a.depth, s, num=k, max_pairs=max_pairs, route=r)
            torch.cuda.synchronize()
            t[r].append(time.perf_counter() - t0)
    for r in routes:
        say(f"  (b) device, route {r:<6s} whole volume resident, synchronised: runs {fmt(t[r])} s, median {med(t[r]):.6f} s, spread {spread(t[r]):.6f} s "
            f"({n / med(t[r]) / 1e9:.2f} G voxels / s)")
    say(f"      whole call (s): {_claim(t['global'], t['lds'], 'global', 'lds')}")

    ok = True
    if not a.no_host:
        sp, ss = min(a.host_sub[0], a.planes), min(a.host_sub[1], a.size)
        sub_d = vol_d[:sp, :ss, :ss].contiguous()
        sub = sub_d.cpu().numpy()
        SP.split_labels3d(sub_d, a.depth, s, num=k)
        ta, ts, host, dsub = [], [], None, None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            host = SP.split_labels3d(sub, a.depth, s, num=k, device="cpu")
            ta.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dsub = SP.split_labels3d(sub_d, a.depth, s, num=k)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ok = all(torch.equal(d.cpu(), h) for d, h in zip(dsub, host))
        say(f"  (a) host form  numpy definition on the sub-volume {sp} x {ss} x {ss} ({int(host.parent.numel())} parts): runs {fmt(ta)} s, median {med(ta):.6f} s, "
            f"spread {spread(ta):.6f} s")
        say(f"      device on the same sub-volume: runs {fmt(ts)} s, median {med(ts):.6f} s, spread {spread(ts):.6f} s; outputs "
            f"{'IDENTICAL' if ok else 'DIFFERENT'}; {_claim(ta, ts, '(a)', '(b)')}")
    else:
        say("  (a) host form  not measured")
    if a.stages:
        stages(vol_d, s, a.depth, max_pairs, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    assert ok, "the host form and the device route differ on the sub-volume"
    return 0


if __name__ == "__main__":
    sys.exit(main())
