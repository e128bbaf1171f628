"""Time the per-object measurements of utils.measure3d on a synthetic sphere stack linked on the device, in one process, the routes alternating:

  (a) the host form: the numpy definition, on a SUB-VOLUME (--host-sub planes side; the first planes, the top-left corner) small enough to finish,
      against the device route on the same sub-volume; the outputs must be identical (the exit status says so);
  (b) the device route (csrc/measure3d.hip) on the whole volume: resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up
      call, with lds_slots = 128 (the per-workgroup LDS table) and lds_slots = 0 (every run straight to the global tables) -- the one A/B;
  --stages: the entry points through ops between two device events, beside the time of their bytes at 8 TB/s (4 B per voxel for the labels plus
      C * sample_bytes for the image; the neighbour rows and planes are expected from the caches).

The volume is utils.synthetic.label_stack (default 32 x 2048^2, dz = 2.5) linked by utils.stack.link_label_stack(device="cuda"); the image is
uint8 x 3.  A claim is made only where the medians differ by more than 3 x the larger spread (max - min).

    python tools/measure3d_bench.py [--planes 32] [--size 2048] [--cells 6000] [--reps 3] [--stages] [--no-host] [--out profiles/r25_measure3d.txt]
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
from ullsam_amd.utils import measure3d as M  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402
from ullsam_amd.utils.stack import link_label_stack  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


def _tensors(out):
    return [t for t in out if t is not None] if isinstance(out, tuple) else [out]


def _claim(ta, tb, a, b):
    gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
    verdict = "no claim (one run)" if min(len(ta), len(tb)) < 2 else f"{b} is faster" if gap > 3 * worse else f"{a} is faster" if -gap > 3 * worse else "no claim"
    return f"{a} / {b} = {med(ta) / med(tb):.2f}x; {a} - {b} = {gap:.6f} s against 3 x the larger spread {3 * worse:.6f} s -> {verdict}"


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stages(vol_d, img_d, k, reps, say):
    """The entry points through ops, each between two device events (the init kernels and, for the contacts, the compaction included)."""
    from ullsam_amd import ops
    n = vol_d.numel()
    max_pairs = 1 << 20
    cap = ops.mosaic_table_slots(max_pairs)
    times = {}

    def timed(name, nbytes, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault((name, nbytes), []).append(e0.elapsed_time(e1))
        return out

    for _ in range(reps + 1):                            # (the first round is the warm-up)
        for slots in (128, 0):
            timed(f"measure_objects3d, no image, lds_slots = {slots}", 4 * n, lambda: ops.measure_objects3d(vol_d, k, None, slots))
            timed(f"measure_objects3d, uint8 x 3, lds_slots = {slots}", 7 * n, lambda: ops.measure_objects3d(vol_d, k, img_d, slots))
        timed(f"object_contacts3d, max_pairs = 2^20 (table of {cap} slots set and read)", 4 * n + 2 * 32 * cap, lambda: ops.object_contacts3d(vol_d, k, max_pairs))
    for (name, nbytes), t in times.items():
        ms = med(t[1:])
        say(f"    stage {name:<78s} {ms * 1e3:11.1f} us (spread {spread(t[1:]) * 1e3:9.1f}); {nbytes / 1e6:8.1f} MB = {nbytes / 8e12 * 1e6:7.1f} us at 8 TB/s: "
            f"x{ms * 1e-3 / max(nbytes / 8e12, 1e-12):.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=6000, help="spheres drawn in the stack's volume")
    ap.add_argument("--rmin", type=float, default=12.0)
    ap.add_argument("--rmax", type=float, default=40.0)
    ap.add_argument("--dz", type=float, default=2.5, help="plane spacing in pixels")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sub", type=int, nargs=2, default=(8, 384), help="planes and side of the sub-volume the numpy host form runs on")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form (the device route alone)")
    ap.add_argument("--stages", action="store_true", help="also time the entry points between device events")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    planes, counts = S.label_stack(1, a.planes, a.size, a.size, a.cells, (a.rmin, a.rmax), a.dz)
    vol_d = link_label_stack(torch.from_numpy(planes).cuda(), counts, device="cuda")[0]
    del planes
    k = int(vol_d.max())
    rng = np.random.default_rng(5)
    img_d = torch.from_numpy(rng.integers(0, 256, (a.planes, a.size, a.size, 3), dtype=np.uint8)).cuda()
    labelled = float((vol_d > 0).float().mean())
    say(f"label_stack {a.planes} x {a.size}^2, {a.cells} spheres of radius {a.rmin}..{a.rmax}, dz = {a.dz}, linked on the device: K = {k} objects, "
        f"{100 * labelled:.1f} % of the {vol_d.numel()} voxels labelled; image uint8 x 3")
    sp, ss = min(a.host_sub[0], a.planes), min(a.host_sub[1], a.size)
    sub_d, simg_d = vol_d[:sp, :ss, :ss].contiguous(), img_d[:sp, :ss, :ss].contiguous()
    sub, simg = sub_d.cpu().numpy(), simg_d.cpu().numpy()
    ok = True
    calls = [("measure_objects, no image", lambda v, i, kw: M.measure_objects(v, None, num=k, **kw)),
             ("measure_objects, uint8 x 3", lambda v, i, kw: M.measure_objects(v, i, num=k, **kw)),
             ("object_contacts", lambda v, i, kw: M.object_contacts(v, num=k, **{n: x for n, x in kw.items() if n != "lds_slots"}))]
    for name, fn in calls:
        ab = name != "object_contacts"
        fn(vol_d, img_d, {"lds_slots": 128})             # warm-up: allocator, code objects
        fn(vol_d, img_d, {"lds_slots": 0})
        fn(sub_d, simg_d, {})
        th, ts, t128, t0, host, dsub = [], [], [], [], None, None
        for _ in range(a.reps):                          # the routes alternate within a round
            if not a.no_host:
                t, host = _timed(lambda: fn(sub, simg, {"device": "cpu"}))
                th.append(t)
                t, dsub = _timed(lambda: fn(sub_d, simg_d, {}))
                ts.append(t)
            t, d128 = _timed(lambda: fn(vol_d, img_d, {"lds_slots": 128}))
            t128.append(t)
            if ab:
                t, d0 = _timed(lambda: fn(vol_d, img_d, {"lds_slots": 0}))
                t0.append(t)
                ok = ok and all(torch.equal(x, y) for x, y in zip(_tensors(d128), _tensors(d0)))
        say(f"{name}")
        say(f"  (b) device     whole volume resident, synchronised{', lds_slots = 128' if ab else ''}: runs {fmt(t128)} s, median {med(t128):.6f} s, spread "
            f"{spread(t128):.6f} s ({vol_d.numel() / med(t128) / 1e9:.2f} G voxels / s)")
        if ab:
            say(f"      lds_slots = 0: runs {fmt(t0)} s, median {med(t0):.6f} s, spread {spread(t0):.6f} s; the same tables; "
                f"A/B {_claim(t0, t128, 'direct', 'table')}")
        if th:
            same = all(torch.equal(d.cpu(), h) for d, h in zip(_tensors(dsub), _tensors(host)))
            ok = ok and same
            say(f"  (a) host form  numpy definition on the sub-volume {sp} x {ss} x {ss}: runs {fmt(th)} s, median {med(th):.6f} s, spread {spread(th):.6f} s")
            say(f"      device on the same sub-volume: runs {fmt(ts)} s, median {med(ts):.6f} s, spread {spread(ts):.6f} s; outputs "
                f"{'IDENTICAL' if same else 'DIFFERENT'}; {_claim(th, ts, '(a)', '(b)')}")
        else:
            say("  (a) host form  not measured")
    if a.stages:
        stages(vol_d, img_d, k, a.reps, say)
    say("not built: an LDS-staged tile with halo (the neighbour rows and planes come through the caches)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    assert ok, "the routes disagree"
    return 0


if __name__ == "__main__":
    sys.exit(main())
