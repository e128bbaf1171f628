"""Time the surface meshes and Euler numbers of utils.mesh3d on a synthetic sphere stack linked on the device, in one process, the routes alternating:

  (a) the host form: the numpy definition, on a SUB-VOLUME (--host-sub planes side; the first planes, the top-left corner) small enough to finish,
      against the device route on the same sub-volume; the outputs must be identical (the exit status says so);
  (b) the device route (csrc/mesh3d.hip) on the whole volume: resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up
      call: label_surfaces, label_surfaces(only = 16 ids) and object_topology;
  --stages: the entry points through ops and the two torch.sort calls between two device events, beside the time of their bytes at 8 TB/s.

The volume is utils.synthetic.label_stack (default 32 x 2048^2, dz = 2.5) linked by utils.stack.link_label_stack(device="cuda").  A claim is made
only where the medians differ by more than 3 x the larger spread (max - min).  profiles/r26_mesh3d.txt also holds the one A/B this tool was built
for: the face masks with a voxel's six neighbours read from global memory ("global") against the tile and its halo staged in LDS ("staged").  The
staged form did not win and was taken out of the library with its side of this tool, so those lines cannot be produced again from this tree.

    python tools/mesh3d_bench.py [--planes 32] [--size 2048] [--cells 6000] [--reps 3] [--stages] [--no-host] [--out profiles/r26_mesh3d.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ullsam_amd.utils import mesh3d as M  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402
from ullsam_amd.utils.stack import link_label_stack  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


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


def stages(vol_d, k, reps, say):
    """The entry points through ops and the two sorts, each between two device events, in the order label_surfaces calls them."""
    from ullsam_amd import ops
    n = vol_d.numel()
    z, h, w = vol_d.shape
    times = {}

    def timed(name, nbytes, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.setdefault(name, (nbytes, []))[1].append(e0.elapsed_time(e1))
        return out

    tiles = ops.mesh3d_tiles(z, h, w)
    for _ in range(reps + 1):                            # (the first round is the warm-up)
        masks, offsets, _ = timed("mesh3d_masks (masks, tile counts and scan)", 5 * n + 12 * tiles, lambda: ops.mesh3d_masks(vol_d, k))
        f = int(offsets[-1])
        raw = timed("mesh3d_faces", n + 12 * f + 8 * tiles, lambda: ops.mesh3d_faces(vol_d, masks, offsets, f))
        fkeys = timed("torch.sort of the face keys (plumbing)", 16 * f, lambda: torch.sort(raw).values)
        craw = timed("mesh3d_corners", 40 * f, lambda: ops.mesh3d_corners(fkeys, h, w))
        corners = timed("torch.sort of the corner keys (plumbing)", 64 * f, lambda: torch.sort(craw).values)
        del craw
        boff = timed("mesh3d_heads (count and scan)", 32 * f, lambda: ops.mesh3d_heads(corners))
        v = int(boff[-1])
        ukeys, _ = timed("mesh3d_vertices", 32 * f + 20 * v, lambda: ops.mesh3d_vertices(corners, boff, v, h, w))
        del corners
        timed("mesh3d_quads (4 F binary searches among V keys)", 24 * f + 8 * v, lambda: ops.mesh3d_quads(fkeys, ukeys, h, w))
        timed("mesh3d_starts, faces and vertices", 16 * (k + 1), lambda: (ops.mesh3d_starts(fkeys, k), ops.mesh3d_starts(ukeys, k)))
        timed("mesh3d_topology", 4 * n + 16 * k, lambda: ops.mesh3d_topology(vol_d, k))
        del masks, raw, fkeys, ukeys
    for name, (nbytes, t) in times.items():
        ms = med(t[1:])
        say(f"    stage {name:<52s} {ms * 1e3:11.1f} us (spread {spread(t[1:]) * 1e3:9.1f}); {nbytes / 1e6:8.1f} MB = {nbytes / 8e12 * 1e6:7.1f} us at 8 TB/s: "
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
    labelled = float((vol_d > 0).float().mean())
    say(f"label_stack {a.planes} x {a.size}^2, {a.cells} spheres of radius {a.rmin}..{a.rmax}, dz = {a.dz}, linked on the device: K = {k} objects, "
        f"{100 * labelled:.1f} % of the {vol_d.numel()} voxels labelled")
    sp, ss = min(a.host_sub[0], a.planes), min(a.host_sub[1], a.size)
    sub_d = vol_d[:sp, :ss, :ss].contiguous()
    sub = sub_d.cpu().numpy()
    present = torch.unique(vol_d[vol_d > 0])
    some = present[torch.linspace(0, len(present) - 1, min(16, len(present))).long()].cpu()
    ok = True
    calls = [("label_surfaces", lambda v, kw: M.label_surfaces(v, num=k, **kw)),
             (f"label_surfaces(only = {len(some)} ids)", lambda v, kw: M.label_surfaces(v, num=k, only=some, **kw)),
             ("object_topology", lambda v, kw: M.object_topology(v, num=k, **kw))]
    for name, fn in calls:
        fn(vol_d, {})                                    # warm-up: allocator, code objects
        fn(sub_d, {})
        th, ts, tg, host, dsub, dg = [], [], [], None, None, None
        for _ in range(a.reps):                          # the routes alternate within a round
            if not a.no_host:
                t, host = _timed(lambda: fn(sub, {"device": "cpu"}))
                th.append(t)
                t, dsub = _timed(lambda: fn(sub_d, {}))
                ts.append(t)
            dg = None
            t, dg = _timed(lambda: fn(vol_d, {}))
            tg.append(t)
        counts_text = f"; F = {len(dg.quads)} quads, V = {len(dg.vertices)} vertices" if hasattr(dg, "quads") else ""
        say(f"{name}")
        say(f"  (b) device     whole volume resident, synchronised: runs {fmt(tg)} s, median {med(tg):.6f} s, spread "
            f"{spread(tg):.6f} s ({vol_d.numel() / med(tg) / 1e9:.2f} G voxels / s){counts_text}")
        del dg
        if th:
            same = all(torch.equal(d.cpu(), h) for d, h in zip(dsub, host))
            ok = ok and same
            say(f"  (a) host form  numpy definition on the sub-volume {sp} x {ss} x {ss}: runs {fmt(th)} s, median {med(th):.6f} s, spread {spread(th):.6f} s")
            say(f"      device on the same sub-volume: runs {fmt(ts)} s, median {med(ts):.6f} s, spread {spread(ts):.6f} s; outputs "
                f"{'IDENTICAL' if same else 'DIFFERENT'}; {_claim(th, ts, '(a)', '(b)')}")
        else:
            say("  (a) host form  not measured")
    if a.stages:
        stages(vol_d, k, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    assert ok, "the routes disagree"
    return 0


if __name__ == "__main__":
    sys.exit(main())
