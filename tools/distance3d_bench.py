"""Time the distance transforms of utils.distance3d on a synthetic sphere stack linked on the device, in one process, the routes alternating:

  (a) the host form: the numpy definition, on a SUB-VOLUME (--host-sub planes side; the first planes, the top-left corner) small enough to finish,
      against the device route on the same sub-volume;
  (b) the device route (csrc/distance3d.hip) on the whole volume: resident on the GPU, torch.cuda.synchronize() before and after, after one
      warm-up call;
  (c) where scipy is installed: scipy.ndimage.distance_transform_edt(volume == 0, sampling=spacing, return_indices=True) on the host, one
      full-volume call for background_feature3d and one for expand_labels3d (single runs have no spread: no claim is made from them).

The volume is utils.synthetic.label_stack (default 32 x 2048^2, dz = 2.5) linked by utils.stack.link_label_stack(device="cuda"), spacing (5, 2, 2);
--worst removes all but one object, the worst case of the unbounded feature scans (every voxel walks up to H and W voxels).

    python tools/distance3d_bench.py [--planes 32] [--size 2048] [--cells 6000] [--reps 3] [--stages] [--worst] [--no-host] [--out profiles/r23_distance3d.txt]

Prints every run, the medians and the spread (max - min), and whether the routes give identical outputs; --out also appends the lines to a file.
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
from ullsam_amd.utils import distance3d as D  # noqa: E402
from ullsam_amd.utils import synthetic as S  # noqa: E402
from ullsam_amd.utils.stack import link_label_stack  # noqa: E402

med = statistics.median
spread = lambda t: max(t) - min(t)
fmt = lambda t: ", ".join(f"{x:.6f}" for x in t)


def _tensors(out):
    return list(out) if isinstance(out, tuple) else [out]


def _scipy():
    try:
        from scipy import ndimage
        return ndimage
    except ImportError:
        return None


def _claim(ta, tb, a, b):
    gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
    verdict = "no claim (one run)" if min(len(ta), len(tb)) < 2 else f"{b} is faster" if gap > 3 * worse else f"{a} is faster" if -gap > 3 * worse else "no claim"
    return f"{a} / {b} = {med(ta) / med(tb):.1f}x; {a} - {b} = {gap:.6f} s against 3 x the larger spread {3 * worse:.6f} s -> {verdict}"


def stages(vol_d, s, reps, say):
    """The device route pass by pass through ops, each between two device events, beside the bytes each pass has to move at 8 TB/s."""
    from ullsam_amd import ops
    z, h, w = vol_d.shape
    n = z * h * w
    k = int(vol_d.max())
    e = (False, False, False)
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
        g, _, _ = timed("z, inner (volume read twice, g written, read, written)", 14 * n, lambda: ops.distance3d_z(vol_d, False, False, num=k))
        hh, _ = timed("y, inner (volume, g read, h written)", 10 * n, lambda: ops.distance3d_y(vol_d, g, None, s, e))
        timed("x, inner -> D2 (volume, h read, D2 written)", 12 * n, lambda: ops.distance3d_x(vol_d, hh, None, "inner", s, e))
        hb, _ = timed("y, inner, r2 = 16", 10 * n, lambda: ops.distance3d_y(vol_d, g, None, s, e, limit=16))
        timed("x, shrink r2 = 16", 12 * n, lambda: ops.distance3d_x(vol_d, hb, None, "shrink", s, e, limit=16))
        best, _ = timed("x, depth (atomics)", 8 * n, lambda: ops.distance3d_x(vol_d, hh, None, "depth", s, e, num=k))
        timed("depth decode", 24 * k, lambda: ops.distance3d_depth_decode(best, h, w))
        del hh, hb
        gf, near, _ = timed("z, feature (volume read twice, g + nearest written, read, written)", 26 * n, lambda: ops.distance3d_z(vol_d, True))
        for r in (8, 64):
            hf, hl = timed(f"y, feature r = {r}", 14 * n, lambda: ops.distance3d_y(vol_d, gf, near, s, limit=r * r))
            timed(f"x, expand r = {r}", 16 * n, lambda: ops.distance3d_x(vol_d, hf, hl, "expand", s, limit=r * r))
        hf, hl = timed("y, feature unbounded", 14 * n, lambda: ops.distance3d_y(vol_d, gf, near, s))
        timed("x, feature unbounded", 20 * n, lambda: ops.distance3d_x(vol_d, hf, hl, "feature", s))
        del g, gf, near, hf, hl
    for (name, nbytes), t in times.items():
        ms = med(t[1:])
        say(f"    stage {name:<72s} {ms * 1e3:11.1f} us (spread {spread(t[1:]) * 1e3:9.1f}); {nbytes / 1e6:8.1f} MB = {nbytes / 8e12 * 1e6:7.1f} us at 8 TB/s: "
            f"x{ms * 1e-3 / max(nbytes / 8e12, 1e-12):.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=6000, help="spheres drawn in the stack's volume")
    ap.add_argument("--rmin", type=float, default=12.0)
    ap.add_argument("--rmax", type=float, default=40.0)
    ap.add_argument("--dz", type=float, default=2.5, help="plane spacing in pixels")
    ap.add_argument("--spacing", type=int, nargs=3, default=(5, 2, 2), help="(sz, sy, sx): integers in the ratio dz : 1 : 1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sub", type=int, nargs=2, default=(8, 384), help="planes and side of the sub-volume the numpy host form runs on")
    ap.add_argument("--worst", action="store_true", help="keep one object only and time the unbounded background_feature3d there")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form and scipy (the device route alone)")
    ap.add_argument("--stages", action="store_true", help="also time the device route pass by pass")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = tuple(a.spacing)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    planes, counts = S.label_stack(1, a.planes, a.size, a.size, a.cells, (a.rmin, a.rmax), a.dz)
    vol_d = link_label_stack(torch.from_numpy(planes).cuda(), counts, device="cuda")[0]
    del planes
    if a.worst:
        ids = torch.unique(vol_d[vol_d > 0])
        vol_d = torch.where(vol_d == ids[len(ids) // 2], vol_d, 0).to(torch.int32).contiguous()
    vol = vol_d.cpu().numpy()
    say(f"label_stack {a.planes} x {a.size}^2, {a.cells} spheres of radius {a.rmin}..{a.rmax}, dz = {a.dz}, linked on the device"
        f"{' (all but one object removed)' if a.worst else ''}: {int((np.bincount(vol.reshape(-1))[1:] > 0).sum())} objects, "
        f"{100 * (vol > 0).mean():.1f} % of the {vol.size} voxels labelled; spacing {s}")
    ndi = None if a.no_host else _scipy()
    say("scipy: " + ("skipped" if a.no_host else "not installed, its route is not measured" if ndi is None else
                     f"installed; {len(os.sched_getaffinity(0))} host cores available to the process"))
    sp, ss = min(a.host_sub[0], a.planes), min(a.host_sub[1], a.size)
    sub = np.ascontiguousarray(vol[:sp, :ss, :ss])
    sub_d = torch.from_numpy(sub).cuda()
    kw = {"spacing": s}
    calls = [("inner_distance3d", lambda x, k: D.inner_distance3d(x, **k), None),
             ("background_feature3d(max_distance2=None)", lambda x, k: D.background_feature3d(x, **k), "feature"),
             ("expand_labels3d(distance=8)", lambda x, k: D.expand_labels3d(x, distance=8, **k), 8),
             ("shrink_labels3d(distance=4)", lambda x, k: D.shrink_labels3d(x, distance=4, **k), None),
             ("object_depth", lambda x, k: D.object_depth(x, **k), None)]
    if a.worst:
        calls = calls[1:2]
    ok = True
    for name, fn, sci in calls:
        dev = fn(vol_d, kw)                               # warm-up: allocator, code objects
        fn(sub_d, kw)
        torch.cuda.synchronize()
        ta, tb, ts, tc, host, dsub, ref = [], [], [], [], None, None, None
        for rep in range(a.reps):
            if not a.no_host and not a.worst:
                t0 = time.perf_counter()
                host = fn(sub, dict(kw, device="cpu"))
                ta.append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dsub = fn(sub_d, kw)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = fn(vol_d, kw)
            torch.cuda.synchronize()
            tb.append(time.perf_counter() - t0)
            if ndi is not None and sci is not None and rep == 0:
                t0 = time.perf_counter()
                edt, idx = ndi.distance_transform_edt(vol == 0, sampling=s, return_indices=True)
                ref = np.rint(edt ** 2).astype(np.int64) if sci == "feature" else np.where(edt <= sci, vol[idx[0], idx[1], idx[2]], 0)
                tc.append(time.perf_counter() - t0)
                del edt, idx
        say(f"{name}")
        say(f"  (b) device     whole volume resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s "
            f"({vol.size / med(tb) / 1e9:.2f} G voxels / s)")
        if ta:
            same = all(torch.equal(d.cpu(), h) for d, h in zip(_tensors(dsub), _tensors(host)))
            ok = ok and same
            say(f"  (a) host form  numpy definition on the sub-volume {sp} x {ss} x {ss}: runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
            say(f"      device on the same sub-volume: runs {fmt(ts)} s, median {med(ts):.6f} s, spread {spread(ts):.6f} s; outputs "
                f"{'IDENTICAL' if same else 'DIFFERENT'}; {_claim(ta, ts, '(a)', '(b)')}")
        else:
            say("  (a) host form  not measured")
        if tc:
            got = _tensors(dev)[0].cpu().numpy()
            agree = int((got == ref).sum())
            say(f"  (c) scipy      one full-volume edt with indices: runs {fmt(tc)} s")
            say(f"      {agree} of {got.size} voxels equal to (b){' (the others are ties, where scipy returns some minimiser)' if agree != got.size and sci != 'feature' else ''}; "
                f"{_claim(tc, tb, '(c)', '(b)')}")
            if sci == "feature":
                ok = ok and agree == got.size
            del got, ref
        else:
            say("  (c) scipy      not measured")
        del dev
    if a.stages:
        stages(vol_d, s, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
