"""Time the distance transforms of utils.distance on a synthetic label frame, in one process, the routes alternating:

  (a) the host form: the numpy definition, labels in host memory;
  (b) the device route (csrc/distance.hip): labels resident on the GPU, torch.cuda.synchronize() before and after, after one warm-up call;
  (c) where scipy is installed: scipy.ndimage on the host -- one full-frame distance_transform_edt(return_indices=True) for the background and for
      expand_labels, one distance_transform_edt(labels == i) per instance for the inner map (what the reference's per-instance loop does).

The frame is utils.synthetic.label_frame (default 2048^2); --worst removes all but one instance, the worst case of the unbounded feature scan (every
pixel walks up to W columns).

    python tools/distance_bench.py [--size 2048] [--cells 400] [--reps 3] [--stages] [--worst] [--no-host] [--out profiles/r18_distance.txt]

scipy's per-instance route costs one full-frame transform per instance (minutes at 2048^2): it runs --scipy-inner-reps times (default 1; a single run
has no spread, so no "faster than" claim is made from it).  The host form of the unbounded background_feature walks the whole row in numpy (minutes on
the --worst frame) and is not measured there.

Prints every run, the medians and the spread (max - min), and whether the routes give identical outputs; --out also appends the lines to a file (the
main input and the --worst frame go into one file).
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
from ullsam_amd.utils import synthetic as S  # noqa: E402

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


def scipy_inner(ndi, lab):
    """One full-frame transform per instance, as the reference does."""
    out = np.zeros(lab.shape, np.int64)
    for i in np.unique(lab[lab > 0]):
        m = lab == i
        out[m] = np.rint(ndi.distance_transform_edt(m)[m] ** 2)
    return out


def scipy_expand(ndi, lab, distance):
    edt, idx = ndi.distance_transform_edt(lab == 0, return_indices=True)
    return np.where(edt <= distance, lab[idx[0], idx[1]], 0)


def scipy_feature(ndi, lab):
    return np.rint(ndi.distance_transform_edt(lab == 0) ** 2).astype(np.int64)


def stages(lab_d, reps, say):
    """The device route stage by stage through ops, each between two device events, beside the bytes each pass has to move at 8 TB/s."""
    from ullsam_amd import ops
    h, w = lab_d.shape
    px = h * w
    k = int(lab_d.max())
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
        g, _, _ = timed("columns, inner (labels read twice, g written, read, written)", 14 * px, lambda: ops.distance_columns(lab_d, False, False, num=k))
        timed("rows, inner -> D2", 10 * px, lambda: ops.distance_rows(lab_d, g, None, "inner"))
        timed("rows, shrink r2 = 16, LDS", 10 * px, lambda: ops.distance_rows(lab_d, g, None, "shrink", limit=16, route="lds"))
        timed("rows, shrink r2 = 16, global", 10 * px, lambda: ops.distance_rows(lab_d, g, None, "shrink", limit=16, route="global"))
        best, _ = timed("rows, depth (atomics)", 6 * px, lambda: ops.distance_rows(lab_d, g, None, "depth", num=k))
        timed("depth decode", 20 * k, lambda: ops.distance_depth_decode(best, w))
        gf, near, _ = timed("columns, feature (labels read twice, g + nearest written, read, written)", 26 * px, lambda: ops.distance_columns(lab_d, True))
        for r in (8, 64):
            for route in ("lds", "global"):
                timed(f"rows, expand r = {r}, {route}", 14 * px, lambda: ops.distance_rows(lab_d, gf, near, "expand", limit=r * r, route=route))
        timed("rows, feature unbounded", 18 * px, lambda: ops.distance_rows(lab_d, gf, near, "feature"))
    for (name, nbytes), t in times.items():
        ms = med(t[1:])
        say(f"    stage {name:<78s} {ms * 1e3:10.1f} us (spread {spread(t[1:]) * 1e3:8.1f}); {nbytes / 1e6:7.1f} MB = {nbytes / 8e12 * 1e6:6.1f} us at 8 TB/s: x{ms * 1e-3 / (nbytes / 8e12):.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--rmin", type=float, default=20.0)
    ap.add_argument("--rmax", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--worst", action="store_true", help="keep one instance only and time the unbounded background_feature there as well")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy host form and scipy (the device route alone)")
    ap.add_argument("--scipy-inner-reps", type=int, default=1, help="runs of scipy's one-transform-per-instance route")
    ap.add_argument("--stages", action="store_true", help="also time the device route stage by stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lab = S.label_frame(1, a.size, a.size, a.cells, (a.rmin, a.rmax))
    if a.worst:
        ids = np.unique(lab[lab > 0])
        lab = np.where(lab == ids[len(ids) // 2], lab, 0).astype(np.int32)
    say(f"label_frame {a.size}^2, {a.cells} cells of radius {a.rmin}..{a.rmax}{' (all but one instance removed)' if a.worst else ''}: "
        f"{len(np.unique(lab[lab > 0]))} instances, {100 * (lab > 0).mean():.1f} % of the pixels labelled")
    ndi = None if a.no_host else _scipy()
    say("scipy: " + ("not installed, its routes are not measured" if ndi is None and not a.no_host else "skipped" if a.no_host else "installed"))
    lab_d = torch.from_numpy(lab).cuda()
    calls = [("inner_distance", lambda x, kw: D.inner_distance(x, **kw), "inner"),
             ("expand_labels(distance=8)", lambda x, kw: D.expand_labels(x, distance=8, **kw), 8),
             ("expand_labels(distance=64)", lambda x, kw: D.expand_labels(x, distance=64, **kw), 64),
             ("shrink_labels(distance=4)", lambda x, kw: D.shrink_labels(x, distance=4, **kw), None),
             ("instance_depth", lambda x, kw: D.instance_depth(x, **kw), None)]
    if a.worst:
        calls.append(("background_feature(max_distance2=None)", lambda x, kw: D.background_feature(x, **kw), "feature"))
    ok = True
    for name, fn, sci in calls:
        dev = fn(lab_d, {})                               # warm-up: allocator, code objects
        torch.cuda.synchronize()
        ta, tb, tc, host, ref = [], [], [], None, None
        for rep in range(a.reps):
            if not a.no_host and sci != "feature":
                t0 = time.perf_counter()
                host = fn(lab, {"device": "cpu"})
                ta.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = fn(lab_d, {})
            torch.cuda.synchronize()
            tb.append(time.perf_counter() - t0)
            if ndi is not None and sci is not None and (sci != "inner" or rep < a.scipy_inner_reps):
                t0 = time.perf_counter()
                ref = scipy_inner(ndi, lab) if sci == "inner" else scipy_feature(ndi, lab) if sci == "feature" else scipy_expand(ndi, lab, sci)
                tc.append(time.perf_counter() - t0)
        say(f"{name}")
        say(f"  (b) device     labels resident, synchronised: runs {fmt(tb)} s, median {med(tb):.6f} s, spread {spread(tb):.6f} s")
        if ta:
            same = all(torch.equal(d.cpu(), h) for d, h in zip(_tensors(dev), _tensors(host)))
            ok = ok and same
            gap, worse = med(ta) - med(tb), max(spread(ta), spread(tb))
            say(f"  (a) host form  numpy definition:              runs {fmt(ta)} s, median {med(ta):.6f} s, spread {spread(ta):.6f} s")
            say(f"      outputs {'IDENTICAL' if same else 'DIFFERENT'}; (a) / (b) = {med(ta) / med(tb):.1f}x; (a) - (b) = {gap:.6f} s against 3 x the larger spread "
                f"{3 * worse:.6f} s -> {'(b) is faster' if gap > 3 * worse else '(a) is faster' if -gap > 3 * worse else 'no claim'}")
        else:
            say("  (a) host form  not measured")
        if tc:
            got = _tensors(dev)[0].cpu().numpy()
            agree = int((got == ref).sum())
            gap, worse = med(tc) - med(tb), max(spread(tc), spread(tb))
            say(f"  (c) scipy      {'one edt per instance' if sci == 'inner' else 'one full-frame edt' if sci == 'feature' else 'one full-frame edt with indices'}: runs {fmt(tc)} s, median {med(tc):.6f} s, "
                f"spread {spread(tc):.6f} s")
            say(f"      {agree} of {got.size} pixels equal to (b){' (the others are ties, where scipy returns some minimiser)' if agree != got.size and sci != 'inner' else ''}; "
                f"(c) / (b) = {med(tc) / med(tb):.1f}x; (c) - (b) = {gap:.6f} s against {3 * worse:.6f} s -> "
                f"{'no claim (one run)' if len(tc) < 2 else '(b) is faster' if gap > 3 * worse else '(c) is faster' if -gap > 3 * worse else 'no claim'}")
            if sci in ("inner", "feature"):
                ok = ok and agree == got.size
        else:
            say("  (c) scipy      not measured")
    if a.stages:
        stages(lab_d, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
