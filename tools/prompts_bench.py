"""Time the prompts-from-labels step on a seeded synthetic label image (utils.synthetic.label_tile: the discs of the microscopy tile), in one process,
the measurements alternating:

  (a) the host loop a user of the reference has: per chosen instance the scipy calls its dataset makes (train_joint_v2.py:342-343, 423-435) on
      the instance's float mask -- a 10-iteration binary_erosion, a 10-iteration binary_dilation, a one-step erosion and a full-frame
      distance_transform_edt -- then np.where on the two candidate sets.  The union of the other instances that the reference also builds per
      instance (and never reads) is left out, and the output says so.  Without scipy on the machine: the numpy host route of utils.prompts,
      and the output says so;
  (b) utils.prompts.prompts_from_labels on the device from a label image that is already there (masks included), torch.cuda.synchronize() around it.

    python tools/prompts_bench.py [--size 1024] [--reps 3] [--out profiles/r12_prompts.txt]

For max_instances 4 and 64: every run, the medians and the spread (max - min), and whether the device's two candidate sets (the op's debug images)
equal (a)'s for every chosen instance.
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
from ullsam_amd.utils import prompts as P  # noqa: E402
from ullsam_amd.utils.synthetic import label_tile  # noqa: E402

try:
    from scipy import ndimage
except ImportError:                                      # the comparison then runs against the numpy host route
    ndimage = None


def scipy_route(labels, chosen, inner_radius=10, ring=(9, 11)):
    """Per chosen id, scipy's four calls on the instance's float mask and np.where on both sets -> [(interior bool, ring bool)].  The union of
    the other instances, which the reference also builds per instance and never reads, is NOT part of this figure."""
    lo, hi = ring
    sets = []
    for i in chosen:
        m = (labels == i).astype(np.float32)
        interior = ndimage.binary_erosion(m, iterations=inner_radius)
        ndimage.binary_dilation(m, iterations=inner_radius)            # computed per instance there as well; only the fallbacks read it
        edge = np.logical_xor(m, ndimage.binary_erosion(m))
        dist = ndimage.distance_transform_edt(~edge)
        around = (dist >= lo) & (dist <= hi) & (m == 0)
        np.where(interior)
        np.where(around)
        sets.append((interior, around))
    return sets


def numpy_route(mask_np, chosen):
    inner, ring = P.candidate_sets(mask_np, chosen)
    P.prompts_from_labels(mask_np, ids=chosen)
    return list(zip(inner, ring))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = scipy_route if ndimage is not None else numpy_route
    what = ("scipy's binary_erosion(iterations=10), binary_dilation(iterations=10), one-step binary_erosion and full-frame distance_transform_edt per "
            "chosen instance, then np.where on both sets; the union of the other instances that the reference also builds per instance, and never "
            "reads, is NOT included" if ndimage is not None else "scipy is ABSENT here: the numpy host route of utils.prompts")
    lines = [f"tools/prompts_bench.py --size {a.size} --reps {a.reps} on {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} host cores available",
             f"how: one process; after one warm-up call per case, {a.reps} runs of (a) and (b) in turn, time.perf_counter() around each, medians and "
             "spread = max - min",
             f"(a) host: {what}",
             "(b) device: utils.prompts.prompts_from_labels(labels on the device, max_instances=..), masks returned, torch.cuda.synchronize() before "
             "and after; the upload of the label image is not timed"]
    med = lambda t: statistics.median(t)
    spread = lambda t: max(t) - min(t)
    fmt = lambda t: ", ".join(f"{x:.4f}" for x in t)
    for max_instances, n_cells, r_range in ((4, 14, (70.0, 150.0)), (64, 96, (20.0, 60.0))):
        lab = label_tile(7, a.size, n_cells, r_range)
        dev = torch.from_numpy(lab).cuda()
        ps = P.prompts_from_labels(dev, max_instances=max_instances)              # warm-up: allocator, code objects
        chosen = ps.ids.tolist()
        torch.cuda.synchronize()
        ta, tb = [], []
        sets = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            sets = host(lab, chosen)
            ta.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ps = P.prompts_from_labels(dev, max_instances=max_instances)
            torch.cuda.synchronize()
            tb.append(time.perf_counter() - t0)
        inner, ring = P.candidate_sets(dev, chosen)
        inner, ring = inner.cpu().numpy(), ring.cpu().numpy()
        same = all(np.array_equal(inner[k], sets[k][0]) and np.array_equal(ring[k], sets[k][1]) for k in range(len(chosen)))
        counts_ok = ps.counts.cpu().numpy().tolist() == [[int(s[0].sum()), int(s[1].sum())] for s in sets]
        lines += [f"{a.size}^2 label image, {len(np.unique(lab)) - 1} instances present, max_instances {max_instances}: {len(chosen)} chosen",
                  f"  (a) host   per-instance loop:                        runs {fmt(ta)} s, median {med(ta):.4f} s, spread {spread(ta):.4f} s",
                  f"  (b) device prompts_from_labels (masks), synchronised: runs {fmt([1e3 * x for x in tb])} ms, median {1e3 * med(tb):.4f} ms, spread {1e3 * spread(tb):.4f} ms",
                  f"  the device's candidate sets equal (a)'s for every chosen instance: {same}; counts equal: {counts_ok}; (a) / (b) = {med(ta) / med(tb):.1f}x"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
