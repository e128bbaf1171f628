"""Brute-force definitions of the prompts derived from an instance label image (ullsam_amd/utils/prompts.py, csrc/prompts.hip): d1, D2_i, the
two candidate sets, the draw rule and the whole PromptSet, as direct minima over pixel pairs in numpy and Python integers.  Only usable at small
sizes.  Nothing here shares code with the package (its own Philox included).

`restrict=True` takes the minima over the only pixels that can attain them -- for d1 the different-label pixels that touch the pixel's label, for D2_i
the instance pixels with a 4-neighbour outside the instance (on a shortest path from p to its nearest such pixel q, the pixel before q is nearer to p,
so it has p's label / lies outside M_i) -- which makes a 300 x 300 frame affordable; tests/test_prompts_cpu.py checks it equals restrict=False."""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox_word0(seed, counter):
    """word 0 of Philox4x32-10, key (seed & 0xffffffff, seed >> 32), in Python integers"""
    seed %= 1 << 64
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c0, c1, c2, c3 = (int(c) & 0xFFFFFFFF for c in counter)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0


def draw(seed, k, m, counter):
    """k distinct ranks out of m, in pick order: r = (w (m - t)) >> 32 is the rank among the candidates not yet picked"""
    picks = []
    for t in range(k):
        r = (philox_word0(seed, counter(t)) * (m - t)) >> 32
        for q in sorted(picks):
            if q <= r:
                r += 1
        picks.append(r)
    return picks


def draw_points(seed, inst, kind, k, m):
    return draw(seed, k, m, lambda t: (inst, t + 16 * kind, 0, 0))


def _touch(mask):
    """pixels with a 4-neighbour (inside the array) in `mask`"""
    t = np.zeros_like(mask)
    t[1:] |= mask[:-1]
    t[:-1] |= mask[1:]
    t[:, 1:] |= mask[:, :-1]
    t[:, :-1] |= mask[:, 1:]
    return t


def _min_over_pairs(py, px, qy, qx, metric, chunk=2048):
    out = np.empty(len(py), np.int64)
    for a in range(0, len(py), chunk):
        dy = py[a:a + chunk, None].astype(np.int32) - qy[None].astype(np.int32)
        dx = px[a:a + chunk, None].astype(np.int32) - qx[None].astype(np.int32)
        out[a:a + chunk] = (np.abs(dy) + np.abs(dx) if metric == "l1" else dy * dy + dx * dx).min(1)
    return out


def d1(labels, restrict=True):
    """int64 [H, W]: city-block distance to the nearest pixel with another label; the outside of the frame (a border of one pixel) differs"""
    H, W = labels.shape
    pad = np.full((H + 2, W + 2), -1, np.int64)
    pad[1:-1, 1:-1] = labels
    out = np.zeros((H, W), np.int64)
    for L in np.unique(labels):
        same = pad == L
        q = ~same & _touch(same) if restrict else ~same
        py, px = np.where(same)
        qy, qx = np.where(q)
        out[py - 1, px - 1] = _min_over_pairs(py, px, qy, qx, "l1")
    return out


def d2(labels, inst, restrict=True):
    """int64 [H, W]: squared Euclidean distance to the nearest pixel of the instance (0 inside it)"""
    m = labels == inst
    q = m & _touch(~m) if restrict else m
    py, px = np.where(~m)
    qy, qx = np.where(q)
    out = np.zeros(labels.shape, np.int64)
    out[py, px] = _min_over_pairs(py, px, qy, qx, "l2")
    return out


def inner_set(labels, inst, inner_radius, d1_map=None):
    d = d1(labels) if d1_map is None else d1_map
    return (labels == inst) & (d > inner_radius)


def ring_set(labels, inst, ring):
    lo, hi = ring
    d = d2(labels, inst)
    return (labels != inst) & (d >= lo * lo) & (d <= hi * hi)


def l1_to_instance(labels, inst):
    m = labels == inst
    py, px = np.where(~m)
    qy, qx = np.where(m & _touch(~m))
    out = np.zeros(labels.shape, np.int64)
    out[py, px] = _min_over_pairs(py, px, qy, qx, "l1")
    return out


def choose(labels, max_instances, seed):
    present = [int(v) for v in np.unique(labels) if v > 0]
    if len(present) <= max_instances:
        return present
    return [present[r] for r in draw(seed, max_instances, len(present), lambda t: (0, t, 1, 0))]


def default_instance(H, W, num_pos, num_neg):
    cl = lambda v, n: min(max(v, 0), n - 1)
    corners = [(cl(10, W), cl(10, H)), (cl(W - 10, W), cl(10, H)), (cl(10, W), cl(H - 10, H)), (cl(W - 10, W), cl(H - 10, H))]
    return [(W // 2, H // 2)] * num_pos + [corners[i % 4] for i in range(num_neg)]


def prompts(labels, num_pos=1, num_neg=3, max_instances=4, ids=None, seed=0, inner_radius=10, ring=(9, 11)):
    """dict(ids, coords, point_labels, boxes, masks, counts, inner, ring) with the dtypes and shapes of utils.prompts.PromptSet; inner / ring are the
    candidate sets as boolean images [N, H, W]"""
    labels = np.asarray(labels)
    H, W = labels.shape
    P = num_pos + num_neg
    point_labels = lambda n: np.tile(np.array([1] * num_pos + [0] * num_neg, np.int32), (n, 1)).reshape(n, P)
    chosen = choose(labels, max_instances, seed) if ids is None else [int(v) for v in ids]
    if ids is None and not chosen:
        return dict(ids=np.zeros(1, np.int32), coords=np.array(default_instance(H, W, num_pos, num_neg), np.float32).reshape(1, P, 2),
                    point_labels=point_labels(1), boxes=np.zeros((1, 4), np.float32), masks=np.zeros((1, H, W), np.float32),
                    counts=np.zeros((1, 2), np.int32), inner=np.zeros((1, H, W), bool), ring=np.zeros((1, H, W), bool))
    d1_map = d1(labels)
    N = len(chosen)
    out = dict(ids=np.array(chosen, np.int32), coords=np.zeros((N, P, 2), np.float32), point_labels=point_labels(N), boxes=np.zeros((N, 4), np.float32),
               masks=np.zeros((N, H, W), np.float32), counts=np.zeros((N, 2), np.int32), inner=np.zeros((N, H, W), bool), ring=np.zeros((N, H, W), bool))
    for n, i in enumerate(chosen):
        m = labels == i
        if not m.any():
            raise ValueError(f"id {i} has no pixels")
        ys, xs = np.where(m)
        inner = inner_set(labels, i, inner_radius, d1_map)
        rng = ring_set(labels, i, ring)
        iy, ix = np.where(inner)
        ry, rx = np.where(rng)
        if len(iy) >= num_pos:
            pos = [(ix[r], iy[r]) for r in draw_points(seed, i, 0, num_pos, len(iy))]
        elif len(iy) > 0:
            pos = [(ix[j % len(iy)], iy[j % len(iy)]) for j in range(num_pos)]
        else:
            pos = [(int(xs.sum()) // len(xs), int(ys.sum()) // len(ys))] * num_pos
        if len(ry) >= num_neg:
            neg = [(rx[r], ry[r]) for r in draw_points(seed, i, 1, num_neg, len(ry))]
        else:
            fy, fx = np.where(l1_to_instance(labels, i) > inner_radius)
            kind = 2
            if len(fy) < num_neg:
                fy, fx = np.where(~m)
                kind = 3
            if len(fy) == 0:
                raise ValueError(f"instance {i} fills the frame")
            ranks = draw_points(seed, i, kind, num_neg, len(fy)) if len(fy) >= num_neg else [j % len(fy) for j in range(num_neg)]
            neg = [(fx[r], fy[r]) for r in ranks]
        out["coords"][n] = np.array(pos + neg, np.float32).reshape(P, 2)
        out["boxes"][n] = (xs.min(), ys.min(), xs.max(), ys.max())
        out["masks"][n] = m
        out["counts"][n] = (len(iy), len(ry))
        out["inner"][n] = inner
        out["ring"][n] = rng
    return out


# ---- the scenes the CPU and GPU tests share ----------------------------------------------------------------------------------------
def _disc(lab, cy, cx, r, v):
    yy, xx = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
    lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v


def scene_a():
    """67 x 131: a disc (1), a one-pixel instance (2), a bar thinner than 21 (3: no interior at radius 10), a corner instance whose ring is clipped on
    two sides (5), two rectangles sharing a border (7, 8: each one's ring lies over the other); ids 4 and 6 are absent"""
    lab = np.zeros((67, 131), np.int32)
    _disc(lab, 33, 30, 16, 1)
    lab[5, 60] = 2
    lab[50:59, 50:101] = 3
    lab[60:67, 122:131] = 5
    lab[10:41, 70:96] = 7
    lab[10:41, 96:126] = 8
    return lab


def scene_b():
    """160 x 96: a 21 x 23 rectangle (2: three interior pixels at radius 10, fewer than num_pos = 4), a disc (4), a disc cut by the frame (11), the
    largest id (65535)"""
    lab = np.zeros((160, 96), np.int32)
    lab[5:26, 5:28] = 2
    _disc(lab, 80, 50, 20, 4)
    _disc(lab, 150, 90, 15, 11)
    lab[100:105, 2:9] = 65535
    return lab


def scene_c():
    """67 x 131: one instance everywhere but two pixels -- no ring, nothing far away, fewer than num_neg pixels outside it"""
    lab = np.ones((67, 131), np.int32)
    lab[0, 0] = 0
    lab[66, 130] = 0
    return lab


def scene_d():
    """160 x 96: one instance everywhere but a 9 x 9 corner of background"""
    lab = np.full((160, 96), 3, np.int32)
    lab[:9, :9] = 0
    return lab


def scene_e():
    """300 x 300: a disc of radius 100, whose window spans several workgroups"""
    lab = np.zeros((300, 300), np.int32)
    _disc(lab, 150, 140, 100, 1)
    return lab
