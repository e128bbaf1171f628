// Tiled segment-everything: the instance label maps of overlapping tiles stitched into one label image (host form and definition:
// utils/mosaic.py; DESIGN.md "7b, continued").  Integer work only -- integer atomics, no float anywhere -- so every output is a function of
// the tiles alone: bit-exact with the numpy definition and identical from run to run.
//
// Ids.  Tile t holds local ids 0..K_t (0 = background); its global ids are base[t] + l for l > 0, base = the exclusive sum of the K_t,
// G = base[T] <= 2^31 - 2.  Every table here is indexed by global id, entry 0 unused.
// Seams.  A seam is the intersection R of the boxes of two 4-neighbour tiles (s, t), t the right (dir 0) or the lower (dir 1) neighbour.  One
// wave walks one row of one seam region, 64 pixels at a time, both tiles in memory order, and sends ONE atomic per run of equal keys along
// the row (a run of whole 64-pixel segments is carried in registers, as label_overlap_kernel in labels.hip does):
//   - the in-seam areas A_s(a), A_t(b) as atomicAdds into areas[g, c], c = the side of the tile the seam lies on (0 left, 1 right, 2 up,
//     3 down): a label has one area per seam it takes part in;
//   - the pair counts n(a, b), a, b > 0, into an open-addressing table in global memory: key = dir << 63 | g_a << 32 | g_b (never 0), a slot
//     is claimed by a 64-bit atomicCAS against 0 and counted with an integer atomicAdd; linear probing, capacity a power of two
//     >= 2 * max_pairs.  The number of claimed slots is counted; once it exceeds max_pairs further NEW keys are refused and flags[1] is set,
//     so the table never fills and a probe sequence always ends.
// Merge.  One thread per slot: n * den >= num * (A_s + A_t - n) in 64-bit (all three are at most |R| < 2^31, num <= den < 2^31), then the
// union of the two ids in parent[G + 1] by linking the LARGER root under the smaller one with an atomicMin (mz_union, label_common.h),
// so a component's root is its smallest id whatever the order.  A flatten pass leaves parent[g] = that root.
// Stats.  One wave per row of a tile's core: visible area and inclusive XYXY box per representative, one atomicAdd per run, box bounds sent
// only when a relaxed load says they would improve (bounds move one way: a stale load costs an atomic, never a result).
// Compaction.  One workgroup (the scan of label_compact_kernel over G + 1 entries): keep = area != 0 and >= min_visible_area, renumbered
// 1..K by ascending representative; label_of_global[g] = final label of parent[g].
// Paste.  mosaic[p] = label_of_global[g(t, tile_t[p - origin_t])] for p in the core of t: the cores partition the frame, so every pixel is
// written exactly once, by an ordinary store (16 bytes per lane where the row's two addresses are 16-byte aligned).  The mosaic is indexed
// in 64 bits.
// Every descriptor (seam regions, cores) is clipped against the tiles and the frame in the kernels, and an id outside 0..K_t reads as
// background and sets flags[0]: malformed input cannot read or write outside the buffers.
#include "pair_table.h"   // the runs of equal keys along a row and the pair table; through it label_common.h: the relaxed atomics, the union-find
#include <limits.h>

// ---- seam counting --------------------------------------------------------------------------------------------------------------------
#define MZ_SEAM_LD 9   // s, t, sy, sx, ty, tx, h, w, dir: the region's origin in the two tiles' own coordinates, its size, 0 = right / 1 = down

// grid (ceil(max seam rows / 4), S), block 256: one wave per row of a seam region
__global__ __launch_bounds__(256) void mosaic_seams_kernel(const int* __restrict__ tiles, int T, int th, int tw, const int* __restrict__ base, long G,
                                                           const int* __restrict__ seams, mz_u64* __restrict__ keys, int* __restrict__ counts,
                                                           mz_u64 mask, int max_pairs, int* __restrict__ areas, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int* d = seams + (long)blockIdx.y * MZ_SEAM_LD;
    const int s = d[0], t = d[1], sy = d[2], sx = d[3], ty = d[4], tx = d[5], h = d[6], w = d[7], dir = d[8];
    if (r >= h) return;                                  // wave-uniform
    if (s < 0 || s >= T || t < 0 || t >= T || sy < 0 || sx < 0 || ty < 0 || tx < 0 || w < 0 || (long)sy + h > th || (long)ty + h > th ||
        (long)sx + w > tw || (long)tx + w > tw || (dir != 0 && dir != 1)) {
        if (lane == 0) mz_store(flags + 0, 1);           // a region outside its tiles is not walked
        return;
    }
    const int bs = base[s], ks = base[s + 1] - bs, bt = base[t], kt = base[t + 1] - bt;
    if (bs < 0 || ks < 0 || bt < 0 || kt < 0 || (long)bs + ks > G || (long)bt + kt > G) {   // base is not the exclusive sum it has to be: no table is indexed with it
        if (lane == 0) mz_store(flags + 0, 1);
        return;
    }
    const int* ps = tiles + ((long)s * th + sy + r) * tw + sx;
    const int* pt = tiles + ((long)t * th + ty + r) * tw + tx;
    const int cs = dir ? 3 : 1, ct = dir ? 2 : 0;        // the seam lies on s's right / lower side and on t's left / upper side
    const mz_u64 top = (mz_u64)dir << 63;
    auto add_s = [&](mz_u64 g, int, int n) { mz_add(areas + 4 * (long)g + cs, n); };
    auto add_t = [&](mz_u64 g, int, int n) { mz_add(areas + 4 * (long)g + ct, n); };
    auto add_p = [&](mz_u64 k, int, int n) { mz_pair_add(k, n, keys, counts, mask, max_pairs, flags); };
    MzRun ra = {0, 0, 0}, rb = {0, 0, 0}, rp = {0, 0, 0};
    bool bad = false;
    for (int xs = 0; xs < w; xs += 64) {
        const int x = xs + lane;
        int a = 0, b = 0;
        if (x < w) {
            a = ps[x];
            b = pt[x];
            if (a < 0 || a > ks) { bad = true; a = 0; }
            if (b < 0 || b > kt) { bad = true; b = 0; }
        }
        const mz_u64 ga = a > 0 ? (mz_u64)(bs + a) : 0, gb = b > 0 ? (mz_u64)(bt + b) : 0;
        mz_segment(ra, ga, xs, lane, add_s);
        mz_segment(rb, gb, xs, lane, add_t);
        mz_segment(rp, (ga && gb) ? (top | (ga << 32) | gb) : 0, xs, lane, add_p);
    }
    mz_flush(ra, lane, add_s);
    mz_flush(rb, lane, add_t);
    mz_flush(rp, lane, add_p);
    if (bad) mz_store(flags + 0, 1);
}

// ---- merge + union-find -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mosaic_iota_kernel(long n, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}
// one thread per slot; areas == nullptr: every pair of the table is merged
__global__ __launch_bounds__(256) void mosaic_merge_kernel(const mz_u64* __restrict__ keys, const int* __restrict__ counts, long cap,
                                                           const int* __restrict__ areas, long G, long num, long den, int* __restrict__ parent,
                                                           int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const mz_u64 k = keys[i];
    if (k == 0) return;
    const int dir = (int)(k >> 63);
    const long ga = (long)((k >> 32) & 0x7fffffffull), gb = (long)(k & 0xffffffffull);
    if (ga < 1 || ga > G || gb < 1 || gb > G) {          // (a hand-made table: the seam kernel writes no such key)
        mz_store(flags + 0, 1);
        return;
    }
    if (areas) {
        const long n = counts[i];
        const long uni = (long)areas[4 * ga + (dir ? 3 : 1)] + (long)areas[4 * gb + (dir ? 2 : 0)] - n;
        if (n <= 0 || n * den < num * uni) return;
    }
    mz_union(parent, (int)ga, (int)gb);
}
__global__ __launch_bounds__(256) void mosaic_flatten_kernel(long n, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mz_store(parent + i, mz_find(parent, (int)i));   // (whatever a concurrent reader finds at i is an ancestor of i)
}

// ---- the cores: stats and paste -------------------------------------------------------------------------------------------------------------
#define MZ_CORE_LD 6   // top, left, h, w of the core in the frame, then the tile's origin (oy, ox) in the frame
struct MzCore {
    int top, left, h, w, oy, ox;
    bool ok;
};
__device__ __forceinline__ MzCore mz_core(const int* __restrict__ cores, int t, int th, int tw, int H, int W) {
    const int* d = cores + (long)t * MZ_CORE_LD;
    MzCore c = {d[0], d[1], d[2], d[3], d[4], d[5], false};
    c.ok = c.top >= 0 && c.left >= 0 && c.h >= 0 && c.w >= 0 && (long)c.top + c.h <= H && (long)c.left + c.w <= W && c.top >= c.oy && c.left >= c.ox &&
           (long)c.top - c.oy + c.h <= th && (long)c.left - c.ox + c.w <= tw;
    return c;
}

// grid (ceil(max core rows / 4), T), block 256: one wave per row of a core
__global__ __launch_bounds__(256) void mosaic_stats_kernel(const int* __restrict__ tiles, int th, int tw, const int* __restrict__ base, long G,
                                                           const int* __restrict__ cores, const int* __restrict__ parent, int H, int W,
                                                           int* __restrict__ areas, int* __restrict__ boxes, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = blockIdx.y;
    const MzCore c = mz_core(cores, t, th, tw, H, W);
    if (!c.ok) {
        if (r == 0 && lane == 0) mz_store(flags + 0, 1);
        return;
    }
    if (r >= c.h) return;                                // wave-uniform
    const int b0 = base[t], kt = base[t + 1] - b0;
    if (b0 < 0 || kt < 0 || (long)b0 + kt > G) {         // base is not the exclusive sum it has to be
        if (lane == 0) mz_store(flags + 0, 1);
        return;
    }
    const int y = c.top + r;
    const int* src = tiles + ((long)t * th + (y - c.oy)) * tw + (c.left - c.ox);
    auto emit = [&](mz_u64 key, int x0, int n) {
        const long v = (long)key;
        mz_add(areas + v, n);
        const int xa = c.left + x0, xb = xa + n - 1;
        int* bx = boxes + 4 * v;
        mz_send_min(bx + 0, xa);
        mz_send_min(bx + 1, y);
        mz_send_max(bx + 2, xb);
        mz_send_max(bx + 3, y);
    };
    MzRun run = {0, 0, 0};
    bool bad = false;
    for (int xs = 0; xs < c.w; xs += 64) {
        const int x = xs + lane;
        int l = x < c.w ? src[x] : 0;
        if (l < 0 || l > kt) { bad = true; l = 0; }
        int p = l > 0 ? parent[b0 + l] : 0;
        if (p < 0 || p > G) { bad = true; p = 0; }       // (a representative is an id)
        mz_segment(run, (mz_u64)p, xs, lane, emit);
    }
    mz_flush(run, lane, emit);
    if (bad) mz_store(flags + 0, 1);
}

__global__ __launch_bounds__(256) void mosaic_stats_init_kernel(long n, int* __restrict__ areas, int* __restrict__ boxes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    areas[i] = 0;
    boxes[4 * i + 0] = INT_MAX;
    boxes[4 * i + 1] = INT_MAX;
    boxes[4 * i + 2] = -1;
    boxes[4 * i + 3] = -1;
}

// grid 1, block 256: thread t owns the ids [1 + t * ceil(G / 256), ...) -- a contiguous share, so the final labels ascend with the representative.
__global__ __launch_bounds__(256) void mosaic_compact_kernel(const int* __restrict__ areas_raw, const int* __restrict__ boxes_raw,
                                                             const int* __restrict__ parent, long G, int min_visible_area,
                                                             int* __restrict__ label_of_global, int* __restrict__ areas, int* __restrict__ boxes,
                                                             int* __restrict__ K) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    const long share = (G + 255) / 256;
    const long g0 = min(1 + t * share, G + 1), g1 = min(g0 + share, G + 1);
    int c = 0;
    for (long g = g0; g < g1; ++g) {
        const int a = areas_raw[g];
        c += (a != 0 && a >= min_visible_area) ? 1 : 0;
    }
    part[t] = c;
    __syncthreads();
    if (t == 0) {                                        // exclusive scan of 256 partial counts
        int s = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = s;
            s += v;
        }
        K[0] = s;
        mz_store(label_of_global, 0);
    }
    __syncthreads();
    int k = part[t];
    for (long g = g0; g < g1; ++g) {                     // first the representatives (only they have an area) ...
        if (parent[g] != g) continue;
        const int a = areas_raw[g];
        const bool keep = a != 0 && a >= min_visible_area;
        mz_store(label_of_global + g, keep ? k + 1 : 0);
        if (keep) {
            areas[k] = a;
#pragma unroll
            for (int j = 0; j < 4; ++j) boxes[4 * (long)k + j] = boxes_raw[4 * g + j];
            ++k;
        }
    }
    __syncthreads();                                     // ... then the other members read their representative's entry
    for (long g = 1 + t; g <= G; g += 256) {
        const int p = parent[g];
        if (p != g) mz_store(label_of_global + g, (p >= 1 && p <= G) ? mz_load(label_of_global + p) : 0);
    }
}

// grid (ceil(max core rows / 4), T), block 256: one wave per row of a core.  vec: both buffers start on a 16-byte boundary.
__global__ __launch_bounds__(256) void mosaic_paste_kernel(const int* __restrict__ tiles, int th, int tw, const int* __restrict__ base, long G,
                                                           const int* __restrict__ cores, const int* __restrict__ log, int H, int W, int vec,
                                                           int* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = blockIdx.y;
    const MzCore c = mz_core(cores, t, th, tw, H, W);
    if (!c.ok || r >= c.h) return;                       // wave-uniform
    const int b0 = base[t];
    const int kt = (b0 >= 0 && base[t + 1] >= b0 && base[t + 1] <= G) ? base[t + 1] - b0 : 0;   // (a base that is no exclusive sum: every id reads as background)
    const int y = c.top + r;
    const long so = ((long)t * th + (y - c.oy)) * tw + (c.left - c.ox);
    const long dof = (long)y * W + c.left;
    const int* src = tiles + so;
    int* dst = labels + dof;
    int done = 0;
    if (vec && ((so | dof) & 3) == 0) {                  // wave-uniform: 16 bytes per lane
        const int w4 = c.w >> 2;
        for (int q = lane; q < w4; q += 64) {
            const int4 v = *reinterpret_cast<const int4*>(src + 4 * q);
            int4 o;
            o.x = mz_look(v.x, b0, kt, log);
            o.y = mz_look(v.y, b0, kt, log);
            o.z = mz_look(v.z, b0, kt, log);
            o.w = mz_look(v.w, b0, kt, log);
            *reinterpret_cast<int4*>(dst + 4 * q) = o;
        }
        done = w4 << 2;
    }
    for (int x = done + lane; x < c.w; x += 64) dst[x] = mz_look(src[x], b0, kt, log);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
#define MZ_TILES_CHECK(what)                                                                                                     \
    ULLSAM_CHECK(T >= 1 && T <= 65535 && th > 0 && tw > 0 && G >= 0 && G <= 2147483646L, what ": need 1 <= T <= 65535, th, tw > 0, 0 <= G <= 2^31 - 2")

extern "C" int ullsam_mosaic_seams(const int* tiles, int T, int th, int tw, const int* base, long G, const int* seams, int S, int max_rows,
                                   unsigned long long* keys, int* counts, long cap, int max_pairs, int* areas, int* flags, void* stream) {
    MZ_TILES_CHECK("mosaic_seams");
    ULLSAM_CHECK(S >= 0 && S <= 65535 && max_rows >= 0 && max_rows <= th, "mosaic_seams: need 0 <= S <= 65535 and 0 <= max_rows <= th");
    ULLSAM_CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && max_pairs >= 1 && 2L * max_pairs <= cap && cap <= (1L << 31),
                 "mosaic_seams: the capacity must be a power of two with 2 * max_pairs <= capacity <= 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!mz_zero(keys, (size_t)cap * 8, s) || !mz_zero(counts, (size_t)cap * 4, s) || !mz_zero(areas, (size_t)(G + 1) * 16, s) || !mz_zero(flags, 16, s)) {
        ullsam_set_error("mosaic_seams: memset failed");
        return -2;
    }
    if (S == 0 || max_rows == 0) return 0;
    mosaic_seams_kernel<<<dim3((unsigned)((max_rows + 3) / 4), (unsigned)S), 256, 0, s>>>(tiles, T, th, tw, base, G, seams, keys, counts,
                                                                                         (mz_u64)(cap - 1), max_pairs, areas, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mosaic_union(const unsigned long long* keys, const int* counts, long cap, const int* areas, long G, long num, long den,
                                   int* parent, int* flags, void* stream) {
    ULLSAM_CHECK(G >= 0 && G <= 2147483646L && cap >= 0 && cap <= (1L << 31), "mosaic_union: need 0 <= G <= 2^31 - 2 and 0 <= slots <= 2^31");
    ULLSAM_CHECK(num > 0 && num <= den && den < (1L << 31), "mosaic_union: need 0 < num <= den < 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    mosaic_iota_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, parent);
    ULLSAM_LAUNCH_CHECK();
    if (cap > 0 && G > 0) {
        mosaic_merge_kernel<<<mz_blocks(cap), 256, 0, s>>>(keys, counts, cap, areas, G, num, den, parent, flags);
        ULLSAM_LAUNCH_CHECK();
        mosaic_flatten_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, parent);
        ULLSAM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int ullsam_mosaic_stats(const int* tiles, int T, int th, int tw, const int* base, long G, const int* cores, int max_rows,
                                   const int* parent, int H, int W, int* areas_raw, int* boxes_raw, int* flags, void* stream) {
    MZ_TILES_CHECK("mosaic_stats");
    ULLSAM_CHECK(H > 0 && W > 0 && max_rows >= 0 && max_rows <= th, "mosaic_stats: need H, W > 0 and 0 <= max_rows <= th");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    mosaic_stats_init_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, areas_raw, boxes_raw);
    ULLSAM_LAUNCH_CHECK();
    if (max_rows == 0) return 0;
    mosaic_stats_kernel<<<dim3((unsigned)((max_rows + 3) / 4), (unsigned)T), 256, 0, s>>>(tiles, th, tw, base, G, cores, parent, H, W, areas_raw,
                                                                                         boxes_raw, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mosaic_compact(const int* areas_raw, const int* boxes_raw, const int* parent, long G, int min_visible_area,
                                     int* label_of_global, int* areas, int* boxes, int* K, void* stream) {
    ULLSAM_CHECK(G >= 0 && G <= 2147483646L, "mosaic_compact: need 0 <= G <= 2^31 - 2");
    mosaic_compact_kernel<<<1, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(areas_raw, boxes_raw, parent, G, min_visible_area, label_of_global,
                                                                               areas, boxes, K);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mosaic_paste(const int* tiles, int T, int th, int tw, const int* base, long G, const int* cores, int max_rows,
                                   const int* label_of_global, int H, int W, int* labels, void* stream) {
    MZ_TILES_CHECK("mosaic_paste");
    ULLSAM_CHECK(H > 0 && W > 0 && max_rows >= 0 && max_rows <= th, "mosaic_paste: need H, W > 0 and 0 <= max_rows <= th");
    if (max_rows == 0) return 0;
    const int vec = (((uintptr_t)tiles | (uintptr_t)labels) & 15) == 0 ? 1 : 0;
    mosaic_paste_kernel<<<dim3((unsigned)((max_rows + 3) / 4), (unsigned)T), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        tiles, th, tw, base, G, cores, label_of_global, H, W, vec, labels);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
