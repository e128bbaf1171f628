// Polygons to an instance label image: exact scanline rasterisation in fixed point (host form and definition: utils/raster.py; DESIGN.md "7b,
// continued (rasterising)").  Integer work only -- ordinary vector stores, integer atomics (sums, minima, maxima, which do not depend on the order
// of arrival) -- so every output is a function of the input alone: bit-exact with the numpy definition and identical from run to run.
//
// q i32 [N, 2]: the vertices (x, y) in 1/256 pixel, |q| <= 65535 * 256; start i32 [R + 1]: ring r owns q[start[r] : start[r + 1]]; ring_label i32 [R]
// in 1..K.  Edge i runs from vertex i to the next vertex of its ring (the last one back to the first).  The centre of pixel (x, y) is
// (256 x + 128, 256 y + 128).
//   edges    one thread per edge: its ring by a search in start, the next vertex, the label, the rows 0..H - 1 whose centre line it crosses
//            (min(y0, y1) <= 256 y + 128 < max(y0, y1)): row0 and cnt.  An exclusive scan of cnt gives off and C, the crossings.
//   scan     three launches: the sum of every block of RS_CHUNK values, an exclusive scan of those sums by one workgroup (64-bit carry: a total
//            above 2^31 - 1 is a status bit), the offsets.
//   keys     one thread per crossing: its edge by a search in off, the row, xs = clamp(ceil(A / B), 0, W) with the endpoints ordered by y,
//            d = y1 - y0, cy = 256 y + 128, A = (x0 - 128) d + (cy - y0)(x1 - x0), B = 256 d; key = label << 32 | row << 16 | xs.
//   covered  the keys sorted: entries 2 j, 2 j + 1 are span j = [xs_a, xs_b) of one (label, row).  covered[label - 1] += xs_b - xs_a: a thread sums
//            a run of consecutive spans, the wave merges its lanes label by label, one atomic each; len[j] = xs_b - xs_a for the per-pixel paint.
//   paint    atomicMax(raw[y, x], rank[label - 1] + 1) over every span: one wave per span, lanes striding its pixels (form 0), or one lane per
//            pixel over a scan of the span lengths (form 1, grid-stride: the pixel total stays on the device).
//   finish   labels = label_of[raw], row-major; area and the inclusive XYXY box per label: a wave takes 512 consecutive pixels, merges its lanes
//            label by label and joins the parts of a label that goes on, so a label that fills them costs one atomic set.
// flags i32 [4]: [0] = status bits: 1 = a ring_label outside 1..K, 2 = a coordinate beyond 65535 * 256, 4 = a total above 2^31 - 1, 8 = an index or a
// value that left its table (skipped; nothing is indexed with it); [1] = C.
#include "label_common.h"
#include <stdint.h>

#define RS_BLOCK 256
#define RS_PER 8
#define RS_CHUNK (RS_BLOCK * RS_PER)
#define RS_LIMIT (65535 * 256)
#define RS_MAX_SIDE 32767
#define RS_MAX_IDS 65535
#define RS_BAD_LABEL 1
#define RS_BAD_COORD 2
#define RS_TOO_MANY 4
#define RS_BAD_INDEX 8
#define RS_INT_MAX 2147483647L

__device__ __forceinline__ bool rs_coord(int v) { return v >= -RS_LIMIT && v <= RS_LIMIT; }
// ceil(a / 256) for either sign (>> on a negative int is the arithmetic shift)
__device__ __forceinline__ int rs_ceil256(int a) { return (a + 255) >> 8; }
// the largest i in 0..n - 1 with table[i] <= t (0 when there is none); every index it reads lies in 0..n - 1 whatever the table holds; n >= 1
__device__ __forceinline__ long rs_find(const int* __restrict__ table, long n, long t) {
    long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if ((long)table[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- scan -----------------------------------------------------------------------------------------------------------------------------------
// (block_exscan<RS_BLOCK>: label_common.h)
// the RS_PER values of a thread, bounds checked; a value outside 0..32767 counts as 0 (a status bit): a block's sum stays below 2^26
__device__ __forceinline__ int rs_take(const int* __restrict__ vals, long n, long i0, int (&c)[RS_PER], int* __restrict__ flags) {
    int sum = 0;
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        int v = i0 + j < n ? vals[i0 + j] : 0;
        if (v < 0 || v > RS_MAX_SIDE) {
            mz_or(flags, RS_BAD_INDEX);
            v = 0;
        }
        c[j] = v;
        sum += v;
    }
    return sum;
}
__global__ __launch_bounds__(RS_BLOCK) void raster_sums_kernel(const int* __restrict__ vals, long n, int* __restrict__ sums, int* __restrict__ flags) {
    int c[RS_PER], total;
    const int mine = rs_take(vals, n, (long)blockIdx.x * RS_CHUNK + (long)threadIdx.x * RS_PER, c, flags);
    (void)block_exscan<RS_BLOCK>(mine, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums[b] = the sum of the blocks before b; *total = the sum of all; either is held at 2^31 - 1, with a status bit, when it is larger
__global__ __launch_bounds__(RS_BLOCK) void raster_scan_sums_kernel(int* __restrict__ sums, long nb, int* __restrict__ total, int* __restrict__ flags) {
    long carry = 0;
    for (long base = 0; base < nb; base += RS_BLOCK) {
        const long i = base + threadIdx.x;
        const long v = i < nb ? (long)sums[i] : 0;
        long all;
        const long ex = carry + block_exscan<RS_BLOCK>(v, all);
        if (i < nb) sums[i] = (int)(ex < RS_INT_MAX ? ex : RS_INT_MAX);
        carry += all;
    }
    if (threadIdx.x == 0) {
        if (carry > RS_INT_MAX) mz_or(flags, RS_TOO_MANY);
        mz_store(total, (int)(carry < RS_INT_MAX ? carry : RS_INT_MAX));
    }
}
__global__ __launch_bounds__(RS_BLOCK) void raster_offsets_kernel(const int* __restrict__ vals, long n, const int* __restrict__ sums, int* __restrict__ off,
                                                                  int* __restrict__ flags) {
    int c[RS_PER], total;
    const long i0 = (long)blockIdx.x * RS_CHUNK + (long)threadIdx.x * RS_PER;
    const int mine = rs_take(vals, n, i0, c, flags);
    long at = (long)sums[blockIdx.x] + block_exscan<RS_BLOCK>(mine, total);
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        if (i0 + j < n) off[i0 + j] = (int)(at < RS_INT_MAX ? at : RS_INT_MAX);
        at += c[j];
    }
}

// ---- edges ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_BLOCK) void raster_edges_kernel(const int* __restrict__ q, long N, const int* __restrict__ start, long R,
                                                                const int* __restrict__ ring_label, int H, long K, int* __restrict__ row0,
                                                                int* __restrict__ cnt, int* __restrict__ nxt, int* __restrict__ elab, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= N) return;
    const long r = rs_find(start, R, i);                  // (start[R] is read as start[r + 1] only)
    const long s0 = start[r], s1 = start[r + 1];
    int r0 = 0, c = 0, lab = 0;
    long j = i;
    if (!(s0 >= 0 && s0 <= i && i < s1 && s1 <= N)) mz_or(flags, RS_BAD_INDEX);   // (a hand-made start)
    else {
        j = i + 1 < s1 ? i + 1 : s0;
        lab = ring_label[r];
        const int x0 = q[2 * i], y0 = q[2 * i + 1], x1 = q[2 * j], y1 = q[2 * j + 1];
        if (lab < 1 || lab > K) {
            mz_or(flags, RS_BAD_LABEL);
            lab = 0;
        } else if (!(rs_coord(x0) && rs_coord(y0) && rs_coord(x1) && rs_coord(y1))) {
            mz_or(flags, RS_BAD_COORD);
            lab = 0;
        } else {
            const int lo = max(rs_ceil256(min(y0, y1) - 128), 0), hi = min(rs_ceil256(max(y0, y1) - 128), H);
            if (hi > lo) {
                r0 = lo;
                c = hi - lo;
            }
        }
    }
    row0[i] = r0;
    cnt[i] = c;
    nxt[i] = (int)j;
    elab[i] = lab;
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------------------
// one thread per crossing; a crossing whose tables do not agree gets the key 0 (label 0: the later stages skip it)
__global__ __launch_bounds__(RS_BLOCK) void raster_keys_kernel(const int* __restrict__ q, long N, const int* __restrict__ row0, const int* __restrict__ cnt,
                                                               const int* __restrict__ nxt, const int* __restrict__ elab, const int* __restrict__ off, long C,
                                                               int H, int W, long K, long long* __restrict__ keys, int* __restrict__ flags) {
    const long c = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (c >= C) return;
    const long e = rs_find(off, N, c);
    const long t = c - (long)off[e], y = (long)row0[e] + t, j = nxt[e];
    const int lab = elab[e];
    long long key = 0;
    if (!(t >= 0 && t < (long)cnt[e] && mz_in(y, H) && mz_in(j, N))) mz_or(flags, RS_BAD_INDEX);
    else if (lab < 1 || lab > K) mz_or(flags, RS_BAD_LABEL);
    else {
        long x0 = q[2 * e], y0 = q[2 * e + 1], x1 = q[2 * j], y1 = q[2 * j + 1];
        if (!(rs_coord((int)x0) && rs_coord((int)y0) && rs_coord((int)x1) && rs_coord((int)y1))) mz_or(flags, RS_BAD_COORD);
        else {
            if (y0 > y1) {                                // the endpoints ordered by y: the value does not depend on the edge's direction
                long s = x0; x0 = x1; x1 = s;
                s = y0; y0 = y1; y1 = s;
            }
            const long cy = 256 * y + 128;
            if (!(y0 <= cy && cy < y1)) mz_or(flags, RS_BAD_INDEX);    // (a hand-made row0)
            else {
                const long d = y1 - y0, a = (x0 - 128) * d + (cy - y0) * (x1 - x0), b = 256 * d;    // |a| < 2^52
                long xs = a / b;                          // truncates towards zero: the ceiling already where a < 0
                if (a % b > 0) ++xs;
                xs = xs < 0 ? 0 : xs > W ? W : xs;
                key = (long long)lab << 32 | (long long)y << 16 | (long long)xs;
            }
        }
    }
    keys[c] = key;
}

// ---- spans ----------------------------------------------------------------------------------------------------------------------------------
// span j of the sorted keys -> (label, row, xa, xb); false (and a status bit) where the two keys are no span of the frame
__device__ __forceinline__ bool rs_span(const long long* __restrict__ keys, long j, int H, int W, long K, int& lab, int& y, int& xa, int& xb,
                                        int* __restrict__ flags) {
    const long long a = keys[2 * j], b = keys[2 * j + 1];
    lab = (int)(a >> 32);
    y = (int)(a >> 16) & 0xFFFF;
    xa = (int)a & 0xFFFF;
    xb = (int)b & 0xFFFF;
    const bool ok = a >= 0 && (a >> 16) == (b >> 16) && lab >= 1 && lab <= K && y < H && xa <= xb && xb <= W;
    if (!ok) mz_or(flags, RS_BAD_INDEX);
    return ok;
}
// the wave merges its lanes label by label: one atomic for every distinct label of the wave, however the spans arrive.  Sums of integers: the
// order of arrival does not matter.
__device__ __forceinline__ void rs_send(int lab, int n, int* __restrict__ covered) {
    mz_u64 todo = __ballot(lab >= 1 && n > 0);
    while (todo) {                                        // wave-uniform
        const int key = __shfl(lab, __builtin_ctzll(todo), 64);
        const bool mine = lab == key;
        int v = mine ? n : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63) == 0) mz_add(covered + (key - 1), v);
        todo &= ~__ballot(mine);
    }
}
// RS_RUN consecutive spans a thread, summed while the label stays the same (the keys are sorted: it mostly does)
#define RS_RUN 4
__global__ __launch_bounds__(RS_BLOCK) void raster_covered_kernel(const long long* __restrict__ keys, long S, int H, int W, long K, int* __restrict__ covered,
                                                                  int* __restrict__ len, int* __restrict__ flags) {
    const long j0 = ((long)blockIdx.x * RS_BLOCK + threadIdx.x) * RS_RUN;
    int cur = -1, sum = 0;                                // (4 spans of at most 32767 pixels on 64 lanes: the wave's sum stays below 2^31)
#pragma unroll
    for (int r = 0; r < RS_RUN; ++r) {
        const long j = j0 + r;
        int lab = -1, n = 0;
        if (j < S) {
            int y, xa, xb;
            if (rs_span(keys, j, H, W, K, lab, y, xa, xb, flags)) n = xb - xa;
            else lab = -1;
            if (len) len[j] = n;
        }
        if (__ballot(lab != cur) != 0) {                  // some lane leaves its run: the wave sends what it holds (wave-uniform)
            rs_send(cur, sum, covered);
            cur = lab;
            sum = 0;
        }
        sum += n;
    }
    rs_send(cur, sum, covered);
}

// ---- paint ----------------------------------------------------------------------------------------------------------------------------------
// the value a span paints: its label's rank + 1, or 0 (a status bit) for a rank outside 0..K - 1
__device__ __forceinline__ int rs_value(const int* __restrict__ rank, int lab, long K, int* __restrict__ flags) {
    const int rk = rank[lab - 1];
    if (mz_in(rk, K)) return rk + 1;
    mz_or(flags, RS_BAD_INDEX);
    return 0;
}
// form 0: one wave per span, its lanes striding the pixels
__global__ __launch_bounds__(RS_BLOCK) void raster_paint_waves_kernel(const long long* __restrict__ keys, long S, const int* __restrict__ rank, int H, int W,
                                                                      long K, int* __restrict__ raw, int* __restrict__ flags) {
    const long j = (long)blockIdx.x * (RS_BLOCK / 64) + (threadIdx.x >> 6);
    if (j >= S) return;                                   // wave-uniform
    int lab, y, xa, xb;
    if (!rs_span(keys, j, H, W, K, lab, y, xa, xb, flags)) return;
    const int v = rs_value(rank, lab, K, flags);
    if (v == 0) return;
    int* __restrict__ row = raw + (long)y * W;
    for (int x = xa + (int)(threadIdx.x & 63); x < xb; x += 64) mz_max(row + x, v);
}
// form 1: one lane per pixel of the spans, found by a search in poff = the exclusive scan of len; *total = the pixels (it stays on the device)
__global__ __launch_bounds__(RS_BLOCK) void raster_paint_pixels_kernel(const long long* __restrict__ keys, long S, const int* __restrict__ rank,
                                                                       const int* __restrict__ poff, const int* __restrict__ total, int H, int W, long K,
                                                                       int* __restrict__ raw, int* __restrict__ flags) {
    const long P = mz_load(total), step = (long)gridDim.x * RS_BLOCK;
    for (long t = (long)blockIdx.x * RS_BLOCK + threadIdx.x; t < P; t += step) {
        const long j = rs_find(poff, S, t);
        int lab, y, xa, xb;
        if (!rs_span(keys, j, H, W, K, lab, y, xa, xb, flags)) continue;
        const long x = (long)xa + (t - (long)poff[j]);
        if (!(x >= xa && x < xb)) {                       // (a hand-made poff)
            mz_or(flags, RS_BAD_INDEX);
            continue;
        }
        const int v = rs_value(rank, lab, K, flags);
        if (v) mz_max(raw + (long)y * W + x, v);
    }
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_BLOCK) void raster_init_kernel(long K, int* __restrict__ area, int* __restrict__ box) {
    const long k = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (k >= K) return;
    area[k] = 0;
    box[4 * k + 0] = 2147483647;
    box[4 * k + 1] = 2147483647;
    box[4 * k + 2] = -1;
    box[4 * k + 3] = -1;
}
// What a wave holds for one label before it sends it: the pixel count and the bounds (wave-uniform).  A bound goes out as an atomic only when a
// plain load says it improves: after the first few waves of a label nearly none does, and the row of a busy label is not hit by five
// operations that its L2 channel takes one after the other.
struct RsPart {
    int key, cnt, x0, y0, x1, y1;
};
__device__ __forceinline__ void rs_flush(RsPart& c, int lane, int* __restrict__ area, int* __restrict__ box) {
    if (c.key > 0 && lane == 0) {
        int* __restrict__ b = box + 4 * (long)(c.key - 1);
        mz_add(area + (c.key - 1), c.cnt);
        const int bx0 = b[0], by0 = b[1], bx1 = b[2], by1 = b[3];   // plain loads: a stale bound only sends an atomic that was not needed
        if (bx0 > c.x0) (void)mz_min(b + 0, c.x0);
        if (by0 > c.y0) (void)mz_min(b + 1, c.y0);
        if (bx1 < c.x1) mz_max(b + 2, c.x1);
        if (by1 < c.y1) mz_max(b + 3, c.y1);
    }
    c.key = 0;
    c.cnt = 0;
}
__device__ __forceinline__ int rs_wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int rs_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
// A wave takes RS_SEGS segments of 64 consecutive pixels.  In every segment it merges its lanes label by label (count and bounds) and keeps the
// last label's part back: where the next segment continues that label the parts join, so a label that fills the wave's pixels costs one atomic set.
#define RS_SEGS 8
__global__ __launch_bounds__(RS_BLOCK) void raster_finish_kernel(const int* __restrict__ raw, int H, int W, const int* __restrict__ label_of, long K,
                                                                 int* __restrict__ labels, int* __restrict__ area, int* __restrict__ box,
                                                                 int* __restrict__ flags) {
    const long n = (long)H * W;
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * (RS_BLOCK / 64) + (threadIdx.x >> 6)) * (64 * RS_SEGS);
    if (base >= n) return;                                // wave-uniform
    RsPart part = {0, 0, 0, 0, 0, 0};
    int ls[RS_SEGS];
#pragma unroll
    for (int s = 0; s < RS_SEGS; ++s) {                   // all the loads of the wave first: they overlap
        const long p = base + 64 * s + lane;
        ls[s] = p < n ? raw[p] : 0;
    }
#pragma unroll
    for (int s = 0; s < RS_SEGS; ++s) {
        const long p = base + 64 * s + lane;
        int l = 0;
        if (p < n) {
            if (!mz_in(ls[s], K + 1)) mz_or(flags, RS_BAD_INDEX);
            else {
                l = label_of[ls[s]];
                if (!mz_in(l, K + 1)) {
                    mz_or(flags, RS_BAD_INDEX);
                    l = 0;
                }
            }
            labels[p] = l;
        }
        ls[s] = l;
    }
#pragma unroll
    for (int s = 0; s < RS_SEGS; ++s) {
        const long p = base + 64 * s + lane;              // (x and y of a lane past the frame are never used: its label is 0)
        const unsigned pu = (unsigned)p, yu = pu / (unsigned)W;   // H * W < 2^30: one 32-bit division a pixel
        const int l = ls[s], x = (int)(pu - yu * (unsigned)W), y = (int)yu;
        const bool one_row = __shfl(y, 0, 64) == __shfl(y, 63, 64);
        mz_u64 todo = __ballot(l > 0);
        while (todo) {                                    // wave-uniform
            const int first = __builtin_ctzll(todo);
            const int key = __shfl(l, first, 64);
            const bool mine = l == key;
            const mz_u64 m = __ballot(mine);
            const int last = 63 - __builtin_clzll(m);
            const int y0 = __shfl(y, first, 64), y1 = __shfl(y, last, 64);   // p grows with the lane, and y with p
            int x0, x1;
            if (one_row) {                                // ... and so does x inside one row
                x0 = __shfl(x, first, 64);
                x1 = __shfl(x, last, 64);
            } else {
                x0 = rs_wave_min(mine ? x : 2147483647);
                x1 = rs_wave_max(mine ? x : -1);
            }
            if (key == part.key) {
                part.cnt += __builtin_popcountll(m);
                part.x0 = min(part.x0, x0);
                part.y0 = min(part.y0, y0);
                part.x1 = max(part.x1, x1);
                part.y1 = max(part.y1, y1);
            } else {
                rs_flush(part, lane, area, box);
                part.key = key;
                part.cnt = __builtin_popcountll(m);
                part.x0 = x0;
                part.y0 = y0;
                part.x1 = x1;
                part.y1 = y1;
            }
            todo &= ~m;
        }
    }
    rs_flush(part, lane, area, box);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define RS_FRAME_CHECK(what) ULLSAM_CHECK(H >= 1 && W >= 1 && H <= RS_MAX_SIDE && W <= RS_MAX_SIDE, what ": need 1 <= H, W <= 32767")
#define RS_IDS_CHECK(what) ULLSAM_CHECK(K >= 0 && K <= RS_MAX_IDS, what ": need 0 <= K <= 65535")
#define RS_COUNT_CHECK(what, n) ULLSAM_CHECK((n) >= 0 && (n) <= RS_INT_MAX, what ": a count must lie in 0..2^31 - 1")
#define RS_MEMSET(what, p, bytes)                                   \
    do {                                                            \
        if (hipMemsetAsync((p), 0, (bytes), s) != hipSuccess) {     \
            ullsam_set_error(what ": memset failed");               \
            return -2;                                              \
        }                                                           \
    } while (0)

static int rs_scan(const int* vals, long n, int* off, int* sums, int* total, int* flags, hipStream_t s) {
    const long nb = (n + RS_CHUNK - 1) / RS_CHUNK;
    raster_sums_kernel<<<(unsigned)nb, RS_BLOCK, 0, s>>>(vals, n, sums, flags);
    ULLSAM_LAUNCH_CHECK();
    raster_scan_sums_kernel<<<1, RS_BLOCK, 0, s>>>(sums, nb, total, flags);
    ULLSAM_LAUNCH_CHECK();
    raster_offsets_kernel<<<(unsigned)nb, RS_BLOCK, 0, s>>>(vals, n, sums, off, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_raster_scan(const int* vals, long n, int* off, int* sums, int* total, int* flags, void* stream) {
    RS_COUNT_CHECK("raster_scan", n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) {
        RS_MEMSET("raster_scan", total, 4);
        return 0;
    }
    return rs_scan(vals, n, off, sums, total, flags, s);
}

extern "C" int ullsam_raster_edges(const int* q, long N, const int* start, long R, const int* ring_label, int H, int W, long K, int* row0, int* cnt, int* nxt,
                                   int* elab, int* off, int* sums, int* flags, void* stream) {
    RS_FRAME_CHECK("raster_edges");
    RS_IDS_CHECK("raster_edges");
    RS_COUNT_CHECK("raster_edges", N);
    ULLSAM_CHECK(R >= 0 && R <= N && (N == 0 || R >= 1), "raster_edges: need 0 <= R <= N, and a ring where there is a vertex");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (N == 0) {
        RS_MEMSET("raster_edges", flags + 1, 4);
        return 0;
    }
    raster_edges_kernel<<<mz_blocks(N, RS_BLOCK), RS_BLOCK, 0, s>>>(q, N, start, R, ring_label, H, K, row0, cnt, nxt, elab, flags);
    ULLSAM_LAUNCH_CHECK();
    return rs_scan(cnt, N, off, sums, flags + 1, flags, s);
}

extern "C" int ullsam_raster_keys(const int* q, long N, const int* row0, const int* cnt, const int* nxt, const int* elab, const int* off, long C, int H, int W,
                                  long K, long long* keys, int* flags, void* stream) {
    RS_FRAME_CHECK("raster_keys");
    RS_IDS_CHECK("raster_keys");
    RS_COUNT_CHECK("raster_keys", N);
    RS_COUNT_CHECK("raster_keys", C);
    ULLSAM_CHECK(C == 0 || N >= 1, "raster_keys: crossings without an edge");
    if (C == 0) return 0;
    raster_keys_kernel<<<mz_blocks(C, RS_BLOCK), RS_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(q, N, row0, cnt, nxt, elab, off, C, H, W, K, keys, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// keys sorted; S = C / 2 spans.  covered i32 [K] is zeroed here; len i32 [S] may be null
extern "C" int ullsam_raster_covered(const long long* keys, long C, int H, int W, long K, int* covered, int* len, int* flags, void* stream) {
    RS_FRAME_CHECK("raster_covered");
    RS_IDS_CHECK("raster_covered");
    RS_COUNT_CHECK("raster_covered", C);
    ULLSAM_CHECK(C % 2 == 0, "raster_covered: the crossings of closed rings come in pairs");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (K > 0) RS_MEMSET("raster_covered", covered, (size_t)K * 4);
    if (C == 0) return 0;
    raster_covered_kernel<<<mz_blocks((C / 2 + RS_RUN - 1) / RS_RUN, RS_BLOCK), RS_BLOCK, 0, s>>>(keys, C / 2, H, W, K, covered, len, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// raw i32 [H, W] is zeroed here.  form 0: one wave per span; form 1: one lane per pixel, poff i32 [S] = the exclusive scan of len, total i32 [1] its sum
extern "C" int ullsam_raster_paint(const long long* keys, long C, const int* rank, int H, int W, long K, int form, const int* poff, const int* total, int* raw,
                                   int* flags, void* stream) {
    RS_FRAME_CHECK("raster_paint");
    RS_IDS_CHECK("raster_paint");
    RS_COUNT_CHECK("raster_paint", C);
    ULLSAM_CHECK(C % 2 == 0, "raster_paint: the crossings of closed rings come in pairs");
    ULLSAM_CHECK(form == 0 || (form == 1 && (C == 0 || (poff && total))), "raster_paint: form is 0 (waves) or 1 (pixels, with poff and total)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RS_MEMSET("raster_paint", raw, (size_t)H * W * 4);
    const long S = C / 2;
    if (S == 0 || K == 0) return 0;
    if (form == 0) raster_paint_waves_kernel<<<mz_blocks(S * 64, RS_BLOCK), RS_BLOCK, 0, s>>>(keys, S, rank, H, W, K, raw, flags);
    else raster_paint_pixels_kernel<<<2048, RS_BLOCK, 0, s>>>(keys, S, rank, poff, total, H, W, K, raw, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// label_of i32 [K + 1]: the label of every raw value (label_of[0] = 0)
extern "C" int ullsam_raster_finish(const int* raw, int H, int W, const int* label_of, long K, int* labels, int* area, int* box, int* flags, void* stream) {
    RS_FRAME_CHECK("raster_finish");
    RS_IDS_CHECK("raster_finish");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (K > 0) {
        raster_init_kernel<<<mz_blocks(K, RS_BLOCK), RS_BLOCK, 0, s>>>(K, area, box);
        ULLSAM_LAUNCH_CHECK();
    }
    raster_finish_kernel<<<mz_blocks(((long)H * W + RS_SEGS - 1) / RS_SEGS, RS_BLOCK), RS_BLOCK, 0, s>>>(raw, H, W, label_of, K, labels, area, box, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
