// Splitting the touching objects of an instance label image: a watershed of every instance's own depth map, written without a flood (host form and
// definition: utils/split.py; DESIGN.md "7b, continued (splitting)").  Integer work only -- no float anywhere, ordinary vector stores, integer atomics
// -- and every choice is a maximum under a strict total order, so every output is a function of the labels alone: bit-exact with the numpy
// definition and identical from run to run whatever the order of arrival.
//
// D2 = inner_distance(labels) (distance.hip), p = the row-major index of a pixel, key(p) = (D2[p], -p): larger D2 first, then the smaller index.
//   ascent   up[p] = the pixel of greatest key among p and its 8 neighbours with p's label (p itself on the background).  One thread per pixel; a
//            workgroup covers SP_TW x SP_TH pixels and either stages them with a one-pixel halo in LDS or reads global memory (the A/B of the route).
//   flatten  up[p] = the root of p's chain, in place: a racing reader sees the old pointer or the root, both ancestors.  At most `steps` hops.
//   passes   every pixel looks right, down-left, down and down-right; where the neighbour has its label and another root, min(D2, D2) goes into the
//            pair table under (smaller root << 32 | larger root) with a maximum per key (pair_table.h mz_pair_max).
//   round    best: over the table's slots, both ends of an edge whose ends lie in different components send S << 32 | (0xFFFFFFFF - the other
//            representative) to their own representative's word with a 64-bit atomicMax -- the greatest (S, -rep Y).  decide: every root with a word
//            takes it back to 0, and where key(X) < key(Y) and sqrt(P_X) - sqrt(S) <= h (exactly, in 64-bit integers) it writes up[X] = Y and raises
//            `changed`.  Both tests read D2 only, so all absorptions of a round are decided on the state at its start; they point to strictly
//            greater keys, so no cycle forms.  The caller flattens and repeats until a round changes nothing.
//   collect  the representatives (up[p] = p on a labelled pixel) are counted, then written as label << 32 | p in no particular order (one atomic
//            per wave); the caller sorts them.
//   relabel  part i of the sorted list gets id i + 1: parent, peak_r2, peak_xy, parts_of, and every pixel takes the id of its root.
// flags i32 [8]: [0] = a label below 0 or above K, or a table entry outside the frame (skipped; nothing is indexed with it), [1] = a pair was
// refused, [2] = the pairs claimed, [3] = a chain longer than its bound, [4] = the representatives counted, [5] = the cursor of the list.
#include "pair_table.h"
#include <stdint.h>

#define SP_TW 64
#define SP_TH 4
#define SP_BLOCK (SP_TW * SP_TH)

// ---- ascent ---------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / SP_TW), ceil(H / SP_TH)), block SP_BLOCK
template <bool LDS>
__global__ __launch_bounds__(SP_BLOCK) void split_ascent_kernel(const int* __restrict__ labels, const int* __restrict__ d2, int H, int W, long K,
                                                                int* __restrict__ up, int* __restrict__ flags) {
    constexpr int LW = SP_TW + 2, LH = SP_TH + 2;
    __shared__ int s_lab[LDS ? LH * LW : 1];
    __shared__ int s_d2[LDS ? LH * LW : 1];
    const int x0 = blockIdx.x * SP_TW, y0 = blockIdx.y * SP_TH;
    if (LDS) {
        for (int i = threadIdx.x; i < LH * LW; i += SP_BLOCK) {
            const int gy = y0 - 1 + i / LW, gx = x0 - 1 + i % LW;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            s_lab[i] = in ? labels[(long)gy * W + gx] : 0;   // (0 is no live label: the frame's outside never matches)
            s_d2[i] = in ? d2[(long)gy * W + gx] : 0;
        }
        __syncthreads();
    }
    const int lx = threadIdx.x % SP_TW, ly = threadIdx.x / SP_TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const int p = y * W + x;                              // H * W < 2^30
    const int l = labels[p];
    if (!mz_live(l, K)) {
        if (l != 0) mz_store(flags + 0, 1);
        up[p] = p;
        return;
    }
    int bd = d2[p], bq = p;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            int nl, nd;
            if (LDS) {
                const int i = (ly + 1 + dy) * LW + (lx + 1 + dx);
                nl = s_lab[i];
                nd = s_d2[i];
            } else {
                const int yy = y + dy, xx = x + dx;
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                nl = labels[p + dy * W + dx];
                nd = d2[p + dy * W + dx];
            }
            const int q = p + dy * W + dx;
            if (nl == l && (nd > bd || (nd == bd && q < bq))) {
                bd = nd;
                bq = q;
            }
        }
    }
    up[p] = bq;
}

// ---- flatten --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split_flatten_kernel(long n, long steps, int* __restrict__ up, int* __restrict__ flags) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int r = mz_load(up + p);
    if (r == (int)p) return;
    for (long s = 0; s < steps; ++s) {
        if (r < 0 || r >= n) {                            // (a hand-made map: the ascent writes no such pointer)
            mz_store(flags + 0, 1);
            return;
        }
        const int nx = mz_load(up + r);
        if (nx == r) {
            mz_store(up + p, r);
            return;
        }
        r = nx;
    }
    mz_store(flags + 3, 1);
}

// ---- passes ---------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 256), H), block 256; up is flattened
__global__ __launch_bounds__(256) void split_passes_kernel(const int* __restrict__ labels, const int* __restrict__ d2, const int* __restrict__ up, int H,
                                                           int W, long K, mz_u64* __restrict__ keys, int* __restrict__ vals, mz_u64 mask, int max_pairs,
                                                           int* __restrict__ flags) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int p = y * W + x;
    const int l = labels[p];
    if (!mz_live(l, K)) return;
    const int dp = d2[p];
    const unsigned rp = (unsigned)up[p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dx = j == 0 ? 1 : j - 2, dy = j == 0 ? 0 : 1;   // right, down-left, down, down-right
        const int xx = x + dx, yy = y + dy;
        if (xx < 0 || xx >= W || yy >= H) continue;
        const int q = p + dy * W + dx;
        if (labels[q] != l) continue;
        const unsigned rq = (unsigned)up[q];
        if (rq == rp) continue;
        const mz_u64 key = ((mz_u64)min(rp, rq) << 32) | (mz_u64)max(rp, rq);
        mz_pair_max(key, min(dp, d2[q]), keys, vals, mask, max_pairs, flags);
    }
}

// ---- one round of merging -------------------------------------------------------------------------------------------------------------------
// one thread per slot; up is flattened: up[a] is the representative of a's component
__global__ __launch_bounds__(256) void split_best_kernel(const mz_u64* __restrict__ keys, const int* __restrict__ vals, long cap, const int* __restrict__ up,
                                                         long n, mz_u64* __restrict__ best, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const mz_u64 k = keys[i];
    if (k == 0) return;
    const long a = (long)(k >> 32), b = (long)(k & 0xffffffffull);
    const int s = vals[i];
    if (a >= n || b >= n || s < 0) {                      // (a hand-made table: the pass kernel writes no such entry)
        mz_store(flags + 0, 1);
        return;
    }
    const unsigned X = (unsigned)up[a], Y = (unsigned)up[b];
    if (X == Y || X >= n || Y >= n) return;
    mz_send_max(best + X, ((mz_u64)(unsigned)s << 32) | (mz_u64)(0xFFFFFFFFu - Y));
    mz_send_max(best + Y, ((mz_u64)(unsigned)s << 32) | (mz_u64)(0xFFFFFFFFu - X));
}
// one thread per pixel; only a root reads and clears its own word and writes its own pointer
__global__ __launch_bounds__(256) void split_decide_kernel(const int* __restrict__ labels, const int* __restrict__ d2, long n, long K, long h,
                                                           mz_u64* __restrict__ best, int* __restrict__ up, int* __restrict__ changed) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    if (!mz_live(labels[p], K) || up[p] != (int)p) return;
    const mz_u64 w = best[p];
    if (w == 0) return;
    best[p] = 0;
    const long S = (long)(w >> 32);
    const long Y = (long)(0xFFFFFFFFu - (unsigned)(w & 0xffffffffull));
    if (Y >= n) return;                                   // (a word the best kernel did not write: the caller zeroes `best` once)
    const long P = d2[p], PY = d2[Y];
    if (!(P < PY || (P == PY && p > Y))) return;          // key(X) < key(Y)
    const long t = P - S - h * h;                         // sqrt(P) - sqrt(S) <= h  <=>  t <= 0 or t^2 <= 4 h^2 S
    if (t > 0 && (mz_u64)t * (mz_u64)t > 4ull * (mz_u64)(h * h) * (mz_u64)S) return;
    mz_store(up + p, (int)Y);
    mz_store(changed, 1);
}

// ---- numbering ------------------------------------------------------------------------------------------------------------------------------
// list == nullptr: flags[4] += the representatives; otherwise list[flags[5]++] = label << 32 | p while there is room
__global__ __launch_bounds__(256) void split_collect_kernel(const int* __restrict__ labels, const int* __restrict__ up, long n, long K, mz_u64* __restrict__ list,
                                                            long room, int* __restrict__ flags) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int l = 0;
    bool rep = false;
    if (p < n) {
        l = labels[p];
        rep = mz_live(l, K) && up[p] == (int)p;
    }
    const mz_u64 m = __ballot(rep);
    if (m == 0) return;                                   // wave-uniform
    const int leader = __builtin_ctzll(m);
    int at = 0;
    if (lane == leader) at = __hip_atomic_fetch_add(flags + (list ? 5 : 4), __builtin_popcountll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    at = __shfl(at, leader, 64);
    if (!rep || !list) return;
    const long slot = (long)at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (slot < room) list[slot] = ((mz_u64)(unsigned)l << 32) | (mz_u64)(unsigned)p;
}
// one thread per part of the sorted list
__global__ __launch_bounds__(256) void split_tables_kernel(const mz_u64* __restrict__ list, long parts, const int* __restrict__ d2, long n, int W, long K,
                                                           int* __restrict__ newid, int* __restrict__ parent, int* __restrict__ peak_r2,
                                                           int* __restrict__ peak_xy, int* __restrict__ parts_of, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= parts) return;
    const mz_u64 k = list[i];
    const long l = (long)(k >> 32), p = (long)(k & 0xffffffffull);
    parent[i] = 0;
    peak_r2[i] = 0;
    peak_xy[2 * i + 0] = -1;
    peak_xy[2 * i + 1] = -1;
    if (l < 1 || l > K || p >= n) {                       // (a hand-made list)
        mz_store(flags + 0, 1);
        return;
    }
    parent[i] = (int)l;
    peak_r2[i] = d2[p];
    peak_xy[2 * i + 0] = (int)(p % W);
    peak_xy[2 * i + 1] = (int)(p / W);
    newid[p] = (int)(i + 1);
    mz_add(parts_of + (l - 1), 1);
}
// one thread per pixel: the id of its root (newid is written at the representatives only, and read there only)
__global__ __launch_bounds__(256) void split_relabel_kernel(const int* __restrict__ labels, const int* __restrict__ up, const int* __restrict__ newid, long n,
                                                            long K, int* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v = 0;
    if (mz_live(labels[p], K)) {
        const int r = up[p];
        if (r >= 0 && r < n) v = newid[r];
    }
    out[p] = v;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define SP_FRAME_CHECK(what) \
    ULLSAM_CHECK(H >= 1 && H <= 32767 && W >= 1 && W <= 32767 && K >= 0 && K <= 2147483647L, what ": need 1 <= H, W <= 32767 and 0 <= K <= 2^31 - 1")
#define SP_FLAT_CHECK(what) \
    ULLSAM_CHECK(n >= 1 && n <= 32767L * 32767L && K >= 0 && K <= 2147483647L, what ": need 1 <= n <= 32767^2 and 0 <= K <= 2^31 - 1")

extern "C" int ullsam_split_ascent(const int* labels, const int* d2, int H, int W, long K, int route, int* up, int* flags, void* stream) {
    SP_FRAME_CHECK("split_ascent");
    ULLSAM_CHECK(route >= 0 && route <= 2, "split_ascent: route in 0..2");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((W + SP_TW - 1) / SP_TW), (unsigned)((H + SP_TH - 1) / SP_TH));
    if (route != 2) split_ascent_kernel<true><<<grid, SP_BLOCK, 0, s>>>(labels, d2, H, W, K, up, flags);
    else split_ascent_kernel<false><<<grid, SP_BLOCK, 0, s>>>(labels, d2, H, W, K, up, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split_flatten(int* up, long n, long steps, int* flags, void* stream) {
    ULLSAM_CHECK(n >= 1 && n <= 32767L * 32767L && steps >= 0 && steps <= n, "split_flatten: need 1 <= n <= 32767^2 and 0 <= steps <= n");
    split_flatten_kernel<<<mz_blocks(n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(n, steps, up, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split_passes(const int* labels, const int* d2, const int* up, int H, int W, long K, unsigned long long* keys, int* vals, long cap,
                                   int max_pairs, int* flags, void* stream) {
    SP_FRAME_CHECK("split_passes");
    ULLSAM_CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && max_pairs >= 1 && 2L * max_pairs <= cap, "split_passes: cap must be a power of two >= 2 * max_pairs");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!mz_zero(keys, (size_t)cap * 8, s) || !mz_zero(vals, (size_t)cap * 4, s)) {
        ullsam_set_error("split_passes: memset failed");
        return -2;
    }
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H);
    split_passes_kernel<<<grid, 256, 0, s>>>(labels, d2, up, H, W, K, reinterpret_cast<mz_u64*>(keys), vals, (mz_u64)(cap - 1), max_pairs, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split_round(const unsigned long long* keys, const int* vals, long cap, const int* labels, const int* d2, long n, long K, int h,
                                  unsigned long long* best, int* up, int* changed, int* flags, void* stream) {
    SP_FLAT_CHECK("split_round");
    ULLSAM_CHECK(cap >= 0 && h >= 0 && h <= 32767, "split_round: need cap >= 0 and 0 <= h <= 32767");
    if (cap == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    split_best_kernel<<<mz_blocks(cap), 256, 0, s>>>(reinterpret_cast<const mz_u64*>(keys), vals, cap, up, n, reinterpret_cast<mz_u64*>(best), flags);
    ULLSAM_LAUNCH_CHECK();
    split_decide_kernel<<<mz_blocks(n), 256, 0, s>>>(labels, d2, n, K, (long)h, reinterpret_cast<mz_u64*>(best), up, changed);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split_collect(const int* labels, const int* up, long n, long K, unsigned long long* list, long room, int* flags, void* stream) {
    SP_FLAT_CHECK("split_collect");
    ULLSAM_CHECK(room >= 0 && (list != nullptr || room == 0), "split_collect: room >= 0, and 0 without a list");
    split_collect_kernel<<<mz_blocks(n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(labels, up, n, K, reinterpret_cast<mz_u64*>(list), room, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split_relabel(const unsigned long long* list, long parts, const int* labels, const int* d2, const int* up, int H, int W, long K,
                                    int* newid, int* out, int* parent, int* peak_r2, int* peak_xy, int* parts_of, int* flags, void* stream) {
    SP_FRAME_CHECK("split_relabel");
    ULLSAM_CHECK(parts >= 0 && parts <= (long)H * W && K <= 2147483646L, "split_relabel: need 0 <= parts <= H * W and K <= 2^31 - 2");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n = (long)H * W;
    if (!mz_zero(parts_of, (size_t)K * 4, s)) {
        ullsam_set_error("split_relabel: memset failed");
        return -2;
    }
    if (parts > 0) {
        split_tables_kernel<<<mz_blocks(parts), 256, 0, s>>>(reinterpret_cast<const mz_u64*>(list), parts, d2, n, W, K, newid, parent, peak_r2, peak_xy, parts_of,
                                                             flags);
        ULLSAM_LAUNCH_CHECK();
    }
    split_relabel_kernel<<<mz_blocks(n), 256, 0, s>>>(labels, up, newid, n, K, out);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
