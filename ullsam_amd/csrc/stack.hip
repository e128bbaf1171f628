// Z-stacks and time-lapse series: the per-plane instance label maps linked along the third axis into 3-D objects (host form and definition:
// utils/stack.py; DESIGN.md "7b, continued (stacks)").  Integer work only -- integer atomics, no float anywhere -- so every output is a
// function of the planes alone: bit-exact with the numpy definition and identical from run to run.
//
// Ids.  Plane z holds local ids 0..K_z (0 = background); its global ids are base[z] + l for l > 0, base = the exclusive sum of the K_z,
// G = base[Z] <= 2^31 - 2, as in mosaic.hip.  Every table here is indexed by global id, entry 0 unused.
// Pairs.  One wave walks one row of plane z and the same row of plane z + 1, 64 pixels at a time, and sends ONE atomic per run of equal keys
// along the row (pair_table.h; a run of whole 64-pixel segments is carried in registers): the areas A(g) of plane z's labels over the whole
// plane, and the pair counts n(a, b), a in plane z, b in plane z + 1, both > 0, into the open-addressing table: key = g_a << 32 | g_b (never
// 0, and g_a < g_b always).
// Best partner.  One thread per slot.  A slot is a CANDIDATE when n > 0 and n * den >= num * u, u = A(a) + A(b) - n.  Every candidate offers
// its slot to succ[g_a] and to pred[g_b] with a compare-and-swap loop that keeps the better of the two slots under the strict order
//   (n1, u1, partner1) beats (n2, u2, partner2)  iff  n1 * u2 > n2 * u1, or they are equal and partner1 < partner2
// (64-bit products: n < 2^31, u < 2^32; two slots of one table never tie, they hold different keys; a hand-made table that repeats a key is
// decided by the smaller slot).  The order is strict and total, so what the word holds at the end is its maximum whatever the order of
// arrival.  A second kernel turns the slots into the partners' ids.
// Link.  mutual: (a, b) is linked iff succ[a] = b and pred[b] = a, so every id has at most one predecessor and the representative of g is the
// head of its chain: a read-only walk over pred / succ, at most Z steps, every step to a smaller id.  all: every candidate is a link and the
// representatives come from a union-find that hooks the LARGER root under the smaller one (mz_union, label_common.h), then a flatten pass.
// Stats.  One wave per row: voxels (64-bit), first and last plane and the inclusive XYXY box per representative, one atomicAdd per run, bounds
// sent only when a relaxed load says they would improve.
// Compaction.  One workgroup: keep = voxels != 0 and >= min_volume and last - first + 1 >= min_planes, renumbered 1..K by ascending
// representative; label_of_global[g] = final label of parent[g].
// Relabel.  volume[p] = label_of_global[g(z, plane_z[p])], 16 bytes per lane where both buffers allow it; indexed in 64 bits.
// An id outside 0..K_z reads as background and sets flags[0]; no table is indexed with it.
#include "pair_table.h"   // the runs of equal keys along a row and the pair table; through it label_common.h: the relaxed atomics, the union-find
#include <limits.h>

struct SkPlane {
    int b0, k;
    bool ok;
};
__device__ __forceinline__ SkPlane sk_plane(const int* __restrict__ base, int z, long G) {
    const int b0 = base[z], k = base[z + 1] - b0;
    return {b0, k, b0 >= 0 && k >= 0 && (long)b0 + k <= G};   // (base has to be the exclusive sum it is said to be: no table is indexed otherwise)
}

// ---- areas and pairs --------------------------------------------------------------------------------------------------------------------
// grid (ceil(H / 4), Z), block 256: one wave per row of plane z (and of plane z + 1 beside it)
__global__ __launch_bounds__(256) void stack_pairs_kernel(const int* __restrict__ planes, int Z, int H, int W, const int* __restrict__ base, long G,
                                                          mz_u64* __restrict__ keys, int* __restrict__ counts, mz_u64 mask, int max_pairs,
                                                          int* __restrict__ areas, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int z = blockIdx.y;
    if (y >= H || z >= Z) return;                        // wave-uniform
    const SkPlane pa = sk_plane(base, z, G);
    const bool next = z + 1 < Z;
    const SkPlane pb = next ? sk_plane(base, z + 1, G) : SkPlane{0, 0, true};
    if (!pa.ok || !pb.ok) {
        if (lane == 0) mz_store(flags + 0, 1);
        return;
    }
    const int* ra = planes + ((long)z * H + y) * W;
    const int* rb = ra + (long)H * W;                    // (read only when there is a next plane)
    auto add_a = [&](mz_u64 g, int, int n) { mz_add(areas + (long)g, n); };
    auto add_p = [&](mz_u64 k, int, int n) { mz_pair_add(k, n, keys, counts, mask, max_pairs, flags); };
    MzRun run_a = {0, 0, 0}, run_p = {0, 0, 0};
    bool bad = false;
    for (int xs = 0; xs < W; xs += 64) {
        const int x = xs + lane;
        int a = 0, b = 0;
        if (x < W) {
            a = ra[x];
            if (a < 0 || a > pa.k) { bad = true; a = 0; }
            if (next) {
                b = rb[x];
                if (b < 0 || b > pb.k) { bad = true; b = 0; }
            }
        }
        const mz_u64 ga = a > 0 ? (mz_u64)(pa.b0 + a) : 0, gb = b > 0 ? (mz_u64)(pb.b0 + b) : 0;
        mz_segment(run_a, ga, xs, lane, add_a);
        if (next) mz_segment(run_p, (ga && gb) ? ((ga << 32) | gb) : 0, xs, lane, add_p);
    }
    mz_flush(run_a, lane, add_a);
    mz_flush(run_p, lane, add_p);
    if (bad) mz_store(flags + 0, 1);
}

// ---- best partner -----------------------------------------------------------------------------------------------------------------------
struct SkCand {
    long a, b, n, u;
    bool ok;
};
// The slot's pair as a candidate; ok = false for an empty slot and for a pair below the threshold.  A key or a count that no pass over a stack
// writes (ids outside 1..G or not ascending, an overlap larger than an area) sets flags[0] and is no candidate.
__device__ __forceinline__ SkCand sk_cand(const mz_u64* __restrict__ keys, const int* __restrict__ counts, long i, const int* __restrict__ areas, long G,
                                          long num, long den, int* __restrict__ flags) {
    SkCand c = {0, 0, 0, 0, false};
    const mz_u64 k = keys[i];
    if (k == 0) return c;
    c.a = (long)(k >> 32);
    c.b = (long)(k & 0xffffffffull);
    c.n = counts[i];
    if (c.a < 1 || c.b > G || c.a >= c.b) {
        mz_store(flags + 0, 1);
        return c;
    }
    if (c.n <= 0) return c;
    const long aa = areas[c.a], ab = areas[c.b];
    if (aa < c.n || ab < c.n) {
        mz_store(flags + 0, 1);
        return c;
    }
    c.u = aa + ab - c.n;                                 // n <= u < 2^32
    c.ok = (mz_u64)c.n * (mz_u64)den >= (mz_u64)num * (mz_u64)c.u;
    return c;
}
// Does candidate slot i (n, u, partner p) beat the slot j that the word holds?  j was offered by a candidate too: its ids and areas are in range.
__device__ __forceinline__ bool sk_beats(long n, long u, long p, long i, int j, int side, const mz_u64* __restrict__ keys, const int* __restrict__ counts,
                                         const int* __restrict__ areas) {
    const mz_u64 kj = keys[j];
    const long aj = (long)(kj >> 32), bj = (long)(kj & 0xffffffffull), nj = counts[j];
    const long uj = (long)areas[aj] + (long)areas[bj] - nj;
    const mz_u64 l = (mz_u64)n * (mz_u64)uj, r = (mz_u64)nj * (mz_u64)u;
    if (l != r) return l > r;
    const long pj = side ? aj : bj;
    if (p != pj) return p < pj;
    return i < j;
}
__device__ __forceinline__ void sk_offer(int* word, long n, long u, long p, long i, int side, const mz_u64* __restrict__ keys, const int* __restrict__ counts,
                                         const int* __restrict__ areas) {
    int cur = mz_load(word);
    while (cur < 0 || (cur != (int)i && sk_beats(n, u, p, i, cur, side, keys, counts, areas))) {
        if (__hip_atomic_compare_exchange_strong(word, &cur, (int)i, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }                                                    // (a failed exchange left the word's value in cur: compare again)
}
__global__ __launch_bounds__(256) void stack_fill_kernel(long n, int* __restrict__ a, int* __restrict__ b, int v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    a[i] = v;
    b[i] = v;
}
// one thread per slot
__global__ __launch_bounds__(256) void stack_best_kernel(const mz_u64* __restrict__ keys, const int* __restrict__ counts, long cap,
                                                         const int* __restrict__ areas, long G, long num, long den, int* __restrict__ succ,
                                                         int* __restrict__ pred, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const SkCand c = sk_cand(keys, counts, i, areas, G, num, den, flags);
    if (!c.ok) return;
    sk_offer(succ + c.a, c.n, c.u, c.b, i, 0, keys, counts, areas);
    sk_offer(pred + c.b, c.n, c.u, c.a, i, 1, keys, counts, areas);
}
// one thread per id: the winning slots become the partners' ids (0: no candidate)
__global__ __launch_bounds__(256) void stack_partner_kernel(const mz_u64* __restrict__ keys, long cap, long n, int* __restrict__ succ, int* __restrict__ pred) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int s = succ[g], p = pred[g];
    succ[g] = (s >= 0 && s < cap) ? (int)(keys[s] & 0xffffffffull) : 0;
    pred[g] = (p >= 0 && p < cap) ? (int)(keys[p] >> 32) : 0;
}

// ---- links and representatives --------------------------------------------------------------------------------------------------------------
// one thread per id: the head of the chain of mutual links that ends in g
__global__ __launch_bounds__(256) void stack_chain_kernel(const int* __restrict__ succ, const int* __restrict__ pred, long G, int* __restrict__ parent,
                                                          int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i > G) return;
    long g = i;
    bool bad = false;
    while (g > 0) {
        const long a = pred[g];
        if (a < 0 || a > G) { bad = true; break; }
        if (a == 0 || succ[a] != g) break;               // no candidate, or a's best partner is another label: g is the head
        if (a >= g) { bad = true; break; }               // (a predecessor lives in the plane before: every step goes down, so the walk ends)
        g = a;
    }
    if (bad) mz_store(flags + 0, 1);
    parent[i] = (int)g;
}
__global__ __launch_bounds__(256) void stack_iota_kernel(long n, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}
// one thread per slot: every candidate is a link
__global__ __launch_bounds__(256) void stack_merge_kernel(const mz_u64* __restrict__ keys, const int* __restrict__ counts, long cap,
                                                          const int* __restrict__ areas, long G, long num, long den, int* __restrict__ parent,
                                                          int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const SkCand c = sk_cand(keys, counts, i, areas, G, num, den, flags);
    if (c.ok) mz_union(parent, (int)c.a, (int)c.b);
}
__global__ __launch_bounds__(256) void stack_flatten_kernel(long n, int* __restrict__ parent) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mz_store(parent + i, mz_find(parent, (int)i));   // (whatever a concurrent reader finds at i is an ancestor of i)
}

// ---- stats ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stack_stats_init_kernel(long n, long* __restrict__ voxels, int* __restrict__ zrange, int* __restrict__ boxes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    voxels[i] = 0;
    zrange[2 * i + 0] = INT_MAX;
    zrange[2 * i + 1] = -1;
    boxes[4 * i + 0] = INT_MAX;
    boxes[4 * i + 1] = INT_MAX;
    boxes[4 * i + 2] = -1;
    boxes[4 * i + 3] = -1;
}
// grid (ceil(H / 4), Z), block 256: one wave per row of a plane
__global__ __launch_bounds__(256) void stack_stats_kernel(const int* __restrict__ planes, int Z, int H, int W, const int* __restrict__ base, long G,
                                                          const int* __restrict__ parent, long* __restrict__ voxels, int* __restrict__ zrange,
                                                          int* __restrict__ boxes, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int z = blockIdx.y;
    if (y >= H || z >= Z) return;                        // wave-uniform
    const SkPlane pl = sk_plane(base, z, G);
    if (!pl.ok) {
        if (lane == 0) mz_store(flags + 0, 1);
        return;
    }
    const int* src = planes + ((long)z * H + y) * W;
    auto emit = [&](mz_u64 key, int x0, int n) {
        const long v = (long)key;
        mz_add(voxels + v, n);
        const int xb = x0 + n - 1;
        int* zr = zrange + 2 * v;
        int* bx = boxes + 4 * v;
        mz_send_min(zr + 0, z);
        mz_send_max(zr + 1, z);
        mz_send_min(bx + 0, x0);
        mz_send_min(bx + 1, y);
        mz_send_max(bx + 2, xb);
        mz_send_max(bx + 3, y);
    };
    MzRun run = {0, 0, 0};
    bool bad = false;
    for (int xs = 0; xs < W; xs += 64) {
        const int x = xs + lane;
        int l = x < W ? src[x] : 0;
        if (l < 0 || l > pl.k) { bad = true; l = 0; }
        int p = l > 0 ? parent[pl.b0 + l] : 0;
        if (p < 0 || p > G) { bad = true; p = 0; }       // (a representative is an id)
        mz_segment(run, (mz_u64)p, xs, lane, emit);
    }
    mz_flush(run, lane, emit);
    if (bad) mz_store(flags + 0, 1);
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sk_keep(const long* __restrict__ vox, const int* __restrict__ zr, long g, int min_planes, long min_volume) {
    const long v = vox[g];
    return v != 0 && v >= min_volume && (long)zr[2 * g + 1] - (long)zr[2 * g] + 1 >= (long)min_planes;
}
// grid 1, block 256: thread t owns the ids [1 + t * ceil(G / 256), ...) -- a contiguous share, so the final labels ascend with the representative.
__global__ __launch_bounds__(256) void stack_compact_kernel(const long* __restrict__ vox_raw, const int* __restrict__ zr_raw, const int* __restrict__ boxes_raw,
                                                            const int* __restrict__ parent, long G, int min_planes, long min_volume,
                                                            int* __restrict__ label_of_global, long* __restrict__ voxels, int* __restrict__ zrange,
                                                            int* __restrict__ boxes, int* __restrict__ K) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    const long share = (G + 255) / 256;
    const long g0 = min(1 + t * share, G + 1), g1 = min(g0 + share, G + 1);
    int c = 0;
    for (long g = g0; g < g1; ++g) c += (parent[g] == g && sk_keep(vox_raw, zr_raw, g, min_planes, min_volume)) ? 1 : 0;
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
    for (long g = g0; g < g1; ++g) {                     // first the representatives ...
        if (parent[g] != g) continue;
        const bool keep = sk_keep(vox_raw, zr_raw, g, min_planes, min_volume);
        mz_store(label_of_global + g, keep ? k + 1 : 0);
        if (keep) {
            voxels[k] = vox_raw[g];
            zrange[2 * (long)k + 0] = zr_raw[2 * g + 0];
            zrange[2 * (long)k + 1] = zr_raw[2 * g + 1];
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

// ---- relabel --------------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(H * W / 1024), Z), block 256: four pixels per thread.  vec: both buffers start on a 16-byte boundary and H * W is a multiple of 4.
__global__ __launch_bounds__(256) void stack_relabel_kernel(const int* __restrict__ planes, int Z, long HW, const int* __restrict__ base, long G,
                                                            const int* __restrict__ log, int vec, int* __restrict__ volume) {
    const int z = blockIdx.y;
    if (z >= Z) return;
    const SkPlane pl = sk_plane(base, z, G);
    const int k = pl.ok ? pl.k : 0;                      // (a base that is no exclusive sum: every id reads as background)
    const int* src = planes + (long)z * HW;
    int* dst = volume + (long)z * HW;
    const long p0 = (long)blockIdx.x * 1024;
    if (vec) {
        const long p = p0 + 4 * (long)threadIdx.x;
        if (p < HW) {                                    // (HW is a multiple of 4: p + 3 < HW)
            const int4 v = *reinterpret_cast<const int4*>(src + p);
            int4 o;
            o.x = mz_look(v.x, pl.b0, k, log);
            o.y = mz_look(v.y, pl.b0, k, log);
            o.z = mz_look(v.z, pl.b0, k, log);
            o.w = mz_look(v.w, pl.b0, k, log);
            *reinterpret_cast<int4*>(dst + p) = o;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long p = p0 + j * 256 + threadIdx.x;
            if (p < HW) dst[p] = mz_look(src[p], pl.b0, k, log);
        }
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------------
#define SK_STACK_CHECK(what)                                                                                                   \
    ULLSAM_CHECK(Z >= 1 && Z <= 65535 && H >= 1 && H <= 46340 && W >= 1 && W <= 46340 && G >= 0 && G <= 2147483646L,             \
                 what ": need 1 <= Z <= 65535, 1 <= H, W <= 46340, 0 <= G <= 2^31 - 2")
#define SK_TABLE_CHECK(what) \
    ULLSAM_CHECK(G >= 0 && G <= 2147483646L && cap >= 0 && cap <= (1L << 31), what ": need 0 <= G <= 2^31 - 2 and 0 <= slots <= 2^31"); \
    ULLSAM_CHECK(num > 0 && num <= den && den < (1L << 31), what ": need 0 < num <= den < 2^31")

extern "C" int ullsam_stack_pairs(const int* planes, int Z, int H, int W, const int* base, long G, unsigned long long* keys, int* counts, long cap,
                                  int max_pairs, int* areas, int* flags, void* stream) {
    SK_STACK_CHECK("stack_pairs");
    ULLSAM_CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && max_pairs >= 1 && 2L * max_pairs <= cap && cap <= (1L << 31),
                 "stack_pairs: the capacity must be a power of two with 2 * max_pairs <= capacity <= 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!mz_zero(keys, (size_t)cap * 8, s) || !mz_zero(counts, (size_t)cap * 4, s) || !mz_zero(areas, (size_t)(G + 1) * 4, s) || !mz_zero(flags, 16, s)) {
        ullsam_set_error("stack_pairs: memset failed");
        return -2;
    }
    stack_pairs_kernel<<<dim3((unsigned)((H + 3) / 4), (unsigned)Z), 256, 0, s>>>(planes, Z, H, W, base, G, keys, counts, (mz_u64)(cap - 1), max_pairs, areas,
                                                                                 flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_stack_best(const unsigned long long* keys, const int* counts, long cap, const int* areas, long G, long num, long den, int* succ,
                                 int* pred, int* flags, void* stream) {
    SK_TABLE_CHECK("stack_best");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    stack_fill_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, succ, pred, -1);
    ULLSAM_LAUNCH_CHECK();
    if (cap > 0 && G > 0) {
        stack_best_kernel<<<mz_blocks(cap), 256, 0, s>>>(keys, counts, cap, areas, G, num, den, succ, pred, flags);
        ULLSAM_LAUNCH_CHECK();
    }
    stack_partner_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(keys, cap, G + 1, succ, pred);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_stack_link(const int* succ, const int* pred, const unsigned long long* keys, const int* counts, long cap, const int* areas, long G,
                                 long num, long den, int* parent, int* flags, void* stream) {
    SK_TABLE_CHECK("stack_link");
    ULLSAM_CHECK((succ != nullptr) == (pred != nullptr), "stack_link: succ and pred come together (mutual) or not at all (every candidate links)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (succ) {
        stack_chain_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(succ, pred, G, parent, flags);
        ULLSAM_LAUNCH_CHECK();
        return 0;
    }
    stack_iota_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, parent);
    ULLSAM_LAUNCH_CHECK();
    if (cap > 0 && G > 0) {
        stack_merge_kernel<<<mz_blocks(cap), 256, 0, s>>>(keys, counts, cap, areas, G, num, den, parent, flags);
        ULLSAM_LAUNCH_CHECK();
        stack_flatten_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, parent);
        ULLSAM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int ullsam_stack_stats(const int* planes, int Z, int H, int W, const int* base, long G, const int* parent, long* voxels_raw, int* zrange_raw,
                                  int* boxes_raw, int* flags, void* stream) {
    SK_STACK_CHECK("stack_stats");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    stack_stats_init_kernel<<<mz_blocks(G + 1), 256, 0, s>>>(G + 1, voxels_raw, zrange_raw, boxes_raw);
    ULLSAM_LAUNCH_CHECK();
    stack_stats_kernel<<<dim3((unsigned)((H + 3) / 4), (unsigned)Z), 256, 0, s>>>(planes, Z, H, W, base, G, parent, voxels_raw, zrange_raw, boxes_raw, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_stack_compact(const long* voxels_raw, const int* zrange_raw, const int* boxes_raw, const int* parent, long G, int min_planes,
                                    long min_volume, int* label_of_global, long* voxels, int* zrange, int* boxes, int* K, void* stream) {
    ULLSAM_CHECK(G >= 0 && G <= 2147483646L, "stack_compact: need 0 <= G <= 2^31 - 2");
    stack_compact_kernel<<<1, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(voxels_raw, zrange_raw, boxes_raw, parent, G, min_planes, min_volume,
                                                                              label_of_global, voxels, zrange, boxes, K);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_stack_relabel(const int* planes, int Z, int H, int W, const int* base, long G, const int* label_of_global, int* volume,
                                    void* stream) {
    SK_STACK_CHECK("stack_relabel");
    const long HW = (long)H * W;
    const int vec = ((((uintptr_t)planes | (uintptr_t)volume) & 15) == 0 && (HW & 3) == 0) ? 1 : 0;
    stack_relabel_kernel<<<dim3((unsigned)((HW + 1023) / 1024), (unsigned)Z), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(planes, Z, HW, base, G,
                                                                                                                             label_of_global, vec, volume);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
