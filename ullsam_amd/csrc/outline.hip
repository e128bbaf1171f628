// Outlines of an instance label image: every instance as closed polygon loops on the pixel lattice (host form and definition: utils/outline.py;
// DESIGN.md "7b, continued (outlines)").  Integer work only -- ordinary vector stores, integer atomics (sums, which do not depend on the order of
// arrival) -- so every output is a function of the labels alone: bit-exact with the numpy definition and identical from run to run.
//
// p = y * W + x; side s of pixel p: 0 = top (east), 1 = right (south), 2 = bottom (west), 3 = left (north), the instance on the right of travel;
// the id of the edge is 4 * p + s.
//   sides       mask[p]: bit s = side s of a labelled pixel faces a pixel that is not of its label (the frame's outside included).  An exclusive
//               scan of popcount(mask) gives off[p]: the compact index of edge (p, s) is off[p] + popcount(mask[p] & ((1 << s) - 1)), so compact
//               order is id order and an edge finds its successor's compact index without a search.
//   scan        three launches: the sum of every block of OL_CHUNK values, an exclusive scan of those sums by one workgroup, the offsets.
//   successors  one thread per pixel, every set side: the local rule on the pixels ahead-left and ahead-right of the head; the edge also writes its
//               direction into pdir[successor], so corners are known without a predecessor search.
//   rank        pointer doubling on the cycles of succ in ping-pong buffers, one 16-byte word an edge: after r rounds mn[e] = the smallest index
//               among the 2^r edges from e on, pos[e] = the steps from e to its first occurrence, jump[e] = the edge 2^r steps ahead.  ceil(log2 E)
//               rounds make every window at least as long as any cycle: mn is the leader, and rank = (length - pos) mod length with length =
//               pos[succ[leader]] + 1.
//   collect     the leaders as label << 32 | compact index, in no particular order (one atomic per wave); the caller sorts them.
//   loops       edges and area2 per loop: a thread sums a run of consecutive edges, the wave merges its lanes loop by loop, one atomic pair each.
//   order       every edge goes to slot estart[loop] + rank of a rank-ordered copy (its id and whether it is a corner); a scan of the corner flags
//               over that copy is the ordered compaction: loop after loop, every loop in travel order from its leader.
//   parents     one thread per loop: a hole walks left from its leader's pixel while the label lasts, takes the loop of that pixel's left side, and
//               repeats from that loop's leader until it stands on an outer loop.
// flags i32 [8]: [0] = a label below 0 or above K (the pixel counts as background), or an index that left its table (skipped; nothing is indexed with
// it), [1] = E, [2] = the corners, [3] = the leaders, [4] = the cursor of the list, [5] = a parent chain longer than L.
#include "label_common.h"
#include <stdint.h>

#define OL_BLOCK 256
#define OL_PER 8
#define OL_CHUNK (OL_BLOCK * OL_PER)

// ---- scan -----------------------------------------------------------------------------------------------------------------------------------
// (block_exscan<OL_BLOCK>: label_common.h)
template <bool POP> __device__ __forceinline__ int ol_value(unsigned char b) { return POP ? __builtin_popcount((unsigned)b & 15u) : (b != 0); }

// the OL_PER values of a thread, bounds checked; returns their sum
template <bool POP> __device__ __forceinline__ int ol_take(const unsigned char* __restrict__ vals, long n, long i0, int (&c)[OL_PER]) {
    int sum = 0;
#pragma unroll
    for (int j = 0; j < OL_PER; ++j) {
        c[j] = i0 + j < n ? ol_value<POP>(vals[i0 + j]) : 0;
        sum += c[j];
    }
    return sum;
}
template <bool POP> __global__ __launch_bounds__(OL_BLOCK) void outline_sums_kernel(const unsigned char* __restrict__ vals, long n, int* __restrict__ sums) {
    int c[OL_PER], total;
    const int mine = ol_take<POP>(vals, n, (long)blockIdx.x * OL_CHUNK + (long)threadIdx.x * OL_PER, c);
    (void)block_exscan<OL_BLOCK>(mine, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums[b] = the sum of the blocks before b; *total = the sum of all
__global__ __launch_bounds__(OL_BLOCK) void outline_scan_sums_kernel(int* __restrict__ sums, long nb, int* __restrict__ total) {
    int carry = 0;
    for (long base = 0; base < nb; base += OL_BLOCK) {
        const long i = base + threadIdx.x;
        const int v = i < nb ? sums[i] : 0;
        int all;
        const int ex = block_exscan<OL_BLOCK>(v, all);
        if (i < nb) sums[i] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) mz_store(total, carry);
}
template <bool POP>
__global__ __launch_bounds__(OL_BLOCK) void outline_offsets_kernel(const unsigned char* __restrict__ vals, long n, const int* __restrict__ sums,
                                                                   int* __restrict__ off) {
    int c[OL_PER], total;
    const long i0 = (long)blockIdx.x * OL_CHUNK + (long)threadIdx.x * OL_PER;
    const int mine = ol_take<POP>(vals, n, i0, c);
    int at = sums[blockIdx.x] + block_exscan<OL_BLOCK>(mine, total);
#pragma unroll
    for (int j = 0; j < OL_PER; ++j) {
        if (i0 + j < n) off[i0 + j] = at;
        at += c[j];
    }
}

// ---- sides ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OL_BLOCK) void outline_sides_kernel(const int* __restrict__ labels, int H, int W, long K, unsigned char* __restrict__ mask,
                                                                 int* __restrict__ flags) {
    const long p = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (p >= (long)H * W) return;
    const int l = labels[p];
    unsigned m = 0;
    if (l < 0 || l > K) mz_store(flags + 0, 1);
    else if (l > 0) {
        const int x = (int)(p % W), y = (int)(p / W);
        m = (unsigned)(y == 0 || labels[p - W] != l) | (unsigned)(x == W - 1 || labels[p + 1] != l) << 1 |
            (unsigned)(y == H - 1 || labels[p + W] != l) << 2 | (unsigned)(x == 0 || labels[p - 1] != l) << 3;
    }
    mask[p] = (unsigned char)m;
}

// ---- successors -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ol_is(const int* __restrict__ labels, int H, int W, int x, int y, int l) {
    return x >= 0 && x < W && y >= 0 && y < H && labels[(long)y * W + x] == l;
}
// one thread per pixel
__global__ __launch_bounds__(OL_BLOCK) void outline_successors_kernel(const int* __restrict__ labels, int H, int W, const unsigned char* __restrict__ mask,
                                                                      const int* __restrict__ off, long E, int conn, int* __restrict__ eid,
                                                                      int* __restrict__ succ, unsigned char* __restrict__ pdir, int* __restrict__ flags) {
    const long p = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (p >= (long)H * W) return;
    const unsigned m = mask[p] & 15u;
    if (m == 0) return;
    const int l = labels[p];
    const int x = (int)(p % W), y = (int)(p / W);
    long e = off[p];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (!(m >> s & 1u)) continue;
        const int lx = x + (s == 0 || s == 1 ? 1 : -1), ly = y + (s == 1 || s == 2 ? 1 : -1);       // ahead-left
        const int rx = x + (s == 0 ? 1 : s == 2 ? -1 : 0), ry = y + (s == 1 ? 1 : s == 3 ? -1 : 0);  // ahead-right
        const bool al = ol_is(labels, H, W, lx, ly, l), ar = ol_is(labels, H, W, rx, ry, l);
        const bool left = conn == 8 ? al : (ar && al), straight = conn == 8 ? (!al && ar) : (ar && !al);
        const long tp = left ? (long)ly * W + lx : straight ? (long)ry * W + rx : p;
        const int ts = left ? (s + 3) & 3 : straight ? s : (s + 1) & 3;
        const unsigned tm = mask[tp] & 15u;
        const long t = (long)off[tp] + __builtin_popcount(tm & ((1u << ts) - 1u));
        if (!mz_in(e, E) || !mz_in(t, E) || !(tm >> ts & 1u)) {            // (hand-made masks or offsets)
            mz_store(flags + 0, 1);
        } else {
            eid[e] = (int)(4 * p + s);
            succ[e] = (int)t;
            pdir[t] = (unsigned char)s;
        }
        ++e;
    }
}

// ---- leader and rank ------------------------------------------------------------------------------------------------------------------------
// the state of an edge in one 16-byte word (one gather a round): x = mn, y = pos, z = jump
__global__ __launch_bounds__(OL_BLOCK) void outline_rank_init_kernel(const int* __restrict__ succ, long E, int4* __restrict__ st, int* __restrict__ flags) {
    const long e = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (e >= E) return;
    int j = succ[e];
    if (!mz_in(j, E)) {                                   // (a hand-made map)
        mz_store(flags + 0, 1);
        j = (int)e;
    }
    st[e] = make_int4((int)e, 0, j, 0);
}
// one round: window 2^r -> 2^(r + 1); reads a, writes b
__global__ __launch_bounds__(OL_BLOCK) void outline_rank_round_kernel(long E, int step, const int4* __restrict__ a, int4* __restrict__ b) {
    const long e = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int4 me = a[e];
    const int4 far = a[me.z];                             // z in 0..E - 1: the init kernel saw to it, and a jump of a jump stays there
    const bool take = far.x < me.x;                       // (a tie keeps the first half: the first occurrence)
    b[e] = make_int4(take ? far.x : me.x, take ? far.y + step : me.y, far.z, 0);
}
// leader and rank from the state; counts the leaders (flags[3]) and the corners (flags[2]), one atomic per wave each
__global__ __launch_bounds__(OL_BLOCK) void outline_rank_finish_kernel(const int* __restrict__ succ, const int* __restrict__ eid,
                                                                       const unsigned char* __restrict__ pdir, long E, const int4* __restrict__ st,
                                                                       int* __restrict__ leader, int* __restrict__ rank, int* __restrict__ flags) {
    const long e = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    bool lead = false, corner = false;
    if (e < E) {
        const int4 me = st[e];
        int r = 0;
        if (me.y != 0) {
            const int j = succ[me.x];                     // the leader's successor is one step short of a whole turn
            if (mz_in(j, E)) r = st[j].y + 1 - me.y;
        }
        leader[e] = me.x;
        rank[e] = r;
        lead = me.x == (int)e;
        corner = (int)pdir[e] != (eid[e] & 3);
    }
    const mz_u64 ml = __ballot(lead), mc = __ballot(corner);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && ml) mz_add(flags + 3, __builtin_popcountll(ml));
    if (lane == 0 && mc) mz_add(flags + 2, __builtin_popcountll(mc));
}

// ---- the loops ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OL_BLOCK) void outline_collect_kernel(const int* __restrict__ labels, long n, const int* __restrict__ eid,
                                                                   const int* __restrict__ leader, long E, mz_u64* __restrict__ list, long room,
                                                                   int* __restrict__ flags) {
    const long e = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool is = false;
    long p = 0;
    if (e < E && leader[e] == (int)e) {
        p = (long)(eid[e] >> 2);
        is = mz_in(p, n);
        if (!is) mz_store(flags + 0, 1);
    }
    const mz_u64 m = __ballot(is);
    if (m == 0) return;                                   // wave-uniform
    const int first = __builtin_ctzll(m);
    int at = 0;
    if (lane == first) at = __hip_atomic_fetch_add(flags + 4, __builtin_popcountll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    at = __shfl(at, first, 64);
    if (!is) return;
    const long slot = (long)at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (slot < room) list[slot] = ((mz_u64)(unsigned)labels[p] << 32) | (mz_u64)(unsigned)e;
    else mz_store(flags + 0, 1);
}


// the loop of edge e, or -1 (a hand-made table)
__device__ __forceinline__ int ol_loop(const int* __restrict__ leader, const int* __restrict__ loop_of, long E, long L, long e) {
    const int l = leader[e];
    if (!mz_in(l, E)) return -1;
    const int lp = loop_of[l];
    return mz_in(lp, L) ? lp : -1;
}
// OL_RUN consecutive edges a thread, summed while the loop stays the same; then the wave merges its lanes key by key: one atomic pair for every
// distinct loop of the wave, however the edges arrive.  Sums of integers: the order of arrival does not matter.
#define OL_RUN 4
__device__ __forceinline__ void ol_send(int lp, int cnt, long long sum, int* __restrict__ edges, long long* __restrict__ area2) {
    mz_u64 todo = __ballot(lp >= 0);
    while (todo) {                                        // wave-uniform
        const int key = __shfl(lp, __builtin_ctzll(todo), 64);
        const bool mine = lp == key;
        int c = mine ? cnt : 0;
        long long v = mine ? sum : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            c += __shfl_xor(c, d, 64);
            v += __shfl_xor(v, d, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            mz_add(edges + key, c);
            mz_add64(area2 + key, v);
        }
        todo &= ~__ballot(mine);
    }
}
__global__ __launch_bounds__(OL_BLOCK) void outline_loops_kernel(const int* __restrict__ eid, const int* __restrict__ leader, const int* __restrict__ loop_of,
                                                                 long E, long L, int W, int* __restrict__ edges, long long* __restrict__ area2,
                                                                 int* __restrict__ flags) {
    const long e0 = ((long)blockIdx.x * OL_BLOCK + threadIdx.x) * OL_RUN;
    int cur = -1, cnt = 0;
    long long sum = 0;
#pragma unroll
    for (int j = 0; j < OL_RUN; ++j) {
        const long e = e0 + j;
        int lp = -1;
        long long cross = 0;
        if (e < E) {
            lp = ol_loop(leader, loop_of, E, L, e);
            if (lp < 0) mz_store(flags + 0, 1);
            const int id = eid[e], s = id & 3;
            const int p = id >> 2, x = p % W, y = p / W;
            cross = s == 0 ? -y : s == 1 ? x + 1 : s == 2 ? y + 1 : -x;   // x_t * y_h - x_h * y_t of the unit edge
        }
        if (__ballot(lp != cur) != 0) {                   // some lane leaves its run: the wave sends what it holds (wave-uniform)
            ol_send(cur, cnt, sum, edges, area2);
            cur = lp;
            cnt = 0;
            sum = 0;
        }
        if (lp >= 0) {
            ++cnt;
            sum += cross;
        }
    }
    ol_send(cur, cnt, sum, edges, area2);
}

// every edge into its slot of the rank-ordered copy
__global__ __launch_bounds__(OL_BLOCK) void outline_order_kernel(const int* __restrict__ eid, const unsigned char* __restrict__ pdir,
                                                                 const int* __restrict__ leader, const int* __restrict__ rank, const int* __restrict__ loop_of,
                                                                 const int* __restrict__ estart, long E, long L, int* __restrict__ reid,
                                                                 unsigned char* __restrict__ corner, int* __restrict__ flags) {
    const long e = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int lp = ol_loop(leader, loop_of, E, L, e);
    const long slot = lp < 0 ? -1 : (long)estart[lp] + rank[e];
    if (!mz_in(slot, E)) {
        mz_store(flags + 0, 1);
        return;
    }
    const int id = eid[e];
    reid[slot] = id;
    corner[slot] = (unsigned char)((int)pdir[e] != (id & 3));
}
// the ordered compaction: the tail of every corner edge of the rank-ordered copy
__global__ __launch_bounds__(OL_BLOCK) void outline_vertices_kernel(const int* __restrict__ reid, const unsigned char* __restrict__ corner,
                                                                    const int* __restrict__ coff, long E, int W, long N, int* __restrict__ vertices) {
    const long i = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= E || !corner[i]) return;
    const long at = coff[i];
    if (!mz_in(at, N)) return;
    const int id = reid[i], s = id & 3, p = id >> 2;
    vertices[2 * at + 0] = p % W + (s == 1 || s == 2);
    vertices[2 * at + 1] = p / W + (s == 2 || s == 3);
}

// ---- parents --------------------------------------------------------------------------------------------------------------------------------
// one thread per loop; lead i32 [L] = the compact index of every loop's leader
__global__ __launch_bounds__(OL_BLOCK) void outline_parents_kernel(const int* __restrict__ labels, int H, int W, const unsigned char* __restrict__ mask,
                                                                   const int* __restrict__ off, const int* __restrict__ eid, const int* __restrict__ leader,
                                                                   const int* __restrict__ loop_of, const int* __restrict__ lead,
                                                                   const long long* __restrict__ area2, long E, long L, int* __restrict__ parent,
                                                                   int* __restrict__ flags) {
    const long i = (long)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= L) return;
    long cur = i;
    for (long hops = 0; area2[cur] <= 0; ++hops) {
        const int le = lead[cur];
        if (hops >= L || !mz_in(le, E)) {                 // (every hop moves strictly left: L hops mean a hand-made table)
            mz_store(flags + 5, 1);
            break;
        }
        long p = (long)(eid[le] >> 2);
        if (!mz_in(p, (long)H * W)) {
            mz_store(flags + 0, 1);
            break;
        }
        const int l = labels[p];
        int x = (int)(p % W);
        while (x > 0 && labels[p - 1] == l) {
            --x;
            --p;
        }
        const long e = (long)off[p] + __builtin_popcount((unsigned)mask[p] & 7u);   // the left side of that pixel
        const int nxt = mz_in(e, E) ? ol_loop(leader, loop_of, E, L, e) : -1;
        if (nxt < 0) {
            mz_store(flags + 0, 1);
            break;
        }
        cur = nxt;
    }
    parent[i] = (int)cur;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define OL_MAX_PIXELS (1L << 29)
#define OL_FRAME_CHECK(what) ULLSAM_CHECK(H >= 1 && W >= 1 && (long)H * W < OL_MAX_PIXELS, what ": need 1 <= H, W and H * W < 2^29")
#define OL_EDGES_CHECK(what) ULLSAM_CHECK(E >= 0 && E < 4 * OL_MAX_PIXELS, what ": need 0 <= E < 2^31")

static long ol_chunks(long n) { return (n + OL_CHUNK - 1) / OL_CHUNK; }

template <bool POP> static int ol_scan(const unsigned char* vals, long n, int* off, int* sums, int* total, hipStream_t s) {
    const long nb = ol_chunks(n);
    outline_sums_kernel<POP><<<(unsigned)nb, OL_BLOCK, 0, s>>>(vals, n, sums);
    ULLSAM_LAUNCH_CHECK();
    outline_scan_sums_kernel<<<1, OL_BLOCK, 0, s>>>(sums, nb, total);
    ULLSAM_LAUNCH_CHECK();
    outline_offsets_kernel<POP><<<(unsigned)nb, OL_BLOCK, 0, s>>>(vals, n, sums, off);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_outline_sides(const int* labels, int H, int W, long K, unsigned char* mask, int* off, int* sums, int* flags, void* stream) {
    OL_FRAME_CHECK("outline_sides");
    ULLSAM_CHECK(K >= 0 && K <= 2147483647L, "outline_sides: need 0 <= K <= 2^31 - 1");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n = (long)H * W;
    outline_sides_kernel<<<mz_blocks(n, OL_BLOCK), OL_BLOCK, 0, s>>>(labels, H, W, K, mask, flags);
    ULLSAM_LAUNCH_CHECK();
    return ol_scan<true>(mask, n, off, sums, flags + 1, s);
}

extern "C" int ullsam_outline_scan(const unsigned char* vals, long n, int* off, int* sums, int* total, void* stream) {
    ULLSAM_CHECK(n >= 0 && n < 4 * OL_MAX_PIXELS, "outline_scan: need 0 <= n < 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) {
        if (hipMemsetAsync(total, 0, 4, s) != hipSuccess) {
            ullsam_set_error("outline_scan: memset failed");
            return -2;
        }
        return 0;
    }
    return ol_scan<false>(vals, n, off, sums, total, s);
}

extern "C" int ullsam_outline_successors(const int* labels, int H, int W, const unsigned char* mask, const int* off, long E, int connectivity, int* eid,
                                         int* succ, unsigned char* pdir, int* flags, void* stream) {
    OL_FRAME_CHECK("outline_successors");
    OL_EDGES_CHECK("outline_successors");
    ULLSAM_CHECK(connectivity == 4 || connectivity == 8, "outline_successors: connectivity is 4 or 8");
    if (E == 0) return 0;
    outline_successors_kernel<<<mz_blocks((long)H * W, OL_BLOCK), OL_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(labels, H, W, mask, off, E, connectivity, eid, succ,
                                                                                                           pdir, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ws i32 [2, E, 4]: the state (mn, pos, jump, 0) twice; rounds = ceil(log2 E)
extern "C" int ullsam_outline_rank(const int* succ, const int* eid, const unsigned char* pdir, long E, int rounds, int* ws, int* leader, int* rank, int* flags,
                                   void* stream) {
    OL_EDGES_CHECK("outline_rank");
    ULLSAM_CHECK(rounds >= 0 && rounds <= 31 && (1L << rounds) >= E && (rounds == 0 || (1L << (rounds - 1)) < E), "outline_rank: rounds must be ceil(log2 E)");
    ULLSAM_CHECK(((uintptr_t)ws & 15) == 0, "outline_rank: ws must be aligned to 16 bytes");
    if (E == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int4* a = reinterpret_cast<int4*>(ws);
    int4* b = a + E;
    outline_rank_init_kernel<<<mz_blocks(E, OL_BLOCK), OL_BLOCK, 0, s>>>(succ, E, a, flags);
    ULLSAM_LAUNCH_CHECK();
    for (int r = 0; r < rounds; ++r) {
        outline_rank_round_kernel<<<mz_blocks(E, OL_BLOCK), OL_BLOCK, 0, s>>>(E, 1 << r, a, b);
        ULLSAM_LAUNCH_CHECK();
        int4* t = a;
        a = b;
        b = t;
    }
    outline_rank_finish_kernel<<<mz_blocks(E, OL_BLOCK), OL_BLOCK, 0, s>>>(succ, eid, pdir, E, a, leader, rank, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_outline_collect(const int* labels, long n, const int* eid, const int* leader, long E, unsigned long long* list, long room, int* flags,
                                      void* stream) {
    OL_EDGES_CHECK("outline_collect");
    ULLSAM_CHECK(n >= 1 && n < OL_MAX_PIXELS && room >= 0, "outline_collect: need 1 <= n < 2^29 and room >= 0");
    if (E == 0) return 0;
    outline_collect_kernel<<<mz_blocks(E, OL_BLOCK), OL_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(labels, n, eid, leader, E, reinterpret_cast<mz_u64*>(list), room,
                                                                                                flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_outline_loops(const int* eid, const int* leader, const int* loop_of, long E, long L, int W, int* edges, long long* area2, int* flags,
                                    void* stream) {
    OL_EDGES_CHECK("outline_loops");
    ULLSAM_CHECK(L >= 0 && L <= E && W >= 1, "outline_loops: need 0 <= L <= E and W >= 1");
    if (E == 0 || L == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(edges, 0, (size_t)L * 4, s) != hipSuccess || hipMemsetAsync(area2, 0, (size_t)L * 8, s) != hipSuccess) {
        ullsam_set_error("outline_loops: memset failed");
        return -2;
    }
    outline_loops_kernel<<<mz_blocks((E + OL_RUN - 1) / OL_RUN, OL_BLOCK), OL_BLOCK, 0, s>>>(eid, leader, loop_of, E, L, W, edges, area2, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_outline_order(const int* eid, const unsigned char* pdir, const int* leader, const int* rank, const int* loop_of, const int* estart, long E,
                                    long L, int* reid, unsigned char* corner, int* flags, void* stream) {
    OL_EDGES_CHECK("outline_order");
    ULLSAM_CHECK(L >= 0 && L <= E, "outline_order: need 0 <= L <= E");
    if (E == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(corner, 0, (size_t)E, s) != hipSuccess) {   // (a slot a hand-made table leaves out holds no corner)
        ullsam_set_error("outline_order: memset failed");
        return -2;
    }
    outline_order_kernel<<<mz_blocks(E, OL_BLOCK), OL_BLOCK, 0, s>>>(eid, pdir, leader, rank, loop_of, estart, E, L, reid, corner, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_outline_vertices(const int* reid, const unsigned char* corner, const int* coff, long E, int W, long N, int* vertices, void* stream) {
    OL_EDGES_CHECK("outline_vertices");
    ULLSAM_CHECK(N >= 0 && N <= E && W >= 1, "outline_vertices: need 0 <= N <= E and W >= 1");
    if (E == 0 || N == 0) return 0;
    outline_vertices_kernel<<<mz_blocks(E, OL_BLOCK), OL_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(reid, corner, coff, E, W, N, vertices);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_outline_parents(const int* labels, int H, int W, const unsigned char* mask, const int* off, const int* eid, const int* leader,
                                      const int* loop_of, const int* lead, const long long* area2, long E, long L, int* parent, int* flags, void* stream) {
    OL_FRAME_CHECK("outline_parents");
    OL_EDGES_CHECK("outline_parents");
    ULLSAM_CHECK(L >= 0 && L <= E, "outline_parents: need 0 <= L <= E");
    if (L == 0) return 0;
    outline_parents_kernel<<<mz_blocks(L, OL_BLOCK), OL_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(labels, H, W, mask, off, eid, leader, loop_of, lead, area2, E, L,
                                                                                                parent, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
