// Simplified outlines of an instance label image: Douglas-Peucker on label_outlines' loops with exact integer arithmetic and a rule that does not
// depend on the direction of travel, so the border two instances share comes out as the same vertices in both rings (host form and definition:
// utils/simplify.py; DESIGN.md "7b, continued (simplifying)").  Integer work only -- ordinary vector stores and integer atomics (max, min, sums,
// none of which depends on the order of arrival) -- so every output is a function of the labels alone.
//
// The input is outline_order's rank-ordered copy of the edges (reid, corner: loop after loop, every loop in travel order from its leader) and
// estart, the first slot of every loop.  A lattice point is (X, Y) in 0..W x 0..H, packed as Y << 16 | X (sides are at most 32767).
//   flags       cand[i]: bit 0 = the tail of slot i is a candidate (a corner, or a fixed point), bit 1 = it is a fixed point: at least three of the
//               four pixel sides that meet there separate different values (the frame's outside is 0).
//   candidates  the compaction (coff = outline_scan of cand): cxy, cloop (a search in estart), kept = fixed; nfixed[loop] counts the fixed ones.
//   anchors     a loop without a fixed point: the candidate of smallest (y, x) by an atomic min of yx << 32 | index; then the one of largest squared
//               distance from it, ties to the smallest (y, x), by an atomic max of d2 << 32 | ~yx; both are marked kept.
//   segments    klist = the kept candidates in order (koff = outline_scan of kept); every other candidate takes pa / pb: the kept candidates before
//               and after it, cyclic in its loop.  A segment is named by its pa.
//   rounds      pass 1: num of every open candidate to an atomic max in segmax[pa] (held as the minimum of ~num); pass 2: those that hold the maximum and pass the threshold send
//               yx << 32 | index to an atomic min in segwin[pa]; pass 3: the winner is marked kept and counted, the others of its segment move pa
//               or pb to it; a segment without a winner is closed for good (pa = -1).  Both tables are reset before every round.  The host asks
//               for a block of rounds at a time; the rounds after one that kept nothing return at once.
//   rings       the kept candidates in order are the vertices; nvert and area2 (the shoelace sum over the ring) per loop.
// flags i32 [4]: [0] = an index that left its table (skipped; nothing is indexed with it); the others are free.
#include "label_common.h"
#include <stdint.h>

#define SM_BLOCK 256
#define SM_NONE 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ int sm_x(int yx) { return yx & 0xFFFF; }
__device__ __forceinline__ int sm_y(int yx) { return yx >> 16; }
__device__ __forceinline__ long long sm_d2(int p, int q) {
    const long long dx = sm_x(p) - sm_x(q), dy = sm_y(p) - sm_y(q);
    return dx * dx + dy * dy;
}

// ---- flags and candidates -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sm_val(const int* __restrict__ labels, int H, int W, int x, int y) {
    return x >= 0 && x < W && y >= 0 && y < H ? labels[(long)y * W + x] : 0;
}
// the tail of edge id as Y << 16 | X, or -1 (a hand-made table)
__device__ __forceinline__ int sm_tail(int id, int H, int W) {
    const int s = id & 3;
    const long p = (long)(id >> 2);
    if (id < 0 || p >= (long)H * W) return -1;
    const int X = (int)(p % W) + (s == 1 || s == 2), Y = (int)(p / W) + (s == 2 || s == 3);
    return Y << 16 | X;
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_flags_kernel(const int* __restrict__ labels, int H, int W, const int* __restrict__ reid,
                                                                  const unsigned char* __restrict__ corner, long E, unsigned char* __restrict__ cand,
                                                                  int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= E) return;
    const int t = sm_tail(reid[i], H, W);
    if (t < 0) {
        mz_store(flags + 0, 1);
        cand[i] = 0;
        return;
    }
    const int X = sm_x(t), Y = sm_y(t);
    const int a = sm_val(labels, H, W, X - 1, Y - 1), b = sm_val(labels, H, W, X, Y - 1), c = sm_val(labels, H, W, X - 1, Y),
              d = sm_val(labels, H, W, X, Y);
    const bool fixed = (a != b) + (c != d) + (a != c) + (b != d) >= 3;
    cand[i] = (unsigned char)(fixed ? 3 : corner[i] ? 1 : 0);
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_candidates_kernel(const int* __restrict__ reid, const unsigned char* __restrict__ cand,
                                                                       const int* __restrict__ coff, const int* __restrict__ estart, long E, long L, long C,
                                                                       int H, int W, int* __restrict__ cxy, int* __restrict__ cloop,
                                                                       unsigned char* __restrict__ kept, int* __restrict__ nfixed, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= E) return;
    const unsigned v = cand[i];
    if (v == 0) return;
    const long at = coff[i];
    const int t = sm_tail(reid[i], H, W);
    long lo = 0, hi = L;                                  // the last loop whose first slot is at or before i
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if ((long)estart[mid] <= i) lo = mid;
        else hi = mid;
    }
    if (!mz_in(at, C) || t < 0 || (long)estart[lo] > i) {
        mz_store(flags + 0, 1);
        return;
    }
    cxy[at] = t;
    cloop[at] = (int)lo;
    kept[at] = (unsigned char)(v >> 1 & 1u);
    if (v & 2u) mz_add(nfixed + lo, 1);
}

// ---- anchors --------------------------------------------------------------------------------------------------------------------------------
// the loop of candidate i when it has no fixed point, else -1
__device__ __forceinline__ int sm_free_loop(const int* __restrict__ cloop, const int* __restrict__ nfixed, long L, long i, int* __restrict__ flags) {
    const int l = cloop[i];
    if (!mz_in(l, L)) {
        mz_store(flags + 0, 1);
        return -1;
    }
    return nfixed[l] == 0 ? l : -1;
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_anchor_first_kernel(const int* __restrict__ cxy, const int* __restrict__ cloop,
                                                                         const int* __restrict__ nfixed, long C, long L, mz_u64* __restrict__ amin,
                                                                         int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C) return;
    const int l = sm_free_loop(cloop, nfixed, L, i, flags);
    if (l >= 0) mz_send_min(amin + l, (mz_u64)(unsigned)cxy[i] << 32 | (mz_u64)(unsigned)i);
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_anchor_far_kernel(const int* __restrict__ cxy, const int* __restrict__ cloop,
                                                                       const int* __restrict__ nfixed, long C, long L, const mz_u64* __restrict__ amin,
                                                                       mz_u64* __restrict__ amax, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C) return;
    const int l = sm_free_loop(cloop, nfixed, L, i, flags);
    if (l < 0) return;
    const int first = (int)(amin[l] >> 32);               // (this loop's candidates all went through the first pass)
    mz_send_max(amax + l, (mz_u64)sm_d2(cxy[i], first) << 32 | (mz_u64)(0xFFFFFFFFu - (unsigned)cxy[i]));
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_anchor_mark_kernel(const int* __restrict__ cxy, const int* __restrict__ cloop,
                                                                        const int* __restrict__ nfixed, long C, long L, const mz_u64* __restrict__ amin,
                                                                        const mz_u64* __restrict__ amax, unsigned char* __restrict__ kept,
                                                                        int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C) return;
    const int l = sm_free_loop(cloop, nfixed, L, i, flags);
    if (l < 0) return;
    const unsigned yx = (unsigned)cxy[i];                 // (such a loop visits a lattice point once: the point names the candidate)
    if (yx == (unsigned)(amin[l] >> 32) || yx == 0xFFFFFFFFu - (unsigned)(amax[l] & 0xFFFFFFFFull)) kept[i] = 1;
}

// ---- segments -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_BLOCK) void simplify_list_kernel(const unsigned char* __restrict__ kept, const int* __restrict__ koff, long C,
                                                                 const int* __restrict__ total, int* __restrict__ klist, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C || !kept[i]) return;
    const long at = koff[i], n = total[0];
    if (mz_in(at, n) && n <= C) klist[at] = (int)i;
    else mz_store(flags + 0, 1);
}
// the kept candidates of loop l are klist[k0 : k1]; false when the tables do not fit (a hand-made table)
__device__ __forceinline__ bool sm_span(const int* __restrict__ cstart, const int* __restrict__ koff, long C, long L, long n, int l, long& k0, long& k1) {
    if (!mz_in(l, L)) return false;
    const long cs = cstart[l], ce = cstart[l + 1];
    if (!(cs >= 0 && cs < ce && ce <= C)) return false;
    k0 = koff[cs];
    k1 = ce < C ? (long)koff[ce] : n;
    return k0 >= 0 && k0 < k1 && k1 <= n && n <= C;
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_segments_kernel(const unsigned char* __restrict__ kept, const int* __restrict__ koff,
                                                                     const int* __restrict__ cloop, const int* __restrict__ cstart, long C, long L,
                                                                     const int* __restrict__ total, const int* __restrict__ klist, int* __restrict__ pa,
                                                                     int* __restrict__ pb, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C) return;
    int a = -1, b = -1;
    if (!kept[i]) {
        long k0, k1;
        const long n = total[0], r = koff[i];
        if (sm_span(cstart, koff, C, L, n, cloop[i], k0, k1) && r >= k0 && r <= k1) {
            a = klist[r > k0 ? r - 1 : k1 - 1];
            b = klist[r < k1 ? r : k0];
            if (!mz_in(a, C) || !mz_in(b, C)) a = b = -1;
        }
        if (a < 0) mz_store(flags + 0, 1);
    }
    pa[i] = a;
    pb[i] = b;
}

// ---- the rounds -----------------------------------------------------------------------------------------------------------------------------
// a round of a block whose predecessor kept nothing has nothing to do: every segment is closed (prev = that round's counter, null for the first)
__device__ __forceinline__ bool sm_idle(const int* __restrict__ prev) { return prev != nullptr && *prev == 0; }
// num of candidate p against the chord a -> b (DESIGN: every value stays below 2^62)
__device__ __forceinline__ mz_u64 sm_num(int p, int a, int b) {
    const long long bx = sm_x(b) - sm_x(a), by = sm_y(b) - sm_y(a), px = sm_x(p) - sm_x(a), py = sm_y(p) - sm_y(a);
    const long long len = bx * bx + by * by, t = px * bx + py * by;
    if (len == 0) return (mz_u64)(px * px + py * py);
    if (t <= 0) return (mz_u64)((px * px + py * py) * len);
    if (t >= len) return (mz_u64)(sm_d2(p, b) * len);
    const long long cr = bx * py - by * px;
    return (mz_u64)(cr * cr);
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_round_max_kernel(const int* __restrict__ cxy, const int* __restrict__ pa, const int* __restrict__ pb,
                                                                      long C, const int* __restrict__ prev, mz_u64* __restrict__ cnum,
                                                                      mz_u64* __restrict__ segmax) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C || sm_idle(prev)) return;
    const int a = pa[i], b = pb[i];
    if (!mz_in(a, C) || !mz_in(b, C)) return;             // closed, kept, or never opened
    const mz_u64 num = sm_num(cxy[i], cxy[a], cxy[b]);
    cnum[i] = num;
    mz_send_min(segmax + a, ~num);                             // (the complement under a minimum: both tables start as all ones, one memset)
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_round_win_kernel(const int* __restrict__ cxy, const int* __restrict__ pa, const int* __restrict__ pb,
                                                                      long C, long long T2, const int* __restrict__ prev,
                                                                      const mz_u64* __restrict__ cnum, const mz_u64* __restrict__ segmax,
                                                                      mz_u64* __restrict__ segwin) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C || sm_idle(prev)) return;
    const int a = pa[i], b = pb[i];
    if (!mz_in(a, C) || !mz_in(b, C)) return;
    const mz_u64 num = cnum[i];
    if (~num != segmax[a]) return;
    const long long len = sm_d2(cxy[a], cxy[b]);
    const mz_u64 bound = ((mz_u64)T2 * (mz_u64)(len == 0 ? 1 : len)) >> 16;   // T2 < 2^32, len < 2^31
    if (num > bound) mz_send_min(segwin + a, (mz_u64)(unsigned)cxy[i] << 32 | (mz_u64)(unsigned)i);
}
__global__ __launch_bounds__(SM_BLOCK) void simplify_round_mark_kernel(const int* __restrict__ cloop, const int* __restrict__ cstart, long C, long L,
                                                                       const int* __restrict__ prev, const mz_u64* __restrict__ segwin,
                                                                       int* __restrict__ pa, int* __restrict__ pb, unsigned char* __restrict__ kept,
                                                                       int* __restrict__ count, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    bool won = false;
    if (i < C && !sm_idle(prev)) {
        const int a = pa[i];
        if (mz_in(a, C) && mz_in(pb[i], C)) {
            const mz_u64 w = segwin[a];
            const long wi = (long)(w & 0xFFFFFFFFull);
            const int l = cloop[i];
            if (w == SM_NONE) pa[i] = -1;                 // no candidate of the segment passes: it stays as it is for good
            else if (wi == i) {
                kept[i] = 1;
                pa[i] = -1;
                won = true;
            } else if (!mz_in(wi, C) || !mz_in(l, L)) {
                mz_store(flags + 0, 1);
                pa[i] = -1;
            } else {
                const long cs = cstart[l], n = (long)cstart[l + 1] - cs;
                if (n < 1 || i - cs >= n || i < cs || a < cs || a - cs >= n || wi < cs || wi - cs >= n) {
                    mz_store(flags + 0, 1);
                    pa[i] = -1;
                } else if ((i - a + n) % n < (wi - a + n) % n) pb[i] = (int)wi;   // between a and the winner, in travel order
                else pa[i] = (int)wi;
            }
        }
    }
    const mz_u64 m = __ballot(won);
    if ((threadIdx.x & 63) == 0 && m) mz_add(count, __builtin_popcountll(m));
}

// ---- rings ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_BLOCK) void simplify_rings_kernel(const int* __restrict__ cxy, const int* __restrict__ cloop, const unsigned char* __restrict__ kept,
                                                                  const int* __restrict__ voff, const int* __restrict__ cstart, long C, long L, long N,
                                                                  const int* __restrict__ total, const int* __restrict__ klist, int* __restrict__ vertices,
                                                                  int* __restrict__ nvert, long long* __restrict__ area2, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i >= C || !kept[i]) return;
    long k0, k1;
    const long n = total[0], r = voff[i];
    const int l = cloop[i];
    if (n != N || !sm_span(cstart, voff, C, L, n, l, k0, k1) || r < k0 || r >= k1) {   // (r < k1 <= n = N: the row exists)
        mz_store(flags + 0, 1);
        return;
    }
    const int j = klist[r + 1 < k1 ? r + 1 : k0];
    if (!mz_in(j, C)) {
        mz_store(flags + 0, 1);
        return;
    }
    const int p = cxy[i], q = cxy[j];
    vertices[2 * r + 0] = sm_x(p);
    vertices[2 * r + 1] = sm_y(p);
    mz_add(nvert + l, 1);
    mz_add64(area2 + l, (mz_u64)((long long)sm_x(p) * sm_y(q) - (long long)sm_x(q) * sm_y(p)));
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define SM_MAX_SIDE 32767
#define SM_MAX_PIXELS (1L << 29)
#define SM_FRAME_CHECK(what) \
    ULLSAM_CHECK(H >= 1 && W >= 1 && H <= SM_MAX_SIDE && W <= SM_MAX_SIDE && (long)H * W < SM_MAX_PIXELS, what ": need 1 <= H, W <= 32767 and H * W < 2^29")
#define SM_TABLE_CHECK(what) ULLSAM_CHECK(C >= 0 && C < 4 * SM_MAX_PIXELS && L >= 0 && L <= C, what ": need 0 <= L <= C < 2^31")
#define SM_MEMSET(ptr, v, bytes, what)                              \
    do {                                                            \
        if (hipMemsetAsync(ptr, v, bytes, s) != hipSuccess) {       \
            ullsam_set_error(what ": memset failed");               \
            return -2;                                              \
        }                                                           \
    } while (0)

extern "C" int ullsam_simplify_flags(const int* labels, int H, int W, const int* reid, const unsigned char* corner, long E, unsigned char* cand, int* flags,
                                     void* stream) {
    SM_FRAME_CHECK("simplify_flags");
    ULLSAM_CHECK(E >= 0 && E < 4 * SM_MAX_PIXELS, "simplify_flags: need 0 <= E < 2^31");
    if (E == 0) return 0;
    simplify_flags_kernel<<<mz_blocks(E, SM_BLOCK), SM_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(labels, H, W, reid, corner, E, cand, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_simplify_candidates(const int* reid, const unsigned char* cand, const int* coff, const int* estart, long E, long L, long C, int H, int W,
                                          int* cxy, int* cloop, unsigned char* kept, int* nfixed, int* flags, void* stream) {
    SM_FRAME_CHECK("simplify_candidates");
    SM_TABLE_CHECK("simplify_candidates");
    ULLSAM_CHECK(E >= C && E < 4 * SM_MAX_PIXELS, "simplify_candidates: need C <= E < 2^31");
    if (C == 0 || L == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SM_MEMSET(nfixed, 0, (size_t)L * 4, "simplify_candidates");
    SM_MEMSET(kept, 0, (size_t)C, "simplify_candidates");
    SM_MEMSET(cloop, 0xFF, (size_t)C * 4, "simplify_candidates");   // (a slot a hand-made table leaves out belongs to no loop)
    SM_MEMSET(cxy, 0, (size_t)C * 4, "simplify_candidates");
    simplify_candidates_kernel<<<mz_blocks(E, SM_BLOCK), SM_BLOCK, 0, s>>>(reid, cand, coff, estart, E, L, C, H, W, cxy, cloop, kept, nfixed, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ws u64 [2, L] is scratch
extern "C" int ullsam_simplify_anchors(const int* cxy, const int* cloop, const int* nfixed, long C, long L, unsigned long long* ws, unsigned char* kept,
                                       int* flags, void* stream) {
    SM_TABLE_CHECK("simplify_anchors");
    if (C == 0 || L == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    mz_u64* amin = reinterpret_cast<mz_u64*>(ws);
    mz_u64* amax = amin + L;
    SM_MEMSET(amin, 0xFF, (size_t)L * 8, "simplify_anchors");
    SM_MEMSET(amax, 0, (size_t)L * 8, "simplify_anchors");
    simplify_anchor_first_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cxy, cloop, nfixed, C, L, amin, flags);
    ULLSAM_LAUNCH_CHECK();
    simplify_anchor_far_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cxy, cloop, nfixed, C, L, amin, amax, flags);
    ULLSAM_LAUNCH_CHECK();
    simplify_anchor_mark_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cxy, cloop, nfixed, C, L, amin, amax, kept, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// koff = outline_scan of kept and total its sum, both on the device; klist i32 [C] is scratch
extern "C" int ullsam_simplify_segments(const unsigned char* kept, const int* koff, const int* total, const int* cloop, const int* cstart, long C, long L,
                                        int* klist, int* pa, int* pb, int* flags, void* stream) {
    SM_TABLE_CHECK("simplify_segments");
    if (C == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SM_MEMSET(klist, 0xFF, (size_t)C * 4, "simplify_segments");
    simplify_list_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(kept, koff, C, total, klist, flags);
    ULLSAM_LAUNCH_CHECK();
    simplify_segments_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(kept, koff, cloop, cstart, C, L, total, klist, pa, pb, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ws u64 [3, C] is scratch (num, segmax, segwin); counts i32 [rounds] (zeroed here)[r] = the candidates round r kept
extern "C" int ullsam_simplify_rounds(const int* cxy, const int* cloop, const int* cstart, long C, long L, long long T2, int rounds, unsigned long long* ws,
                                      int* pa, int* pb, unsigned char* kept, int* counts, int* flags, void* stream) {
    SM_TABLE_CHECK("simplify_rounds");
    ULLSAM_CHECK(T2 >= 0 && T2 <= 65280LL * 65280LL && rounds >= 1 && rounds <= 1024, "simplify_rounds: need 0 <= T2 <= (255 * 256)^2 and 1 <= rounds <= 1024");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SM_MEMSET(counts, 0, (size_t)rounds * 4, "simplify_rounds");
    if (C == 0) return 0;
    mz_u64* cnum = reinterpret_cast<mz_u64*>(ws);
    mz_u64* segmax = cnum + C;
    mz_u64* segwin = segmax + C;
    for (int r = 0; r < rounds; ++r) {
        const int* prev = r ? counts + r - 1 : nullptr;
        SM_MEMSET(segmax, 0xFF, (size_t)C * 16, "simplify_rounds");   // segmax and segwin, one after the other
        simplify_round_max_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cxy, pa, pb, C, prev, cnum, segmax);
        ULLSAM_LAUNCH_CHECK();
        simplify_round_win_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cxy, pa, pb, C, T2, prev, cnum, segmax, segwin);
        ULLSAM_LAUNCH_CHECK();
        simplify_round_mark_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cloop, cstart, C, L, prev, segwin, pa, pb, kept, counts + r, flags);
        ULLSAM_LAUNCH_CHECK();
    }
    return 0;
}

// voff = outline_scan of kept and total = N its sum, both on the device; vertices i32 [N, 2]; nvert i32 [L] and area2 i64 [L] are zeroed here
extern "C" int ullsam_simplify_rings(const int* cxy, const int* cloop, const unsigned char* kept, const int* voff, const int* total, const int* cstart, long C,
                                     long L, long N, int* klist, int* vertices, int* nvert, long long* area2, int* flags, void* stream) {
    SM_TABLE_CHECK("simplify_rings");
    ULLSAM_CHECK(N >= 0 && N <= C, "simplify_rings: need 0 <= N <= C");
    if (L == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SM_MEMSET(nvert, 0, (size_t)L * 4, "simplify_rings");
    SM_MEMSET(area2, 0, (size_t)L * 8, "simplify_rings");
    if (C == 0 || N == 0) return 0;
    SM_MEMSET(klist, 0xFF, (size_t)C * 4, "simplify_rings");
    simplify_list_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(kept, voff, C, total, klist, flags);
    ULLSAM_LAUNCH_CHECK();
    simplify_rings_kernel<<<mz_blocks(C, SM_BLOCK), SM_BLOCK, 0, s>>>(cxy, cloop, kept, voff, cstart, C, L, N, total, klist, vertices, nvert, area2, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
