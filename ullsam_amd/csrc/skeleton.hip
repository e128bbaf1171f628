// Skeletons of an instance label image: Guo and Hall's two-sub-iteration parallel thinning of every instance at once, and the end points, junctions,
// links and local widths of the result (host form and definition: utils/skeleton.py; DESIGN.md "7b, continued (skeletons)").  Integer work only --
// no float anywhere, ordinary vector stores, integer atomics -- and a sub-iteration is a function of the state at its start, so every output is a
// function of the labels alone: bit-exact with the numpy definition and identical from run to run.
//
// The image holds a pixel's label while it stands and 0 once it is deleted.  A neighbour of p is ON when it lies in the frame and holds p's label;
// the code of p has bit i for N, NE, E, SE, S, SW, W, NW (y grows downwards).  p is deleted in a sub-iteration of parity q iff table q holds its
// code; a table is 256 bits = eight 32-bit words (bit code & 31 of word code >> 5), built here from the rule at compile time and handed to the
// kernels by value (scalar registers: the lookup is eight selects and a shift, no memory).
//   step     one sub-iteration per launch: one lane per pixel reads src and its 8 neighbours and writes dst (the caller ping-pongs the two).
//   lds      SK_S sub-iterations per launch: a workgroup stages its SK_CW x SK_CH core and a halo of SK_S pixels in LDS and runs the sub-iterations
//            there, ping-ponging two LDS images.  What lies outside the staged tile is unknown, so after j sub-iterations only the pixels at least j
//            from the tile's rim are exact (a pixel's next state needs its 8 neighbours' current ones): sub-iteration j computes the pixels at
//            least j + 1 from the rim, and after SK_S of them the core is exact and only the core is written.  The frame's outside is 0 for ever,
//            which is exact.  A tile without a labelled pixel writes its zeros and leaves.
//   counters a lane that deletes adds to the counter of its sub-iteration: one atomic per wave in `step`; in `lds` an LDS counter per sub-iteration,
//            core pixels only (every pixel is in one core), then one atomic per workgroup and sub-iteration.
//   nodes    one lane per pixel: its links (4-adjacent pixels of its label; diagonal ones when neither pixel 4-adjacent to both holds the label),
//            its degree, the node class, and its contributions straight to the global tables with integer atomics (a skeleton is sparse).
// flags i32 [4]: [0] = a label below 0 (thinning) or outside 0..K (nodes): it reads as background, nothing is indexed with it; [1] = a pixel was
// deleted in a sub-iteration whose index is not below `limit`.
#include "label_common.h"
#include <stdint.h>

#define SK_TW 64                      // step / nodes: a workgroup covers SK_TW x SK_TH pixels
#define SK_TH 4
#define SK_CW 64                      // lds: the core, the sub-iterations of a launch = the depth of the halo, the staged tile
#define SK_CH 32
#define SK_S 8
#define SK_LW (SK_CW + 2 * SK_S)
#define SK_LH (SK_CH + 2 * SK_S)
#define SK_N (SK_LW * SK_LH)
#define SK_PER ((SK_N + 255) / 256)

struct SkTable { unsigned w[8]; };

constexpr bool sk_deletable(int code, int parity) {
    const int p2 = code & 1, p3 = (code >> 1) & 1, p4 = (code >> 2) & 1, p5 = (code >> 3) & 1, p6 = (code >> 4) & 1, p7 = (code >> 5) & 1,
              p8 = (code >> 6) & 1, p9 = (code >> 7) & 1;
    const int c = ((1 - p2) & (p3 | p4)) + ((1 - p4) & (p5 | p6)) + ((1 - p6) & (p7 | p8)) + ((1 - p8) & (p9 | p2));
    const int n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8), n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9);
    const int n = n1 < n2 ? n1 : n2;
    const int m = parity == 0 ? ((p2 | p3 | (1 - p5)) & p4) : ((p6 | p7 | (1 - p9)) & p8);
    return c == 1 && n >= 2 && n <= 3 && m == 0;
}
constexpr SkTable sk_table(int parity) {
    SkTable t{};
    for (int code = 0; code < 256; ++code)
        if (sk_deletable(code, parity)) t.w[code >> 5] |= 1u << (code & 31);
    return t;
}
static constexpr SkTable SK_TABLE[2] = {sk_table(0), sk_table(1)};

__device__ __forceinline__ bool sk_hit(const SkTable& t, int code) {
    unsigned w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w = (code >> 5) == k ? t.w[k] : w;
    return (w >> (code & 31)) & 1u;
}

// ---- one sub-iteration from global memory -----------------------------------------------------------------------------------------------------
// grid (ceil(W / SK_TW), ceil(H / SK_TH)), block 256
__global__ __launch_bounds__(256) void skel_step_kernel(const int* __restrict__ src, int* __restrict__ dst, int H, int W, SkTable tab, int over,
                                                        int* __restrict__ count, int* __restrict__ flags) {
    const int x = blockIdx.x * SK_TW + threadIdx.x % SK_TW, y = blockIdx.y * SK_TH + threadIdx.x / SK_TW;
    bool del = false;
    if (x < W && y < H) {
        const int p = y * W + x;                          // H * W < 2^30
        int l = src[p];
        if (l < 0) {
            mz_store(flags + 0, 1);
            l = 0;
        }
        if (l > 0) {
            const bool n = y > 0, s = y + 1 < H, w = x > 0, e = x + 1 < W;
            int code = 0;
            code |= (n && src[p - W] == l) ? 1 : 0;
            code |= (n && e && src[p - W + 1] == l) ? 2 : 0;
            code |= (e && src[p + 1] == l) ? 4 : 0;
            code |= (s && e && src[p + W + 1] == l) ? 8 : 0;
            code |= (s && src[p + W] == l) ? 16 : 0;
            code |= (s && w && src[p + W - 1] == l) ? 32 : 0;
            code |= (w && src[p - 1] == l) ? 64 : 0;
            code |= (n && w && src[p - W - 1] == l) ? 128 : 0;
            del = sk_hit(tab, code);
        }
        dst[p] = del ? 0 : l;
    }
    const mz_u64 m = __ballot(del);
    if (m != 0 && (int)(threadIdx.x & 63) == __builtin_ctzll(m)) {
        mz_add(count, __builtin_popcountll(m));
        if (over) mz_store(flags + 1, 1);
    }
}

// ---- SK_S sub-iterations on a tile in LDS -----------------------------------------------------------------------------------------------------
// grid (ceil(W / SK_CW), ceil(H / SK_CH)), block 256; index = the number of the launch's first sub-iteration
__global__ __launch_bounds__(256) void skel_lds_kernel(const int* __restrict__ src, int* __restrict__ dst, int H, int W, SkTable tab0, SkTable tab1,
                                                       int index, int limit, int* __restrict__ counts, int* __restrict__ flags) {
    __shared__ int s_img[2][SK_N];
    __shared__ int s_cnt[SK_S];
    __shared__ int s_any;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SK_CW - SK_S, y0 = blockIdx.y * SK_CH - SK_S;
    if (tid < SK_S) s_cnt[tid] = 0;
    if (tid == 0) s_any = 0;
    __syncthreads();
    int any = 0;
    for (int i = tid; i < SK_N; i += 256) {
        const int gy = y0 + i / SK_LW, gx = x0 + i % SK_LW;
        int v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            v = src[gy * W + gx];
            if (v < 0) {
                mz_store(flags + 0, 1);
                v = 0;
            }
        }
        s_img[0][i] = v;                                  // (0 is no live label: the frame's outside never matches)
        any |= v;
    }
    if (any) s_any = 1;                                   // (every writer stores the same word)
    __syncthreads();
    any = s_any;
    if (any) {
#pragma unroll 1
        for (int j = 0; j < SK_S; ++j) {
            const int* a = s_img[j & 1];
            int* b = s_img[(j + 1) & 1];
            const SkTable tab = ((index + j) & 1) ? tab1 : tab0;
#pragma unroll
            for (int k = 0; k < SK_PER; ++k) {
                const int i = tid + 256 * k;
                const int ly = i / SK_LW, lx = i % SK_LW;
                if (i >= SK_N || min(min(lx, SK_LW - 1 - lx), min(ly, SK_LH - 1 - ly)) <= j) continue;     // at least j + 1 from the rim
                int v = a[i];
                if (v > 0) {
                    int code = 0;
                    code |= (a[i - SK_LW] == v) ? 1 : 0;
                    code |= (a[i - SK_LW + 1] == v) ? 2 : 0;
                    code |= (a[i + 1] == v) ? 4 : 0;
                    code |= (a[i + SK_LW + 1] == v) ? 8 : 0;
                    code |= (a[i + SK_LW] == v) ? 16 : 0;
                    code |= (a[i + SK_LW - 1] == v) ? 32 : 0;
                    code |= (a[i - 1] == v) ? 64 : 0;
                    code |= (a[i - SK_LW - 1] == v) ? 128 : 0;
                    if (sk_hit(tab, code)) {
                        v = 0;
                        if (lx >= SK_S && lx < SK_S + SK_CW && ly >= SK_S && ly < SK_S + SK_CH) atomicAdd(&s_cnt[j], 1);
                    }
                }
                b[i] = v;
            }
            __syncthreads();
        }
    }
    const int* fin = s_img[any ? (SK_S & 1) : 0];
    for (int i = tid; i < SK_CW * SK_CH; i += 256) {
        const int cy = i / SK_CW, cx = i % SK_CW;
        const int gy = y0 + SK_S + cy, gx = x0 + SK_S + cx;
        if (gy < H && gx < W) dst[gy * W + gx] = fin[(cy + SK_S) * SK_LW + cx + SK_S];
    }
    if (tid < SK_S && s_cnt[tid] != 0) {
        mz_add(counts + tid, s_cnt[tid]);
        if (index + tid >= limit) mz_store(flags + 1, 1);
    }
}

// ---- links, degrees, node classes, the per-id tables ------------------------------------------------------------------------------------------
// grid (ceil(W / SK_TW), ceil(H / SK_TH)), block 256.  table i64 [7, K]: pixels, end points, junctions, isolated, orthogonal links, diagonal links,
// the sum of the degrees; any of table, d2, nodes may be NULL.
__global__ __launch_bounds__(256) void skel_nodes_kernel(const int* __restrict__ img, const int* __restrict__ d2, int H, int W, long K,
                                                         long* __restrict__ table, long* __restrict__ d2_sum, int* __restrict__ d2_min,
                                                         int* __restrict__ d2_max, unsigned char* __restrict__ nodes, int* __restrict__ flags) {
    const int x = blockIdx.x * SK_TW + threadIdx.x % SK_TW, y = blockIdx.y * SK_TH + threadIdx.x / SK_TW;
    if (x >= W || y >= H) return;
    const int p = y * W + x;
    const int l = img[p];
    if (!mz_live(l, K)) {
        if (l != 0) mz_store(flags + 0, 1);
        if (nodes) nodes[p] = 0;
        return;
    }
    const bool n = y > 0, s = y + 1 < H, w = x > 0, e = x + 1 < W;
    const bool sN = n && img[p - W] == l, sNE = n && e && img[p - W + 1] == l, sE = e && img[p + 1] == l, sSE = s && e && img[p + W + 1] == l;
    const bool sS = s && img[p + W] == l, sSW = s && w && img[p + W - 1] == l, sW = w && img[p - 1] == l, sNW = n && w && img[p - W - 1] == l;
    const int dNE = sNE && !sN && !sE, dSE = sSE && !sE && !sS, dSW = sSW && !sS && !sW, dNW = sNW && !sW && !sN;
    const int deg = (int)sN + (int)sE + (int)sS + (int)sW + dNE + dSE + dSW + dNW;
    if (nodes) nodes[p] = (unsigned char)(deg == 0 ? 4 : deg >= 3 ? 3 : deg);
    const long r = (long)l - 1;
    if (table) {
        mz_add(table + 0 * K + r, 1);
        if (deg == 1) mz_add(table + 1 * K + r, 1);
        if (deg >= 3) mz_add(table + 2 * K + r, 1);
        if (deg == 0) mz_add(table + 3 * K + r, 1);
        if (sE || sS) mz_add(table + 4 * K + r, (int)sE + (int)sS);                      // every link once: right, down,
        if (dSE || dSW) mz_add(table + 5 * K + r, dSE + dSW);                            // down-right, down-left
        if (deg) mz_add(table + 6 * K + r, deg);
    }
    if (d2) {
        const int v = d2[p];
        mz_add64(d2_sum + r, (mz_u64)(long)v);
        mz_send_min(d2_min + r, v);
        mz_send_max(d2_max + r, v);
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define SK_FRAME_CHECK(what) ULLSAM_CHECK(H >= 1 && H <= 32767 && W >= 1 && W <= 32767, what ": need 1 <= H, W <= 32767")

extern "C" int ullsam_skel_step(const int* src, int* dst, int H, int W, int index, int limit, int* count, int* flags, void* stream) {
    SK_FRAME_CHECK("skel_step");
    ULLSAM_CHECK(index >= 0 && limit >= 0 && src != dst, "skel_step: need index, limit >= 0 and two images");
    const dim3 grid((unsigned)((W + SK_TW - 1) / SK_TW), (unsigned)((H + SK_TH - 1) / SK_TH));
    skel_step_kernel<<<grid, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(src, dst, H, W, SK_TABLE[index & 1], index >= limit ? 1 : 0, count, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_skel_tile(const int* src, int* dst, int H, int W, int index, int limit, int* counts, int* flags, void* stream) {
    SK_FRAME_CHECK("skel_tile");
    ULLSAM_CHECK(index >= 0 && index <= 2147483647 - SK_S && limit >= 0 && src != dst, "skel_tile: need 0 <= index <= 2^31 - 9, limit >= 0 and two images");
    const dim3 grid((unsigned)((W + SK_CW - 1) / SK_CW), (unsigned)((H + SK_CH - 1) / SK_CH));
    skel_lds_kernel<<<grid, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(src, dst, H, W, SK_TABLE[0], SK_TABLE[1], index, limit, counts, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_skel_measure(const int* skeleton, const int* d2, int H, int W, long K, long* table, long* d2_sum, int* d2_min, int* d2_max,
                                   unsigned char* nodes, int* flags, void* stream) {
    SK_FRAME_CHECK("skel_measure");
    ULLSAM_CHECK(K >= 0 && K <= 2147483647L, "skel_measure: need 0 <= K <= 2^31 - 1");
    ULLSAM_CHECK(d2 == nullptr || (d2_sum != nullptr && d2_min != nullptr && d2_max != nullptr), "skel_measure: d2 needs d2_sum, d2_min and d2_max");
    const dim3 grid((unsigned)((W + SK_TW - 1) / SK_TW), (unsigned)((H + SK_TH - 1) / SK_TH));
    skel_nodes_kernel<<<grid, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(skeleton, d2, H, W, K, table, d2_sum, d2_min, d2_max, nodes, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
