// Exact squared Euclidean distance transforms of an instance label image (host form and definition: utils/distance.py; DESIGN.md "7b, continued
// (distances)").  Integer work only -- no float anywhere, ordinary vector stores, integer atomics -- so every output is a function of the labels
// alone: bit-exact with the numpy definition and identical from run to run.
//
// Two transforms, each separated into a column pass and a row pass:
//   inner:   for a pixel p of instance i, the smallest |p - q|^2 over the pixels q with another label (the background is another label; with edge
//            set, so are the pixels just outside the frame).
//   feature: for every pixel, the smallest |p - q|^2 over the labelled pixels q, and the smallest label among the pixels that attain it.
// Column pass.  One lane per column (coalesced along x), one band of DT_BAND rows per wave: the band is walked down and then up.  The state a walk
// carries into its band (the first row of the run of equal labels / the nearest labelled pixel) is found by a search from the band's end towards
// the frame's end, at most H steps.  inner: g(x, y) = the vertical distance to the nearest pixel of the column with another label = the distance to
// the end of the vertical run + 1; feature: g = the vertical distance to the nearest labelled pixel of the column and near = its label, the smaller
// one of the two at equal distance.  g is 16 bits: finite values are <= 32767, DT_INF16 says "none" (an open frame end, an empty column).
// Row pass.  One thread per pixel, grid (ceil(W / 256), H).  inner: only the horizontal run of equal label around p matters -- the first other
// pixel on either side is at vertical distance 0, nothing beyond it can win --
//   D2 = min(g(x)^2, (distance to the first other pixel on either side)^2, min over x' of the run of (x - x')^2 + g(x')^2)
// and the scan outward stops when dx^2 >= best, after at most g(x) steps a side.  feature: the lexicographic minimum of (dx^2 + g(x')^2, near(x'))
// over the row, scanned outward while dx^2 <= best.  Every scan is bounded by maxdx <= W whatever the input.  A call that only asks whether a
// distance exceeds a bound (limit: expand, shrink, background_feature(max_distance2)) never looks farther than isqrt(limit) columns; when that is
// at most DT_HALO the row segment and its halo are staged in LDS and the scan reads LDS only, otherwise it reads global memory (L2).
// Output modes of the row pass: the distance map, the (distance, nearest) pair, the expanded labels, the shrunk labels, the per-instance deepest
// pixel: a 64-bit atomicMax of D2 << 32 | (0xFFFFFFFF - linear index), sent only when a relaxed load says it improves -- the largest D2 and, among
// its pixels, the first in row-major order whatever the order of arrival.
// flags[0] = 1 when a label is negative or above K (the pixel is skipped; no table is indexed with it).
#include "label_common.h"   // the relaxed atomics, isqrt_floor
#include <limits.h>
#include <stdint.h>

#define DT_INF16 0xFFFFu
#define DT_INF 0x7FFFFFFFu
#define DT_BAND 64
#define DT_TILE 256
#define DT_HALO 128
enum { DT_INNER = 0, DT_FEATURE = 1, DT_EXPAND = 2, DT_SHRINK = 3, DT_DEPTH = 4 };

// ---- column pass ----------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), ceil(H / DT_BAND)), block 64
template <bool FEATURE>
__global__ __launch_bounds__(64) void dist_columns_kernel(const int* __restrict__ labels, int H, int W, int edge, long K, unsigned short* __restrict__ g,
                                                         int* __restrict__ near, int* __restrict__ flags) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int y0 = blockIdx.y * DT_BAND, y1 = min(y0 + DT_BAND, H);
    if (y0 >= H) return;
    const int* col = labels + x;
    bool bad = false;
    if (!FEATURE) {
        int l = col[(long)y0 * W], start = y0;           // start: the first row of the vertical run of equal labels that holds y
        while (start > 0 && col[(long)(start - 1) * W] == l) --start;
        for (int y = y0; y < y1; ++y) {
            const int v = col[(long)y * W];
            if (v < 0 || v > K) bad = true;
            if (v != l) { l = v; start = y; }
            const unsigned d = (start == 0 && !edge) ? DT_INF16 : (unsigned)(y - start + 1);
            g[(long)y * W + x] = (unsigned short)(v > 0 ? d : 0u);
        }
        int end = y1 - 1;                                // end: the last row of that run
        l = col[(long)end * W];
        while (end < H - 1 && col[(long)(end + 1) * W] == l) ++end;
        for (int y = y1 - 1; y >= y0; --y) {
            const int v = col[(long)y * W];
            if (v != l) { l = v; end = y; }
            const unsigned d = (end == H - 1 && !edge) ? DT_INF16 : (unsigned)(end - y + 1);
            if (v > 0 && d < g[(long)y * W + x]) g[(long)y * W + x] = (unsigned short)d;
        }
    } else {
        int py = -1, pl = 0;                             // the nearest labelled pixel at or above y
        for (int k = y0 - 1; k >= 0; --k) {
            const int v = col[(long)k * W];
            if (v > 0) { py = k; pl = v; break; }
        }
        for (int y = y0; y < y1; ++y) {
            const int v = col[(long)y * W];
            if (v < 0 || v > K) bad = true;
            if (v > 0) { py = y; pl = v; }
            g[(long)y * W + x] = (unsigned short)(py < 0 ? DT_INF16 : (unsigned)(y - py));
            near[(long)y * W + x] = pl;
        }
        py = -1; pl = 0;                                 // ... and at or below y
        for (int k = y1; k < H; ++k) {
            const int v = col[(long)k * W];
            if (v > 0) { py = k; pl = v; break; }
        }
        for (int y = y1 - 1; y >= y0; --y) {
            const int v = col[(long)y * W];
            if (v > 0) { py = y; pl = v; }
            if (py < 0) continue;
            const unsigned d = (unsigned)(py - y), cur = g[(long)y * W + x];
            if (d < cur || (d == cur && pl < near[(long)y * W + x])) {   // equal distance above and below: the smaller label
                g[(long)y * W + x] = (unsigned short)d;
                near[(long)y * W + x] = pl;
            }
        }
    }
    if (bad) mz_store(flags + 0, 1);
}

// ---- row pass -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned dt_sq16(unsigned g) { return g == DT_INF16 ? DT_INF : g * g; }

// grid (ceil(W / DT_TILE), H), block DT_TILE.  LDS: maxdx <= DT_HALO, every read of the scan falls into the staged segment.
template <bool LDS, int MODE>
__global__ __launch_bounds__(DT_TILE) void dist_rows_kernel(const int* __restrict__ labels, const unsigned short* __restrict__ g, const int* __restrict__ near,
                                                           int H, int W, int edge, unsigned limit, int maxdx, long K, int* __restrict__ out0,
                                                           int* __restrict__ out1, mz_u64* __restrict__ best, int* __restrict__ flags) {
    constexpr bool FEAT = MODE == DT_FEATURE || MODE == DT_EXPAND;
    constexpr int SEG = LDS ? DT_TILE + 2 * DT_HALO : 1;
    __shared__ int s_lab[SEG];                           // inner: the labels; feature: the nearest labels of the column pass
    __shared__ unsigned short s_g[SEG];
    const int y = blockIdx.y, x0 = blockIdx.x * DT_TILE, x = x0 + (int)threadIdx.x;
    const long row = (long)y * W;
    const int* rl = (FEAT ? near : labels) + row;
    const unsigned short* rg = g + row;
    const int lo = max(x0 - DT_HALO, 0);
    if (LDS) {
        const int hi = min(x0 + DT_TILE + DT_HALO, W);
        for (int i = lo + (int)threadIdx.x; i < hi; i += DT_TILE) {
            s_lab[i - lo] = rl[i];
            s_g[i - lo] = rg[i];
        }
        __syncthreads();
    }
    if (x >= W) return;
    auto L = [&](int i) -> int { return LDS ? s_lab[i - lo] : rl[i]; };
    auto G = [&](int i) -> unsigned { return LDS ? s_g[i - lo] : rg[i]; };
    const int l = labels[row + x];
    if (!FEAT) {
        if (MODE != DT_DEPTH) out0[row + x] = 0;
        if (l <= 0 || l > K) {
            if (l != 0) mz_store(flags + 0, 1);
            return;
        }
        unsigned bd = dt_sq16(G(x));
#pragma unroll
        for (int side = -1; side <= 1; side += 2) {
            for (int dx = 1; dx <= maxdx && (unsigned)(dx * dx) < bd; ++dx) {
                const int xx = x + side * dx;
                if (xx < 0 || xx >= W) {                 // the frame's end: another label when edge is set, nothing otherwise
                    if (edge) bd = (unsigned)(dx * dx);
                    break;
                }
                if (L(xx) != l) {                        // the end of the run
                    bd = (unsigned)(dx * dx);
                    break;
                }
                const unsigned gg = G(xx);
                if (gg != DT_INF16) bd = min(bd, (unsigned)(dx * dx) + gg * gg);
            }
        }
        if (MODE == DT_INNER) out0[row + x] = (int)bd;
        if (MODE == DT_SHRINK) out0[row + x] = bd > limit ? l : 0;
        if (MODE == DT_DEPTH) {
            const mz_u64 word = ((mz_u64)bd << 32) | (mz_u64)(0xFFFFFFFFu - (unsigned)(row + x));
            mz_send_max(best + (l - 1), word);
        }
    } else {
        if (l < 0 || l > K) mz_store(flags + 0, 1);
        unsigned bd = dt_sq16(G(x));
        int bl = bd == DT_INF ? 0 : L(x);
        for (int dx = 1; dx <= maxdx && (unsigned)(dx * dx) <= min(bd, limit); ++dx) {
#pragma unroll
            for (int side = -1; side <= 1; side += 2) {
                const int xx = x + side * dx;
                if (xx < 0 || xx >= W) continue;
                const unsigned gg = G(xx);
                if (gg == DT_INF16) continue;
                const unsigned c = (unsigned)(dx * dx) + gg * gg;
                if (c > bd) continue;
                const int ll = L(xx);
                if (c < bd || ll < bl) { bd = c; bl = ll; }
            }
        }
        if (bd > limit) { bd = DT_INF; bl = 0; }
        if (MODE == DT_FEATURE) {
            out0[row + x] = (int)bd;
            out1[row + x] = bl;
        } else {
            out0[row + x] = l > 0 ? l : bl;              // (bd <= limit = r2 wherever bl != 0)
        }
    }
}

// one thread per instance: the winning word becomes (r2, x, y); an absent id keeps its 0 word: r2 = 0, xy = (-1, -1)
__global__ __launch_bounds__(256) void dist_depth_decode_kernel(const mz_u64* __restrict__ best, long K, int W, int* __restrict__ r2, int* __restrict__ xy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    const mz_u64 w = best[i];
    if (w == 0) {
        r2[i] = 0;
        xy[2 * i + 0] = -1;
        xy[2 * i + 1] = -1;
        return;
    }
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(w & 0xffffffffull);
    r2[i] = (int)(w >> 32);
    xy[2 * i + 0] = (int)(idx % (unsigned)W);
    xy[2 * i + 1] = (int)(idx / (unsigned)W);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define DT_FRAME_CHECK(what) \
    ULLSAM_CHECK(H >= 1 && H <= 32767 && W >= 1 && W <= 32767 && K >= 0 && K <= 2147483647L, what ": need 1 <= H, W <= 32767 and 0 <= K <= 2^31 - 1")

extern "C" int ullsam_distance_columns(const int* labels, int H, int W, int feature, int edge, long K, unsigned short* g, int* nearest, int* flags,
                                       void* stream) {
    DT_FRAME_CHECK("distance_columns");
    ULLSAM_CHECK(!feature || nearest != nullptr, "distance_columns: the feature transform writes the nearest labels too");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + DT_BAND - 1) / DT_BAND));
    if (feature) dist_columns_kernel<true><<<grid, 64, 0, s>>>(labels, H, W, edge, K, g, nearest, flags);
    else dist_columns_kernel<false><<<grid, 64, 0, s>>>(labels, H, W, edge, K, g, nearest, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

template <int MODE>
static void dt_rows_launch(bool lds, dim3 grid, hipStream_t s, const int* labels, const unsigned short* g, const int* nearest, int H, int W, int edge,
                           unsigned limit, int maxdx, long K, int* out0, int* out1, mz_u64* best, int* flags) {
    if (lds) dist_rows_kernel<true, MODE><<<grid, DT_TILE, 0, s>>>(labels, g, nearest, H, W, edge, limit, maxdx, K, out0, out1, best, flags);
    else dist_rows_kernel<false, MODE><<<grid, DT_TILE, 0, s>>>(labels, g, nearest, H, W, edge, limit, maxdx, K, out0, out1, best, flags);
}

extern "C" int ullsam_distance_rows(const int* labels, const unsigned short* g, const int* nearest, int H, int W, int mode, int edge, long limit,
                                    int route, long K, int* out0, int* out1, unsigned long long* best, int* flags, void* stream) {
    DT_FRAME_CHECK("distance_rows");
    ULLSAM_CHECK(mode >= DT_INNER && mode <= DT_DEPTH && route >= 0 && route <= 2, "distance_rows: mode in 0..4, route in 0..2");
    ULLSAM_CHECK(limit >= 0 && limit <= 2147483647L, "distance_rows: need 0 <= limit <= 2^31 - 1");
    const bool feat = mode == DT_FEATURE || mode == DT_EXPAND;
    ULLSAM_CHECK(!feat || nearest != nullptr, "distance_rows: the feature modes read the column pass's nearest labels");
    ULLSAM_CHECK((mode != DT_INNER && mode != DT_DEPTH) || limit == 2147483647L, "distance_rows: the distance map and the depths are unbounded (limit = 2^31 - 1)");
    ULLSAM_CHECK(mode == DT_DEPTH ? (best != nullptr || K == 0) : out0 != nullptr, "distance_rows: the mode's output is missing");
    ULLSAM_CHECK(mode != DT_FEATURE || out1 != nullptr, "distance_rows: the feature pair has two outputs");
    const int maxdx = limit == 2147483647L ? W : min(isqrt_floor(limit), W);
    ULLSAM_CHECK(route != 1 || maxdx <= DT_HALO, "distance_rows: the LDS route holds a halo of at most 128 columns");
    const bool lds = route == 1 || (route == 0 && maxdx <= DT_HALO);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mode == DT_DEPTH && !mz_zero(best, (size_t)K * 8, s)) {
        ullsam_set_error("distance_rows: memset failed");
        return -2;
    }
    const dim3 grid((unsigned)((W + DT_TILE - 1) / DT_TILE), (unsigned)H);
    mz_u64* b = reinterpret_cast<mz_u64*>(best);
    const unsigned lim = (unsigned)limit;
    switch (mode) {
        case DT_INNER: dt_rows_launch<DT_INNER>(lds, grid, s, labels, g, nearest, H, W, edge, lim, maxdx, K, out0, out1, b, flags); break;
        case DT_FEATURE: dt_rows_launch<DT_FEATURE>(lds, grid, s, labels, g, nearest, H, W, edge, lim, maxdx, K, out0, out1, b, flags); break;
        case DT_EXPAND: dt_rows_launch<DT_EXPAND>(lds, grid, s, labels, g, nearest, H, W, edge, lim, maxdx, K, out0, out1, b, flags); break;
        case DT_SHRINK: dt_rows_launch<DT_SHRINK>(lds, grid, s, labels, g, nearest, H, W, edge, lim, maxdx, K, out0, out1, b, flags); break;
        default: dt_rows_launch<DT_DEPTH>(lds, grid, s, labels, g, nearest, H, W, edge, lim, maxdx, K, out0, out1, b, flags); break;
    }
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_distance_depth_decode(const unsigned long long* best, long K, int W, int* r2, int* xy, void* stream) {
    ULLSAM_CHECK(K >= 0 && K <= 2147483646L && W >= 1 && W <= 32767, "distance_depth_decode: need 0 <= K <= 2^31 - 2 and 1 <= W <= 32767");
    if (K == 0) return 0;
    dist_depth_decode_kernel<<<mz_blocks(K), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(reinterpret_cast<const mz_u64*>(best), K, W, r2,
                                                                                                           xy);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
