// Exact anisotropic squared Euclidean distance transforms of an instance label volume (host form and definition: utils/distance3d.py; DESIGN.md
// "7b, continued (3-D distances)").  volume i32 [Z, H, W], spacing (sz, sy, sx) positive integers, |p - q|^2 = sz^2 dz^2 + sy^2 dy^2 + sx^2 dx^2.
// Integer work only -- no float anywhere, ordinary vector stores, integer atomics -- so every output is a function of the volume alone: bit-exact
// with the numpy definition and identical from run to run.  csrc/distance.hip is the 2-D form; this file adds one pass and the weights.
//
// Two transforms, each separated into a z pass, a y pass and an x pass:
//   inner:   for a voxel p of object i, the smallest |p - q|^2 over the voxels q with another label (the background is another label; with the
//            edge set for an axis, so are the voxels just outside the volume along it).
//   feature: for every voxel, the smallest |p - q|^2 over the labelled voxels q, and the smallest label among the voxels that attain it.
// z pass.  One lane per (y, x) column of voxels, lanes along x (every step of the walk reads one contiguous row segment), one band of D3_BAND planes
// per wave: the band is walked down and then up.  The state a walk carries into its band is found by a search from the band's end towards the
// volume's end, at most Z steps.  inner: g = the distance in voxels to the end of the run of equal label along z, plus 1; feature: g = the distance
// in voxels to the nearest labelled voxel of the column and near = its label, the smaller one at equal distance.  g is 16 bits, D3_INF16 = none.
// y pass.  One thread per voxel, lanes along x: the scan runs along y at stride W, coalesced across the wave.  inner, within the run [a, b] of
// equal label along y:  h = min(sy^2 (y - a + 1)^2, sy^2 (b + 1 - y)^2, min over y' of the run of sy^2 (y - y')^2 + sz^2 g(y')^2)  -- the first
// other voxel past a run end is at offset 0 in z, nothing beyond it can win; an open end contributes only when the edge counts.  feature: the
// lexicographic minimum of (sy^2 (y - y')^2 + sz^2 g(y')^2, near(y')) over the line.  h is int32, D3_INF = none.
// x pass.  The same along x with h in place of sz^2 g^2, and the output modes of dist_rows_kernel fused: the distance map, the (distance,
// nearest) pair, the expanded labels, the shrunk labels, the per-object deepest voxel: a 64-bit atomicMax of D2 << 32 | (0xFFFFFFFF - linear
// index), sent only when a relaxed load says it improves (Z * H * W <= 2^31 - 1: the index fits).
// Every scan is `for d = 1; d <= maxd` with maxd from the host: n_a - 1 + e_a, or floor(sqrt(limit) / s_a) for a call that only asks whether a
// distance exceeds a bound.  The inner scan stops at w d^2 >= best, the feature scan only at w d^2 > best (a tie with a smaller id must be seen).
// Arithmetic: the host bounds B = sum over the axes of s_a^2 (n_a - 1 + e_a)^2 by 2^31 - 2, so every w d^2 the loops form and every finite g^2,
// h is at most B; a sum of two such terms is formed in unsigned 32 bits (< 2^32) and "none" is skipped before adding.
// flags[0] = 1 when a label is negative or above K (the voxel is skipped; no table is indexed with it).
#include "label_common.h"   // the relaxed atomics, isqrt_floor
#include <limits.h>
#include <stdint.h>

#define D3_INF16 0xFFFFu
#define D3_INF 0x7FFFFFFFu
#define D3_BAND 64
#define D3_TILE 256
enum { D3_INNER = 0, D3_FEATURE = 1, D3_EXPAND = 2, D3_SHRINK = 3, D3_DEPTH = 4 };

// ---- z pass ---------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), H, ceil(Z / D3_BAND)), block 64
template <bool FEATURE>
__global__ __launch_bounds__(64) void dist3_z_kernel(const int* __restrict__ vol, int Z, int H, int W, int edge, long K, unsigned short* __restrict__ g,
                                                    int* __restrict__ near, int* __restrict__ flags) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int z0 = blockIdx.z * D3_BAND, z1 = min(z0 + D3_BAND, Z);
    if (z0 >= Z) return;
    const long plane = (long)H * W, at = (long)y * W + x;
    const int* col = vol + at;
    bool bad = false;
    if (!FEATURE) {
        int l = col[z0 * plane], start = z0;              // start: the first plane of the run of equal labels along z that holds z
        while (start > 0 && col[(start - 1) * plane] == l) --start;
        for (int z = z0; z < z1; ++z) {
            const int v = col[z * plane];
            if (v < 0 || v > K) bad = true;
            if (v != l) { l = v; start = z; }
            const unsigned d = (start == 0 && !edge) ? D3_INF16 : (unsigned)(z - start + 1);
            g[z * plane + at] = (unsigned short)(v > 0 ? d : 0u);
        }
        int end = z1 - 1;                                 // end: the last plane of that run
        l = col[end * plane];
        while (end < Z - 1 && col[(end + 1) * plane] == l) ++end;
        for (int z = z1 - 1; z >= z0; --z) {
            const int v = col[z * plane];
            if (v != l) { l = v; end = z; }
            const unsigned d = (end == Z - 1 && !edge) ? D3_INF16 : (unsigned)(end - z + 1);
            if (v > 0 && d < g[z * plane + at]) g[z * plane + at] = (unsigned short)d;
        }
    } else {
        int pz = -1, pl = 0;                              // the nearest labelled voxel at or before z
        for (int k = z0 - 1; k >= 0; --k) {
            const int v = col[k * plane];
            if (v > 0) { pz = k; pl = v; break; }
        }
        for (int z = z0; z < z1; ++z) {
            const int v = col[z * plane];
            if (v < 0 || v > K) bad = true;
            if (v > 0) { pz = z; pl = v; }
            g[z * plane + at] = (unsigned short)(pz < 0 ? D3_INF16 : (unsigned)(z - pz));
            near[z * plane + at] = pl;
        }
        pz = -1; pl = 0;                                  // ... and at or after z
        for (int k = z1; k < Z; ++k) {
            const int v = col[k * plane];
            if (v > 0) { pz = k; pl = v; break; }
        }
        for (int z = z1 - 1; z >= z0; --z) {
            const int v = col[z * plane];
            if (v > 0) { pz = z; pl = v; }
            if (pz < 0) continue;
            const unsigned d = (unsigned)(pz - z), cur = g[z * plane + at];
            if (d < cur || (d == cur && pl < near[z * plane + at])) {    // equal distance before and after: the smaller label
                g[z * plane + at] = (unsigned short)d;
                near[z * plane + at] = pl;
            }
        }
    }
    if (bad) mz_store(flags + 0, 1);
}

// ---- y pass ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned d3_sq16(unsigned g, unsigned wz) { return g == D3_INF16 ? D3_INF : wz * (g * g); }

// grid (ceil(W / 64), ceil(H / 4), Z), block (64, 4).  wz = sz^2, wy = sy^2.
template <bool FEATURE>
__global__ __launch_bounds__(256) void dist3_y_kernel(const int* __restrict__ vol, const unsigned short* __restrict__ g, const int* __restrict__ near, int H,
                                                     int W, unsigned wz, unsigned wy, int edge, unsigned limit, int maxd, int* __restrict__ h,
                                                     int* __restrict__ hl) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const long base = (long)blockIdx.z * H * W + x;     // the line of this voxel: base + y' * W
    const long p = base + (long)y * W;
    if (!FEATURE) {
        const int l = vol[p];
        if (l <= 0) {
            h[p] = 0;
            return;
        }
        unsigned bd = d3_sq16(g[p], wz);
#pragma unroll
        for (int side = -1; side <= 1; side += 2) {
            for (int d = 1; d <= maxd; ++d) {
                const unsigned wd = wy * (unsigned)(d * d);
                if (wd >= bd) break;
                const int yy = y + side * d;
                if (yy < 0 || yy >= H) {                  // the volume's end: another label when the edge counts, nothing otherwise
                    if (edge) bd = wd;
                    break;
                }
                const long q = base + (long)yy * W;
                if (vol[q] != l) {                        // the end of the run
                    bd = wd;
                    break;
                }
                const unsigned gg = g[q];
                if (gg != D3_INF16) bd = min(bd, wd + wz * (gg * gg));
            }
        }
        h[p] = (int)bd;
    } else {
        unsigned bd = d3_sq16(g[p], wz);
        int bl = bd == D3_INF ? 0 : near[p];
        for (int d = 1; d <= maxd; ++d) {
            const unsigned wd = wy * (unsigned)(d * d);
            if (wd > min(bd, limit)) break;
#pragma unroll
            for (int side = -1; side <= 1; side += 2) {
                const int yy = y + side * d;
                if (yy < 0 || yy >= H) continue;
                const long q = base + (long)yy * W;
                const unsigned gg = g[q];
                if (gg == D3_INF16) continue;
                const unsigned c = wd + wz * (gg * gg);
                if (c > bd) continue;
                const int ll = near[q];
                if (c < bd || ll < bl) { bd = c; bl = ll; }
            }
        }
        h[p] = (int)min(bd, D3_INF);
        hl[p] = bl;
    }
}

// ---- x pass ---------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / D3_TILE), H, Z), block D3_TILE.  wx = sx^2.  inner modes: h, and the labels from vol; feature modes: (h, hl).
template <int MODE>
__global__ __launch_bounds__(D3_TILE) void dist3_x_kernel(const int* __restrict__ vol, const int* __restrict__ h, const int* __restrict__ hl, int H, int W,
                                                         unsigned wx, int edge, unsigned limit, int maxd, long K, int* __restrict__ out0,
                                                         int* __restrict__ out1, mz_u64* __restrict__ best, int* __restrict__ flags) {
    constexpr bool FEAT = MODE == D3_FEATURE || MODE == D3_EXPAND;
    const int x = blockIdx.x * D3_TILE + (int)threadIdx.x;
    if (x >= W) return;
    const long row = ((long)blockIdx.z * H + blockIdx.y) * W;
    const int l = vol[row + x];
    if (!FEAT) {
        if (MODE != D3_DEPTH) out0[row + x] = 0;
        if (l <= 0 || l > K) {
            if (l != 0) mz_store(flags + 0, 1);
            return;
        }
        unsigned bd = (unsigned)h[row + x];
#pragma unroll
        for (int side = -1; side <= 1; side += 2) {
            for (int d = 1; d <= maxd; ++d) {
                const unsigned wd = wx * (unsigned)(d * d);
                if (wd >= bd) break;
                const int xx = x + side * d;
                if (xx < 0 || xx >= W) {
                    if (edge) bd = wd;
                    break;
                }
                if (vol[row + xx] != l) {
                    bd = wd;
                    break;
                }
                const unsigned hh = (unsigned)h[row + xx];
                if (hh < D3_INF) bd = min(bd, wd + hh);
            }
        }
        if (MODE == D3_INNER) out0[row + x] = (int)bd;
        if (MODE == D3_SHRINK) out0[row + x] = bd > limit ? l : 0;
        if (MODE == D3_DEPTH) {
            const mz_u64 word = ((mz_u64)bd << 32) | (mz_u64)(0xFFFFFFFFu - (unsigned)(row + x));
            mz_send_max(best + (l - 1), word);
        }
    } else {
        if (l < 0 || l > K) mz_store(flags + 0, 1);
        unsigned bd = min((unsigned)h[row + x], D3_INF);
        int bl = bd == D3_INF ? 0 : hl[row + x];
        for (int d = 1; d <= maxd; ++d) {
            const unsigned wd = wx * (unsigned)(d * d);
            if (wd > min(bd, limit)) break;
#pragma unroll
            for (int side = -1; side <= 1; side += 2) {
                const int xx = x + side * d;
                if (xx < 0 || xx >= W) continue;
                const unsigned hh = (unsigned)h[row + xx];
                if (hh >= D3_INF) continue;
                const unsigned c = wd + hh;
                if (c > bd) continue;
                const int ll = hl[row + xx];
                if (c < bd || ll < bl) { bd = c; bl = ll; }
            }
        }
        if (bd > limit) { bd = D3_INF; bl = 0; }
        if (MODE == D3_FEATURE) {
            out0[row + x] = (int)bd;
            out1[row + x] = bl;
        } else {
            out0[row + x] = l > 0 ? l : bl;              // (bd <= limit = r2 wherever bl != 0)
        }
    }
}

// one thread per object: the winning word becomes (r2, x, y, z); an absent id keeps its 0 word: r2 = 0, xyz = (-1, -1, -1)
__global__ __launch_bounds__(256) void dist3_depth_decode_kernel(const mz_u64* __restrict__ best, long K, int H, int W, int* __restrict__ r2,
                                                                int* __restrict__ xyz) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    const mz_u64 w = best[i];
    if (w == 0) {
        r2[i] = 0;
        xyz[3 * i + 0] = -1;
        xyz[3 * i + 1] = -1;
        xyz[3 * i + 2] = -1;
        return;
    }
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(w & 0xffffffffull);
    const unsigned line = idx / (unsigned)W;
    r2[i] = (int)(w >> 32);
    xyz[3 * i + 0] = (int)(idx % (unsigned)W);
    xyz[3 * i + 1] = (int)(line % (unsigned)H);
    xyz[3 * i + 2] = (int)(line / (unsigned)H);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define D3_MAX_B 2147483646L

static bool d3_volume_ok(int Z, int H, int W, long K) {
    return Z >= 1 && Z <= 32767 && H >= 1 && H <= 32767 && W >= 1 && W <= 32767 && (long)Z * H * W <= 2147483647L && K >= 0 && K <= 2147483647L;
}
#define D3_VOLUME_CHECK(what) \
    ULLSAM_CHECK(d3_volume_ok(Z, H, W, K), what ": need 1 <= Z, H, W <= 32767, Z * H * W <= 2^31 - 1 and 0 <= K <= 2^31 - 1")

// B = the largest finite squared distance the passes can form (every term below 2^63: s <= 46340, n <= 32767)
static bool d3_metric_ok(int Z, int H, int W, int sz, int sy, int sx, int ez, int ey, int ex) {
    if (sz < 1 || sz > 46340 || sy < 1 || sy > 46340 || sx < 1 || sx > 46340) return false;
    const long a = (long)sz * (Z - 1 + (ez ? 1 : 0)), b = (long)sy * (H - 1 + (ey ? 1 : 0)), c = (long)sx * (W - 1 + (ex ? 1 : 0));
    return a * a + b * b + c * c <= D3_MAX_B;
}
#define D3_METRIC_CHECK(what) \
    ULLSAM_CHECK(d3_metric_ok(Z, H, W, sz, sy, sx, ez, ey, ex), what ": need 1 <= s <= 46340 and sum of s_a^2 (n_a - 1 + e_a)^2 <= 2^31 - 2")

// the farthest step of a scan along an axis of n voxels at spacing s: the whole line, or floor(sqrt(limit) / s) = isqrt(limit / s^2) when bounded
static int d3_reach(int n, int s, int e, long limit) {
    const int whole = n - 1 + (e ? 1 : 0);
    return limit == 2147483647L ? whole : min(isqrt_floor(limit / ((long)s * s)), whole);
}

extern "C" int ullsam_distance3d_z(const int* volume, int Z, int H, int W, int feature, int ez, long K, unsigned short* g, int* nearest, int* flags,
                                   void* stream) {
    D3_VOLUME_CHECK("distance3d_z");
    ULLSAM_CHECK(!feature || nearest != nullptr, "distance3d_z: the feature transform writes the nearest labels too");
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)H, (unsigned)((Z + D3_BAND - 1) / D3_BAND));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (feature) dist3_z_kernel<true><<<grid, 64, 0, s>>>(volume, Z, H, W, ez, K, g, nearest, flags);
    else dist3_z_kernel<false><<<grid, 64, 0, s>>>(volume, Z, H, W, ez, K, g, nearest, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_distance3d_y(const int* volume, const unsigned short* g, const int* nearest, int Z, int H, int W, int feature, int sz, int sy,
                                   int sx, int ez, int ey, int ex, long limit, int* h, int* hlabel, void* stream) {
    const long K = 0;
    D3_VOLUME_CHECK("distance3d_y");
    D3_METRIC_CHECK("distance3d_y");
    ULLSAM_CHECK(limit >= 0 && limit <= 2147483647L, "distance3d_y: need 0 <= limit <= 2^31 - 1");
    ULLSAM_CHECK(!feature || (nearest != nullptr && hlabel != nullptr), "distance3d_y: the feature transform reads and writes the nearest labels too");
    ULLSAM_CHECK(!feature || (ez == 0 && ey == 0 && ex == 0), "distance3d_y: the feature transform has no edge");
    const int maxd = d3_reach(H, sy, ey, limit);
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)Z);
    const unsigned wz = (unsigned)sz * (unsigned)sz, wy = (unsigned)sy * (unsigned)sy;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (feature) dist3_y_kernel<true><<<grid, dim3(64, 4), 0, s>>>(volume, g, nearest, H, W, wz, wy, ey, (unsigned)limit, maxd, h, hlabel);
    else dist3_y_kernel<false><<<grid, dim3(64, 4), 0, s>>>(volume, g, nearest, H, W, wz, wy, ey, (unsigned)limit, maxd, h, hlabel);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_distance3d_x(const int* volume, const int* h, const int* hlabel, int Z, int H, int W, int mode, int sz, int sy, int sx, int ez,
                                   int ey, int ex, long limit, long K, int* out0, int* out1, unsigned long long* best, int* flags, void* stream) {
    D3_VOLUME_CHECK("distance3d_x");
    D3_METRIC_CHECK("distance3d_x");
    ULLSAM_CHECK(mode >= D3_INNER && mode <= D3_DEPTH, "distance3d_x: mode in 0..4");
    ULLSAM_CHECK(limit >= 0 && limit <= 2147483647L, "distance3d_x: need 0 <= limit <= 2^31 - 1");
    const bool feat = mode == D3_FEATURE || mode == D3_EXPAND;
    ULLSAM_CHECK(!feat || hlabel != nullptr, "distance3d_x: the feature modes read the y pass's nearest labels");
    ULLSAM_CHECK(!feat || (ez == 0 && ey == 0 && ex == 0), "distance3d_x: the feature modes have no edge");
    ULLSAM_CHECK((mode != D3_INNER && mode != D3_DEPTH) || limit == 2147483647L, "distance3d_x: the distance map and the depths are unbounded (limit = 2^31 - 1)");
    ULLSAM_CHECK(mode == D3_DEPTH ? (best != nullptr || K == 0) : out0 != nullptr, "distance3d_x: the mode's output is missing");
    ULLSAM_CHECK(mode != D3_FEATURE || out1 != nullptr, "distance3d_x: the feature pair has two outputs");
    const int maxd = d3_reach(W, sx, ex, limit);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mode == D3_DEPTH && !mz_zero(best, (size_t)K * 8, s)) {
        ullsam_set_error("distance3d_x: memset failed");
        return -2;
    }
    const dim3 grid((unsigned)((W + D3_TILE - 1) / D3_TILE), (unsigned)H, (unsigned)Z);
    mz_u64* b = reinterpret_cast<mz_u64*>(best);
    const unsigned lim = (unsigned)limit, wx = (unsigned)sx * (unsigned)sx;
    switch (mode) {
        case D3_INNER: dist3_x_kernel<D3_INNER><<<grid, D3_TILE, 0, s>>>(volume, h, hlabel, H, W, wx, ex, lim, maxd, K, out0, out1, b, flags); break;
        case D3_FEATURE: dist3_x_kernel<D3_FEATURE><<<grid, D3_TILE, 0, s>>>(volume, h, hlabel, H, W, wx, ex, lim, maxd, K, out0, out1, b, flags); break;
        case D3_EXPAND: dist3_x_kernel<D3_EXPAND><<<grid, D3_TILE, 0, s>>>(volume, h, hlabel, H, W, wx, ex, lim, maxd, K, out0, out1, b, flags); break;
        case D3_SHRINK: dist3_x_kernel<D3_SHRINK><<<grid, D3_TILE, 0, s>>>(volume, h, hlabel, H, W, wx, ex, lim, maxd, K, out0, out1, b, flags); break;
        default: dist3_x_kernel<D3_DEPTH><<<grid, D3_TILE, 0, s>>>(volume, h, hlabel, H, W, wx, ex, lim, maxd, K, out0, out1, b, flags); break;
    }
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_distance3d_depth_decode(const unsigned long long* best, long K, int H, int W, int* r2, int* xyz, void* stream) {
    ULLSAM_CHECK(K >= 0 && K <= 2147483646L && H >= 1 && H <= 32767 && W >= 1 && W <= 32767,
                 "distance3d_depth_decode: need 0 <= K <= 2^31 - 2 and 1 <= H, W <= 32767");
    if (K == 0) return 0;
    dist3_depth_decode_kernel<<<mz_blocks(K), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(reinterpret_cast<const mz_u64*>(best), K, H,
                                                                                                            W, r2, xyz);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
