// Per-object measurements and contacts from a label VOLUME: measure.hip with a third axis (host form and definition: utils/measure3d.py; DESIGN.md
// "7b, continued (3-D measurements)").  Integer work only -- integer atomics, no float anywhere -- so every output is a function of the inputs
// alone: bit-exact with the numpy definition and identical from run to run.
//
// volume i32 [Z, H, W] with ids 0..K (0 = background), 1 <= Z, H, W <= 32767 and Z * H * W <= 2^31 - 1: x * x < 2^30, every count < 2^31, so every
// coordinate sum stays below 2^61 and the largest sum of all, sum v^2 of 16-bit samples, below 65535^2 (2^31 - 1) < 2^63.  Row k - 1 of every table
// belongs to id k.
// measure3d_kernel.  One workgroup of 256 threads owns a tile of 256 columns x M3_TILE_R rows x M3_TILE_P planes; wave w takes the (plane, row)
// lines w, w + 4, ... of the tile, 64 voxels at a time in memory order.  A lane loads its label and the labels at y - 1, y + 1, z - 1, z + 1 (four
// coalesced loads); left and right come by __shfl, with one extra load at each end of the segment; -1 stands for "outside the volume".  Per axis a:
// f_a = the voxel's faces normal to a that face "not k" (0..2), c_a = those facing another object; boundary = any f_a > 0.  The seven counters of a
// lane ride in ONE 64-bit word (8 bits each: boundary <= 64 and every face count <= 128 per segment) through the segmented wave scan of measure.hip
// (head flags by __ballot, six shuffle steps); the run's last lane owns the totals.  Sum x and sum x^2 of a run are closed forms of (x0, n); sum y =
// n y, sum z = n z, sum xy = y sum x, sum xz = z sum x, sum yz = n y z.  A run of whole segments of one label is carried in wave-uniform registers to
// the end of the tile's row.  Background runs send nothing.
// Accumulation: as in measure.hip.  A table in the LDS of the workgroup (open addressing keyed by label, lds_slots entries of 17 + 2 C 64-bit sums
// and 6 + 2 C 32-bit bounds, LDS integer atomics; dynamic LDS, 33344 bytes at 128 slots and C = 4, the 64 bytes of table pointers in front
// included); a label that finds no slot within M3_PROBES probes sends its totals straight to the global tables; at the end of the tile the table is
// flushed with one global atomic per nonzero quantity and label.  lds_slots = 0: everything goes straight to the global tables.  Box, min and max are
// sent only when a relaxed load says they would improve.
// contacts3d_kernel.  One wave per (z, y) row: the key a << 32 | b (a < b, both positive) of the voxel with its right, its y + 1 and its z + 1
// neighbour -- every adjacent voxel pair is seen once -- as runs of equal keys along the row, one carrier per axis, into ONE pair table of
// pair_table.h whose counts are i64 [cap, 3] = (nz, ny, nx).
// An id outside 0..K reads as background and sets flags[0]; no table is indexed with it.  The volume is indexed in 64 bits; every load is one element
// per lane, so any element-aligned base pointer works.  Init kernels set every table: nothing depends on the caller's memory.
#include "pair_table.h"
#include <limits.h>

#define M3_TILE_W 256
#define M3_TILE_R 8      // rows of a tile (ops.MEASURE3D_TILE_R)
#define M3_TILE_P 4      // planes of a tile (ops.MEASURE3D_TILE_P): a voxel's z neighbours are lines of the same workgroup for 3 of 4 planes
#define M3_MAX_SLOTS 128
#define M3_PROBES 8
#define M3_NSUM 17       // voxels; sum x, y, z, x^2, y^2, z^2, xy, xz, yz; boundary voxels, fz, fy, fx, cz, cy, cx
#define M3_MAX_SIDE 32767
#define M3_EVEN_BYTES 0x00ff00ff00ff00ffull   // the 8-bit counters of a segment's scan word, spread to 16-bit fields

typedef unsigned long long m3_u64;

struct M3Out {
    long* voxels;        // [K]
    int* box;            // [K, 6]
    long* mom;           // [K, 9]
    long* surf;          // [K, 7]
    long* isum;          // [K, C]
    long* isum2;         // [K, C]
    int* imin;           // [K, C]
    int* imax;           // [K, C]
};

// The totals of one run of label `label` on row (z, y): columns x0 .. x0 + n - 1.  The seven counters (boundary voxels, fz, fy, fx, cz, cy, cx) in
// 16-bit fields (a tile's row gives at most 512 each): counter 2 i in ca, counter 2 i + 1 in cb, at bit 16 i.
template <int C> struct M3Run {
    int label, x0, n;
    m3_u64 ca, cb;
    int s[C ? C : 1];
    m3_u64 s2[C ? C : 1];
    int mn[C ? C : 1], mx[C ? C : 1];
};

// The tile kernel keeps the eight table pointers in the first 64 bytes of its LDS, in M3Out's order, and reads one where a total leaves for global
// memory: held in scalar registers through the row loop they would push the kernel past its scalar registers (spills).
// the address of the q-th 64-bit sum of table row `row`
template <int C> __device__ __forceinline__ long* m3_sum_ptr(const m3_u64* o, long row, int q) {
    if (q == 0) return reinterpret_cast<long*>(o[0]) + row;
    if (q < 10) return reinterpret_cast<long*>(o[2]) + 9 * row + (q - 1);
    if (q < M3_NSUM) return reinterpret_cast<long*>(o[3]) + 7 * row + (q - 10);
    if (q < M3_NSUM + C) return reinterpret_cast<long*>(o[4]) + C * row + (q - M3_NSUM);
    return reinterpret_cast<long*>(o[5]) + C * row + (q - M3_NSUM - C);
}
// the address of the j-th 32-bit bound of table row `row`: j = 0..2 the box's minima, 3..5 its maxima, then C minima and C maxima of the channels
template <int C> __device__ __forceinline__ int* m3_ext_ptr(const m3_u64* o, long row, int j) {
    if (j < 6) return reinterpret_cast<int*>(o[1]) + 6 * row + j;
    if (j < 6 + C) return reinterpret_cast<int*>(o[6]) + C * row + (j - 6);
    return reinterpret_cast<int*>(o[7]) + C * row + (j - 6 - C);
}
template <int C> __device__ __forceinline__ bool m3_ext_is_min(int j) { return j < 3 || (j >= 6 && j < 6 + C); }

template <int C> __device__ __forceinline__ void m3_emit(const M3Run<C>& r, int y, int z, int slots, int* skey, m3_u64* ssum, int* sext, const m3_u64* out) {
    constexpr int NQ = M3_NSUM + 2 * C, NM = 6 + 2 * C;
    const m3_u64 n = (m3_u64)r.n, x0 = (m3_u64)r.x0, x1 = x0 + n - 1, yy = (m3_u64)y, zz = (m3_u64)z;
    const m3_u64 sx = n * (x0 + x1) / 2;                                                      // n (x0 + x1) is even
    const m3_u64 sxx = (x1 * (x1 + 1) * (2 * x1 + 1) - (x0 ? (x0 - 1) * x0 * (2 * x0 - 1) : 0)) / 6;   // S(x1) - S(x0 - 1), S(m) = m (m + 1) (2 m + 1) / 6 < 2^46
    m3_u64 q[NQ];
    q[0] = n; q[1] = sx; q[2] = n * yy; q[3] = n * zz; q[4] = sxx; q[5] = n * yy * yy; q[6] = n * zz * zz;
    q[7] = sx * yy; q[8] = sx * zz; q[9] = n * yy * zz;
#pragma unroll
    for (int i = 0; i < 7; ++i) q[10 + i] = ((i & 1 ? r.cb : r.ca) >> (16 * (i >> 1))) & 0xffff;
    int m[NM];
    m[0] = r.x0; m[1] = y; m[2] = z; m[3] = (int)x1; m[4] = y; m[5] = z;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        q[M3_NSUM + c] = (m3_u64)r.s[c];
        q[M3_NSUM + C + c] = r.s2[c];
        m[6 + c] = r.mn[c];
        m[6 + C + c] = r.mx[c];
    }
    const int slot = mz_lds_slot<M3_PROBES>(r.label, slots, skey);
    if (slot >= 0) {
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (q[i]) atomicAdd(ssum + slot * NQ + i, q[i]);
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            if (m3_ext_is_min<C>(j)) atomicMin(sext + slot * NM + j, m[j]);
            else atomicMax(sext + slot * NM + j, m[j]);
        }
    } else {
        const long row = (long)r.label - 1;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (q[i]) mz_add64(m3_sum_ptr<C>(out, row, i), q[i]);
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            if (m3_ext_is_min<C>(j)) mz_send_min(m3_ext_ptr<C>(out, row, j), m[j]);
            else mz_send_max(m3_ext_ptr<C>(out, row, j), m[j]);
        }
    }
}

// grid (ceil(W / 256), ceil(H / M3_TILE_R), ceil(Z / M3_TILE_P)), block 256
template <int C>
__global__ __launch_bounds__(256) void measure3d_kernel(const int* __restrict__ vol, int Z, int H, int W, int K, const void* __restrict__ img, int bytes,
                                                        int slots, M3Out tables, int* __restrict__ flags) {
    constexpr int NQ = M3_NSUM + 2 * C, NM = 6 + 2 * C, CC = C ? C : 1;
    extern __shared__ m3_u64 m3_lds[];                  // 64 + slots * (8 NQ + 4 NM + 4) bytes: the table pointers alone with slots = 0
    m3_u64* out = m3_lds;
    m3_u64* ssum = m3_lds + 8;
    int* sext = reinterpret_cast<int*>(ssum + slots * NQ);
    int* skey = sext + slots * NM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        out[0] = (m3_u64)tables.voxels; out[1] = (m3_u64)tables.box; out[2] = (m3_u64)tables.mom; out[3] = (m3_u64)tables.surf;
        out[4] = (m3_u64)tables.isum; out[5] = (m3_u64)tables.isum2; out[6] = (m3_u64)tables.imin; out[7] = (m3_u64)tables.imax;
    }
    for (int i = tid; i < slots; i += 256) skey[i] = 0;
    for (int i = tid; i < slots * NQ; i += 256) ssum[i] = 0;
    for (int i = tid; i < slots * NM; i += 256) sext[i] = m3_ext_is_min<C>(i % NM) ? INT_MAX : -1;
    __syncthreads();
    const int tx0 = blockIdx.x * M3_TILE_W, ty0 = blockIdx.y * M3_TILE_R, tz0 = blockIdx.z * M3_TILE_P;
    const int plane = H * W;                             // < 2^30
    bool bad = false;
    for (int r = wave; r < M3_TILE_R * M3_TILE_P; r += 4) {
        const int y = ty0 + r % M3_TILE_R, z = tz0 + r / M3_TILE_R;
        if (y >= H || z >= Z) continue;                  // wave-uniform (the barrier is below the loop)
        const long row = (long)z * plane + (long)y * W;
        M3Run<C> carry;                                  // wave-uniform: a run of whole segments not yet sent (label 0: none)
        carry.label = 0;
        for (int sg = 0; sg < M3_TILE_W / 64; ++sg) {
            const int xs = tx0 + sg * 64;
            if (xs >= W) break;                          // wave-uniform
            const int x = xs + lane;
            int l = -1, up = -1, dn = -1, zb = -1, zf = -1;
            if (x < W) {
                l = vol[row + x];
                if (l < 0 || l > K) { bad = true; l = 0; }
                if (y > 0) up = mz_clean(vol[row - W + x], K);
                if (y + 1 < H) dn = mz_clean(vol[row + W + x], K);
                if (z > 0) zb = mz_clean(vol[row - plane + x], K);
                if (z + 1 < Z) zf = mz_clean(vol[row + plane + x], K);
            }
            int lf = __shfl_up(l, 1, 64), rt = __shfl_down(l, 1, 64);
            if (lane == 0) lf = xs > 0 ? mz_clean(vol[row + xs - 1], K) : -1;
            if (lane == 63) rt = xs + 64 < W ? mz_clean(vol[row + xs + 64], K) : -1;
            const int k = l > 0 ? l : 0;
            m3_u64 pk = 0;                               // boundary | fz << 8 | fy << 16 | fx << 24 | cz << 32 | cy << 40 | cx << 48
            int s[CC], mn[CC], mx[CC];
            m3_u64 s2[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) { s[c] = 0; s2[c] = 0; mn[c] = INT_MAX; mx[c] = -1; }
            if (k) {
                const int fz = (zb != k) + (zf != k), fy = (up != k) + (dn != k), fx = (lf != k) + (rt != k);
                const int cz = (zb != k && zb > 0) + (zf != k && zf > 0), cy = (up != k && up > 0) + (dn != k && dn > 0),
                          cx = (lf != k && lf > 0) + (rt != k && rt > 0);
                pk = (m3_u64)((fz + fy + fx) > 0 ? 1 : 0) | ((m3_u64)fz << 8) | ((m3_u64)fy << 16) | ((m3_u64)fx << 24) | ((m3_u64)cz << 32) |
                     ((m3_u64)cy << 40) | ((m3_u64)cx << 48);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int v = mz_sample(img, bytes, (row + x) * C + c);
                    s[c] = v; s2[c] = (m3_u64)((unsigned)v * (unsigned)v); mn[c] = v; mx[c] = v;
                }
            }
            const int prev = __shfl_up(k, 1, 64);
            const bool head = lane == 0 || k != prev;
            const m3_u64 hm = __ballot(head);
            const int start = 63 - __builtin_clzll(hm & (~0ull >> (63 - lane)));   // the head of this lane's run (bit 0 is always set)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {           // segmented inclusive scan: lane - d still inside the run
                const bool take = lane - d >= start;
                const m3_u64 tp = __shfl_up(pk, d, 64);
                if (take) pk += tp;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int ts = __shfl_up(s[c], d, 64);
                    const m3_u64 ts2 = __shfl_up(s2[c], d, 64);
                    const int tn = __shfl_up(mn[c], d, 64), tm = __shfl_up(mx[c], d, 64);
                    if (take) { s[c] += ts; s2[c] += ts2; mn[c] = min(mn[c], tn); mx[c] = max(mx[c], tm); }
                }
            }
            M3Run<C> run;
            run.label = k; run.x0 = xs + start; run.n = lane - start + 1;
            run.ca = pk & M3_EVEN_BYTES; run.cb = (pk >> 8) & M3_EVEN_BYTES;
#pragma unroll
            for (int c = 0; c < C; ++c) { run.s[c] = s[c]; run.s2[c] = s2[c]; run.mn[c] = mn[c]; run.mx[c] = mx[c]; }
            const int k0 = __builtin_amdgcn_readfirstlane(k);
            const bool whole = hm == 1ull && k0 > 0;     // one label over the whole segment: lane 63 holds its totals
            const bool more = sg + 1 < M3_TILE_W / 64 && xs + 64 < W;   // the row of the tile goes on (wave-uniform, as is `whole`)
            const bool ext = whole && k0 == carry.label; // the carried run goes on through this segment
            if (carry.label && !ext) {
                if (lane == 0) m3_emit<C>(carry, y, z, slots, skey, ssum, sext, out);
                carry.label = 0;
            }
            if (whole && more) {                         // carried on: nothing is sent for this segment
                if (!ext) {
                    carry.label = k0; carry.x0 = xs; carry.n = 0; carry.ca = 0; carry.cb = 0;
#pragma unroll
                    for (int c = 0; c < C; ++c) { carry.s[c] = 0; carry.s2[c] = 0; carry.mn[c] = INT_MAX; carry.mx[c] = -1; }
                }
                const m3_u64 tpk = __shfl(pk, 63, 64);
                carry.n += 64; carry.ca += tpk & M3_EVEN_BYTES; carry.cb += (tpk >> 8) & M3_EVEN_BYTES;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    carry.s[c] += __shfl(s[c], 63, 64); carry.s2[c] += __shfl(s2[c], 63, 64);
                    carry.mn[c] = min(carry.mn[c], __shfl(mn[c], 63, 64)); carry.mx[c] = max(carry.mx[c], __shfl(mx[c], 63, 64));
                }
            } else {
                if (ext && lane == 63) {                 // the last segment of the tile's row ends the carried run: lane 63's run takes it over
                    run.x0 = carry.x0; run.n += carry.n; run.ca += carry.ca; run.cb += carry.cb;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        run.s[c] += carry.s[c]; run.s2[c] += carry.s2[c];
                        run.mn[c] = min(run.mn[c], carry.mn[c]); run.mx[c] = max(run.mx[c], carry.mx[c]);
                    }
                }
                carry.label = 0;
                const bool last = lane == 63 || (((hm >> lane) >> 1) & 1ull);
                if (last && k) m3_emit<C>(run, y, z, slots, skey, ssum, sext, out);
            }
        }
    }
    if (bad) mz_store(flags + 0, 1);
    __syncthreads();
    for (int i = tid; i < slots * NQ; i += 256) {        // one global atomic per nonzero quantity and label
        const int key = skey[i / NQ];
        const m3_u64 v = ssum[i];
        if (key > 0 && key <= K && v) mz_add64(m3_sum_ptr<C>(out, (long)key - 1, i % NQ), v);
    }
    for (int i = tid; i < slots * NM; i += 256) {
        const int key = skey[i / NM], j = i % NM, v = sext[i];
        if (key <= 0 || key > K) continue;
        if (m3_ext_is_min<C>(j)) { if (v != INT_MAX) mz_send_min(m3_ext_ptr<C>(out, (long)key - 1, j), v); }
        else if (v >= 0) mz_send_max(m3_ext_ptr<C>(out, (long)key - 1, j), v);
    }
}

__global__ __launch_bounds__(256) void measure3d_init_kernel(int K, int C, M3Out out, int* __restrict__ flags) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < 4) flags[k] = 0;
    if (k >= K) return;
    out.voxels[k] = 0;
    for (int j = 0; j < 6; ++j) out.box[6 * k + j] = j < 3 ? INT_MAX : -1;
    for (int j = 0; j < 9; ++j) out.mom[9 * k + j] = 0;
    for (int j = 0; j < 7; ++j) out.surf[7 * k + j] = 0;
    for (int c = 0; c < C; ++c) {
        out.isum[C * k + c] = 0; out.isum2[C * k + c] = 0;
        out.imin[C * k + c] = INT_MAX; out.imax[C * k + c] = -1;
    }
}

// ---- contacts -------------------------------------------------------------------------------------------------------------------------
// grid ceil(Z * H / 4), block 256: one wave per (z, y) row
__global__ __launch_bounds__(256) void contacts3d_kernel(const int* __restrict__ vol, int Z, int H, int W, int K, mz_u64* __restrict__ keys,
                                                         long* __restrict__ counts, mz_u64 mask, int max_pairs, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long line = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= (long)Z * H) return;                     // wave-uniform
    const int z = (int)(line / H), y = (int)(line % H);
    const long plane = (long)H * W, row = line * W;
    auto addz = [&](mz_u64 k, int, int n) { mz_pair_add_axis(k, 0, n, keys, counts, mask, max_pairs, flags); };
    auto addy = [&](mz_u64 k, int, int n) { mz_pair_add_axis(k, 1, n, keys, counts, mask, max_pairs, flags); };
    auto addx = [&](mz_u64 k, int, int n) { mz_pair_add_axis(k, 2, n, keys, counts, mask, max_pairs, flags); };
    MzRun rz = {0, 0, 0}, ry = {0, 0, 0}, rx = {0, 0, 0};
    bool bad = false;
    for (int xs = 0; xs < W; xs += 64) {
        const int x = xs + lane;
        int l = 0, dn = 0, zf = 0;
        if (x < W) {
            l = vol[row + x];
            if (l < 0 || l > K) { bad = true; l = 0; }
            if (y + 1 < H) dn = mz_clean(vol[row + W + x], K);
            if (z + 1 < Z) zf = mz_clean(vol[row + plane + x], K);
        }
        int rt = __shfl_down(l, 1, 64);
        if (lane == 63) rt = xs + 64 < W ? mz_clean(vol[row + xs + 64], K) : 0;
        mz_segment(rx, mz_pair_key(l, rt), xs, lane, addx);
        mz_segment(ry, mz_pair_key(l, dn), xs, lane, addy);
        mz_segment(rz, mz_pair_key(l, zf), xs, lane, addz);
    }
    mz_flush(rx, lane, addx);
    mz_flush(ry, lane, addy);
    mz_flush(rz, lane, addz);
    if (bad) mz_store(flags + 0, 1);
}
__global__ __launch_bounds__(256) void contacts3d_init_kernel(long cap, mz_u64* __restrict__ keys, long* __restrict__ counts, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < 4) flags[i] = 0;
    if (i >= cap) return;
    keys[i] = 0;
    counts[3 * i + 0] = 0; counts[3 * i + 1] = 0; counts[3 * i + 2] = 0;
}
// one thread per slot: the claimed slots, in no particular order, as rows (key, nz, ny, nx); flags[3] counts them
__global__ __launch_bounds__(256) void contacts3d_compact_kernel(const mz_u64* __restrict__ keys, const long* __restrict__ counts, long cap, int max_rows,
                                                                 long* __restrict__ rows, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const mz_u64 k = keys[i];
    if (k == 0) return;
    const int r = __hip_atomic_fetch_add(flags + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r < max_rows) {
        rows[4 * (long)r + 0] = (long)k;
        rows[4 * (long)r + 1] = counts[3 * i + 0];
        rows[4 * (long)r + 2] = counts[3 * i + 1];
        rows[4 * (long)r + 3] = counts[3 * i + 2];
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
#define M3_VOLUME_CHECK(what) \
    ULLSAM_CHECK(Z >= 1 && H >= 1 && W >= 1 && Z <= M3_MAX_SIDE && H <= M3_MAX_SIDE && W <= M3_MAX_SIDE && (long)Z * H * W <= 2147483647L && K >= 0 && \
                 K <= 2147483646, what ": need 1 <= Z, H, W <= 32767, Z * H * W <= 2^31 - 1 and 0 <= K <= 2^31 - 2")

extern "C" int ullsam_measure_objects3d(const int* volume, int Z, int H, int W, int K, const void* intensity, int channels, int sample_bytes, int lds_slots,
                                        long* voxels, int* box, long* moments, long* surface, long* isum, long* isum2, int* imin, int* imax,
                                        int* flags, void* stream) {
    M3_VOLUME_CHECK("measure_objects3d");
    ULLSAM_CHECK(channels >= 0 && channels <= 4 && (channels == 0 || sample_bytes == 1 || sample_bytes == 2),
                 "measure_objects3d: need 0 <= channels <= 4 of 1- or 2-byte samples");
    ULLSAM_CHECK(channels == 0 || intensity != nullptr, "measure_objects3d: channels > 0 without an image");
    ULLSAM_CHECK(lds_slots >= 0 && lds_slots <= M3_MAX_SLOTS && (lds_slots & (lds_slots - 1)) == 0,
                 "measure_objects3d: lds_slots must be 0 or a power of two <= 128");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const M3Out out = {voxels, box, moments, surface, isum, isum2, imin, imax};
    measure3d_init_kernel<<<(unsigned)(((long)K + 255) / 256 + 1), 256, 0, s>>>(K, channels, out, flags);
    ULLSAM_LAUNCH_CHECK();
    const dim3 grid((unsigned)((W + M3_TILE_W - 1) / M3_TILE_W), (unsigned)((H + M3_TILE_R - 1) / M3_TILE_R), (unsigned)((Z + M3_TILE_P - 1) / M3_TILE_P));
    const size_t lds = 64 + (size_t)lds_slots * (8 * (M3_NSUM + 2 * channels) + 4 * (6 + 2 * channels) + 4);   // at most 33344 bytes
    switch (channels) {
        case 0: measure3d_kernel<0><<<grid, 256, lds, s>>>(volume, Z, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        case 1: measure3d_kernel<1><<<grid, 256, lds, s>>>(volume, Z, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        case 2: measure3d_kernel<2><<<grid, 256, lds, s>>>(volume, Z, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        case 3: measure3d_kernel<3><<<grid, 256, lds, s>>>(volume, Z, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        default: measure3d_kernel<4><<<grid, 256, lds, s>>>(volume, Z, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
    }
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_object_contacts3d(const int* volume, int Z, int H, int W, int K, unsigned long long* keys, long* counts, long cap, int max_pairs,
                                        long* rows, int* flags, void* stream) {
    M3_VOLUME_CHECK("object_contacts3d");
    ULLSAM_CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && max_pairs >= 1 && 2L * max_pairs <= cap && cap <= (1L << 31),
                 "object_contacts3d: the capacity must be a power of two with 2 * max_pairs <= capacity <= 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    contacts3d_init_kernel<<<mz_blocks(cap), 256, 0, s>>>(cap, keys, counts, flags);
    ULLSAM_LAUNCH_CHECK();
    contacts3d_kernel<<<(unsigned)(((long)Z * H + 3) / 4), 256, 0, s>>>(volume, Z, H, W, K, keys, counts, (mz_u64)(cap - 1), max_pairs, flags);
    ULLSAM_LAUNCH_CHECK();
    contacts3d_compact_kernel<<<mz_blocks(cap), 256, 0, s>>>(keys, counts, cap, max_pairs, rows, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
