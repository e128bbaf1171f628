// Per-instance measurements and contacts from a label image (host form and definition: utils/measure.py; DESIGN.md "7b, continued:
// measurements").  Integer work only -- integer atomics, no float anywhere -- so every output is a function of the inputs alone: bit-exact
// with the numpy definition and identical from run to run.
//
// labels i32 [H, W] with ids 0..K (0 = background), 1 <= H, W <= 46340: x * x < 2^31 and every area < 2^31, so every sum stays below 2^62.
// Row k - 1 of every table belongs to label k.
// measure_kernel.  One workgroup of 256 threads owns a 256-column x 32-row tile of the frame; wave w takes the rows w, w + 4, ... of the tile,
// 64 pixels at a time in memory order.  A lane loads its label and the labels above and below (rows y - 1, y + 1, coalesced); left and right
// come by __shfl, with one extra load at each end of the segment; -1 stands for "outside the frame".  From the four neighbours: edges = the
// sides facing "not k" (0..4), contact_edges = those facing another instance, boundary = edges > 0.  A run of equal labels inside the segment is
// reduced by a segmented wave scan (head flags by __ballot, six shuffle steps); the run's last lane owns the totals.  Sum x and sum x^2 of a run
// are closed forms of (x0, len); sum y, sum y^2, sum xy follow from y.  A run of whole segments of one label is carried in wave-uniform
// registers to the end of the tile's row.  Background runs send nothing.
// Accumulation.  The run's totals go into a table in the LDS of the workgroup (open addressing keyed by label, lds_slots entries of 64-bit
// sums, LDS integer atomics; dynamic LDS); a label that finds no slot within MS_PROBES probes sends its totals straight to the global tables,
// one 64-bit integer atomic per nonzero quantity (integer adds commute: same result).  At the end of the tile the table is flushed with one
// global atomic per nonzero quantity and label.  lds_slots = 0: everything goes straight to the global tables; measured, the table is about
// 1.5 x faster per call (profiles/r16_measure.txt).  Box, min and max are sent only when a relaxed load says they would improve.
// contacts_kernel.  One wave per row: the key a << 32 | b (a < b, both positive) of the pixel with its right neighbour and of the pixel with
// the one below -- every adjacent pixel pair is seen once -- as runs of equal keys along the row into the pair table of pair_table.h (64-bit counts here).
// An id outside 0..K reads as background and sets flags[0]; no table is indexed with it.  The frame is indexed in 64 bits; every load is one
// element per lane, so any element-aligned base pointer works.  Init kernels set every table: nothing depends on the caller's memory.
#include "pair_table.h"
#include <limits.h>

#define MS_TILE_W 256
#define MS_TILE_H 32
#define MS_MAX_SLOTS 128
#define MS_PROBES 8
#define MS_NSUM 9        // area, sum x, sum y, sum x^2, sum y^2, sum xy, boundary pixels, edges, contact edges

typedef unsigned long long ms_u64;

struct MsOut {
    long* area;          // [K]
    int* box;            // [K, 4]
    long* mom;           // [K, 5]
    long* per;           // [K, 3]
    long* isum;          // [K, C]
    long* isum2;         // [K, C]
    int* imin;           // [K, C]
    int* imax;           // [K, C]
};

// The totals of one run of label `label` on row y: columns x0 .. x0 + n - 1.
template <int C> struct MsRun {
    int label, x0, n;
    int bnd, e, ce;
    int s[C ? C : 1];
    ms_u64 s2[C ? C : 1];
    int mn[C ? C : 1], mx[C ? C : 1];
};

// the address of the q-th 64-bit sum of table row `row`
template <int C> __device__ __forceinline__ long* ms_sum_ptr(const MsOut& o, long row, int q) {
    if (q == 0) return o.area + row;
    if (q < 6) return o.mom + 5 * row + (q - 1);
    if (q < MS_NSUM) return o.per + 3 * row + (q - 6);
    if (q < MS_NSUM + C) return o.isum + C * row + (q - MS_NSUM);
    return o.isum2 + C * row + (q - MS_NSUM - C);
}
// the address of the j-th 32-bit bound of table row `row`: j = 0, 1 the box's minima, 2, 3 its maxima, then C minima and C maxima of the channels
template <int C> __device__ __forceinline__ int* ms_ext_ptr(const MsOut& o, long row, int j) {
    if (j < 4) return o.box + 4 * row + j;
    if (j < 4 + C) return o.imin + C * row + (j - 4);
    return o.imax + C * row + (j - 4 - C);
}
template <int C> __device__ __forceinline__ bool ms_ext_is_min(int j) { return j < 2 || (j >= 4 && j < 4 + C); }

template <int C> __device__ __forceinline__ void ms_emit(const MsRun<C>& r, int y, int slots, int* skey, ms_u64* ssum, int* sext, const MsOut& out) {
    constexpr int NQ = MS_NSUM + 2 * C, NM = 4 + 2 * C;
    const ms_u64 n = (ms_u64)r.n, x0 = (ms_u64)r.x0, x1 = x0 + n - 1, yy = (ms_u64)y;
    const ms_u64 sx = n * (x0 + x1) / 2;                                                      // n (x0 + x1) is even
    const ms_u64 sxx = (x1 * (x1 + 1) * (2 * x1 + 1) - (x0 ? (x0 - 1) * x0 * (2 * x0 - 1) : 0)) / 6;   // S(x1) - S(x0 - 1), S(m) = m (m + 1) (2 m + 1) / 6 < 2^48
    ms_u64 q[NQ];
    q[0] = n; q[1] = sx; q[2] = n * yy; q[3] = sxx; q[4] = n * yy * yy; q[5] = sx * yy;
    q[6] = (ms_u64)r.bnd; q[7] = (ms_u64)r.e; q[8] = (ms_u64)r.ce;
    int m[NM];
    m[0] = r.x0; m[1] = y; m[2] = (int)x1; m[3] = y;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        q[MS_NSUM + c] = (ms_u64)r.s[c];
        q[MS_NSUM + C + c] = r.s2[c];
        m[4 + c] = r.mn[c];
        m[4 + C + c] = r.mx[c];
    }
    const int slot = mz_lds_slot<MS_PROBES>(r.label, slots, skey);
    if (slot >= 0) {                                     // (this tail and m3_emit's are alike, but one template for both changes both tile kernels' code)
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (q[i]) atomicAdd(ssum + slot * NQ + i, q[i]);
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            if (ms_ext_is_min<C>(j)) atomicMin(sext + slot * NM + j, m[j]);
            else atomicMax(sext + slot * NM + j, m[j]);
        }
    } else {
        const long row = (long)r.label - 1;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (q[i]) mz_add64(ms_sum_ptr<C>(out, row, i), q[i]);
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            if (ms_ext_is_min<C>(j)) mz_send_min(ms_ext_ptr<C>(out, row, j), m[j]);
            else mz_send_max(ms_ext_ptr<C>(out, row, j), m[j]);
        }
    }
}

// grid (ceil(W / 256), ceil(H / 32)), block 256
template <int C>
__global__ __launch_bounds__(256) void measure_kernel(const int* __restrict__ labels, int H, int W, int K, const void* __restrict__ img, int bytes,
                                                      int slots, MsOut out, int* __restrict__ flags) {
    constexpr int NQ = MS_NSUM + 2 * C, NM = 4 + 2 * C, CC = C ? C : 1;
    extern __shared__ ms_u64 ms_lds[];                  // slots * (8 NQ + 4 NM + 4) bytes: nothing with slots = 0
    ms_u64* ssum = ms_lds;
    int* sext = reinterpret_cast<int*>(ssum + slots * NQ);
    int* skey = sext + slots * NM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < slots; i += 256) skey[i] = 0;
    for (int i = tid; i < slots * NQ; i += 256) ssum[i] = 0;
    for (int i = tid; i < slots * NM; i += 256) sext[i] = ms_ext_is_min<C>(i % NM) ? INT_MAX : -1;
    __syncthreads();
    const int tx0 = blockIdx.x * MS_TILE_W, ty0 = blockIdx.y * MS_TILE_H;
    bool bad = false;
    for (int r = wave; r < MS_TILE_H; r += 4) {
        const int y = ty0 + r;
        if (y >= H) break;                               // wave-uniform (the barrier is below the loop)
        const long row = (long)y * W;
        MsRun<C> carry;                                  // wave-uniform: a run of whole segments not yet sent (label 0: none)
        carry.label = 0;
        for (int sg = 0; sg < MS_TILE_W / 64; ++sg) {
            const int xs = tx0 + sg * 64;
            if (xs >= W) break;                          // wave-uniform
            const int x = xs + lane;
            int l = -1, up = -1, dn = -1;
            if (x < W) {
                l = labels[row + x];
                if (l < 0 || l > K) { bad = true; l = 0; }
                if (y > 0) up = mz_clean(labels[row - W + x], K);
                if (y + 1 < H) dn = mz_clean(labels[row + W + x], K);
            }
            int lf = __shfl_up(l, 1, 64), rt = __shfl_down(l, 1, 64);
            if (lane == 0) lf = xs > 0 ? mz_clean(labels[row + xs - 1], K) : -1;
            if (lane == 63) rt = xs + 64 < W ? mz_clean(labels[row + xs + 64], K) : -1;
            const int k = l > 0 ? l : 0;
            int e = 0, ce = 0;
            int s[CC], mn[CC], mx[CC];
            ms_u64 s2[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) { s[c] = 0; s2[c] = 0; mn[c] = INT_MAX; mx[c] = -1; }
            if (k) {
                e = (up != k) + (dn != k) + (lf != k) + (rt != k);
                ce = (up != k && up > 0) + (dn != k && dn > 0) + (lf != k && lf > 0) + (rt != k && rt > 0);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int v = mz_sample(img, bytes, (row + x) * C + c);
                    s[c] = v; s2[c] = (ms_u64)((unsigned)v * (unsigned)v); mn[c] = v; mx[c] = v;
                }
            }
            int pk = (e > 0 ? 1 : 0) | (e << 8) | (ce << 18);   // boundary <= 64, edges <= 256, contact edges <= 256 per segment: one scan for the three
            const int prev = __shfl_up(k, 1, 64);
            const bool head = lane == 0 || k != prev;
            const ms_u64 hm = __ballot(head);
            const int start = 63 - __builtin_clzll(hm & (~0ull >> (63 - lane)));   // the head of this lane's run (bit 0 is always set)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {           // segmented inclusive scan: lane - d still inside the run
                const bool take = lane - d >= start;
                const int tp = __shfl_up(pk, d, 64);
                if (take) pk += tp;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int ts = __shfl_up(s[c], d, 64);
                    const ms_u64 ts2 = __shfl_up(s2[c], d, 64);
                    const int tn = __shfl_up(mn[c], d, 64), tm = __shfl_up(mx[c], d, 64);
                    if (take) { s[c] += ts; s2[c] += ts2; mn[c] = min(mn[c], tn); mx[c] = max(mx[c], tm); }
                }
            }
            MsRun<C> run;
            run.label = k; run.x0 = xs + start; run.n = lane - start + 1;
            run.bnd = pk & 0xff; run.e = (pk >> 8) & 0x3ff; run.ce = (pk >> 18) & 0x3ff;
#pragma unroll
            for (int c = 0; c < C; ++c) { run.s[c] = s[c]; run.s2[c] = s2[c]; run.mn[c] = mn[c]; run.mx[c] = mx[c]; }
            const int k0 = __builtin_amdgcn_readfirstlane(k);
            if (hm == 1ull && k0 > 0) {                  // one label over the whole segment: lane 63 holds its totals
                MsRun<C> t;
                t.bnd = __shfl(run.bnd, 63, 64); t.e = __shfl(run.e, 63, 64); t.ce = __shfl(run.ce, 63, 64);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    t.s[c] = __shfl(s[c], 63, 64); t.s2[c] = __shfl(s2[c], 63, 64);
                    t.mn[c] = __shfl(mn[c], 63, 64); t.mx[c] = __shfl(mx[c], 63, 64);
                }
                if (k0 == carry.label) {
                    carry.n += 64; carry.bnd += t.bnd; carry.e += t.e; carry.ce += t.ce;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        carry.s[c] += t.s[c]; carry.s2[c] += t.s2[c];
                        carry.mn[c] = min(carry.mn[c], t.mn[c]); carry.mx[c] = max(carry.mx[c], t.mx[c]);
                    }
                } else {
                    if (carry.label && lane == 0) ms_emit<C>(carry, y, slots, skey, ssum, sext, out);
                    carry = t;
                    carry.label = k0; carry.x0 = xs; carry.n = 64;
                }
            } else {
                if (carry.label && lane == 0) ms_emit<C>(carry, y, slots, skey, ssum, sext, out);
                carry.label = 0;
                const bool last = lane == 63 || (((hm >> lane) >> 1) & 1ull);
                if (last && k) ms_emit<C>(run, y, slots, skey, ssum, sext, out);
            }
        }
        if (carry.label && lane == 0) ms_emit<C>(carry, y, slots, skey, ssum, sext, out);
    }
    if (bad) mz_store(flags + 0, 1);
    __syncthreads();
    for (int i = tid; i < slots * NQ; i += 256) {        // one global atomic per nonzero quantity and label
        const int key = skey[i / NQ];
        const ms_u64 v = ssum[i];
        if (key > 0 && key <= K && v) mz_add64(ms_sum_ptr<C>(out, (long)key - 1, i % NQ), v);
    }
    for (int i = tid; i < slots * NM; i += 256) {
        const int key = skey[i / NM], j = i % NM, v = sext[i];
        if (key <= 0 || key > K) continue;
        if (ms_ext_is_min<C>(j)) { if (v != INT_MAX) mz_send_min(ms_ext_ptr<C>(out, (long)key - 1, j), v); }
        else if (v >= 0) mz_send_max(ms_ext_ptr<C>(out, (long)key - 1, j), v);
    }
}

__global__ __launch_bounds__(256) void measure_init_kernel(int K, int C, MsOut out, int* __restrict__ flags) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < 4) flags[k] = 0;
    if (k >= K) return;
    out.area[k] = 0;
    out.box[4 * k + 0] = INT_MAX; out.box[4 * k + 1] = INT_MAX; out.box[4 * k + 2] = -1; out.box[4 * k + 3] = -1;
    for (int j = 0; j < 5; ++j) out.mom[5 * k + j] = 0;
    for (int j = 0; j < 3; ++j) out.per[3 * k + j] = 0;
    for (int c = 0; c < C; ++c) {
        out.isum[C * k + c] = 0; out.isum2[C * k + c] = 0;
        out.imin[C * k + c] = INT_MAX; out.imax[C * k + c] = -1;
    }
}

// ---- contacts -------------------------------------------------------------------------------------------------------------------------
// grid ceil(H / 4), block 256: one wave per row
__global__ __launch_bounds__(256) void contacts_kernel(const int* __restrict__ labels, int H, int W, int K, mz_u64* __restrict__ keys,
                                                       long* __restrict__ counts, mz_u64 mask, int max_pairs, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= H) return;                                  // wave-uniform
    const long row = (long)y * W;
    auto add = [&](mz_u64 k, int, int n) { mz_pair_add(k, n, keys, counts, mask, max_pairs, flags); };
    MzRun rr = {0, 0, 0}, rd = {0, 0, 0};
    bool bad = false;
    for (int xs = 0; xs < W; xs += 64) {
        const int x = xs + lane;
        int l = 0, dn = 0;
        if (x < W) {
            l = labels[row + x];
            if (l < 0 || l > K) { bad = true; l = 0; }
            if (y + 1 < H) dn = mz_clean(labels[row + W + x], K);
        }
        int rt = __shfl_down(l, 1, 64);
        if (lane == 63) rt = xs + 64 < W ? mz_clean(labels[row + xs + 64], K) : 0;
        mz_segment(rr, mz_pair_key(l, rt), xs, lane, add);
        mz_segment(rd, mz_pair_key(l, dn), xs, lane, add);
    }
    mz_flush(rr, lane, add);
    mz_flush(rd, lane, add);
    if (bad) mz_store(flags + 0, 1);
}
__global__ __launch_bounds__(256) void contacts_init_kernel(long cap, mz_u64* __restrict__ keys, long* __restrict__ counts, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < 4) flags[i] = 0;
    if (i >= cap) return;
    keys[i] = 0;
    counts[i] = 0;
}
// one thread per slot: the claimed slots, in no particular order, as rows (key, n); flags[3] counts them
__global__ __launch_bounds__(256) void contacts_compact_kernel(const mz_u64* __restrict__ keys, const long* __restrict__ counts, long cap, int max_rows,
                                                               long* __restrict__ rows, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const mz_u64 k = keys[i];
    if (k == 0) return;
    const int r = __hip_atomic_fetch_add(flags + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r < max_rows) {
        rows[2 * (long)r + 0] = (long)k;
        rows[2 * (long)r + 1] = counts[i];
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
#define MS_FRAME_CHECK(what) \
    ULLSAM_CHECK(H >= 1 && W >= 1 && H <= 46340 && W <= 46340 && K >= 0 && K <= 2147483646, what ": need 1 <= H, W <= 46340 and 0 <= K <= 2^31 - 2")

extern "C" int ullsam_measure_instances(const int* labels, int H, int W, int K, const void* intensity, int channels, int sample_bytes, int lds_slots,
                                        long* area, int* box, long* moments, long* perimeter, long* isum, long* isum2, int* imin, int* imax,
                                        int* flags, void* stream) {
    MS_FRAME_CHECK("measure_instances");
    ULLSAM_CHECK(channels >= 0 && channels <= 4 && (channels == 0 || sample_bytes == 1 || sample_bytes == 2),
                 "measure_instances: need 0 <= channels <= 4 of 1- or 2-byte samples");
    ULLSAM_CHECK(channels == 0 || intensity != nullptr, "measure_instances: channels > 0 without an image");
    ULLSAM_CHECK(lds_slots >= 0 && lds_slots <= MS_MAX_SLOTS && (lds_slots & (lds_slots - 1)) == 0,
                 "measure_instances: lds_slots must be 0 or a power of two <= 128");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const MsOut out = {area, box, moments, perimeter, isum, isum2, imin, imax};
    measure_init_kernel<<<(unsigned)(((long)K + 255) / 256 + 1), 256, 0, s>>>(K, channels, out, flags);
    ULLSAM_LAUNCH_CHECK();
    const dim3 grid((unsigned)((W + MS_TILE_W - 1) / MS_TILE_W), (unsigned)((H + MS_TILE_H - 1) / MS_TILE_H));
    const size_t lds = (size_t)lds_slots * (8 * (MS_NSUM + 2 * channels) + 4 * (4 + 2 * channels) + 4);   // at most 24064 bytes
    switch (channels) {
        case 0: measure_kernel<0><<<grid, 256, lds, s>>>(labels, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        case 1: measure_kernel<1><<<grid, 256, lds, s>>>(labels, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        case 2: measure_kernel<2><<<grid, 256, lds, s>>>(labels, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        case 3: measure_kernel<3><<<grid, 256, lds, s>>>(labels, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
        default: measure_kernel<4><<<grid, 256, lds, s>>>(labels, H, W, K, intensity, sample_bytes, lds_slots, out, flags); break;
    }
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_label_contacts(const int* labels, int H, int W, int K, unsigned long long* keys, long* counts, long cap, int max_pairs,
                                     long* rows, int* flags, void* stream) {
    MS_FRAME_CHECK("label_contacts");
    ULLSAM_CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && max_pairs >= 1 && 2L * max_pairs <= cap && cap <= (1L << 31),
                 "label_contacts: the capacity must be a power of two with 2 * max_pairs <= capacity <= 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    contacts_init_kernel<<<mz_blocks(cap), 256, 0, s>>>(cap, keys, counts, flags);
    ULLSAM_LAUNCH_CHECK();
    contacts_kernel<<<(unsigned)((H + 3) / 4), 256, 0, s>>>(labels, H, W, K, keys, counts, (mz_u64)(cap - 1), max_pairs, flags);
    ULLSAM_LAUNCH_CHECK();
    contacts_compact_kernel<<<mz_blocks(cap), 256, 0, s>>>(keys, counts, cap, max_pairs, rows, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
