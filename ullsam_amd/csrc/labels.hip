// Instance label maps (reference: app.py:688-707 save_instance paints every saved mask into one uint16 canvas with
// final_mask[mask] = instance_id, later instances on top; app.py:807-826 export_mask resizes that canvas with Image.NEAREST and removes
// the padding) and the integer contingency table two label images are scored from.  Integer work only: every output is a function of
// which records cover a pixel, so it is bit-exact with the host forms (utils/amg.py) and identical from run to run.
//
// Painting.  Records arrive as uncompressed column-major RLEs (the format of rle_expand_kernel in regions.hip): a run is a vertical
// segment of the image, i.e. a CONTIGUOUS range of the transposed frame rawT[x * H + y].  So the records are painted into a transposed
// int32 scratch [W, H] straight from the concatenated counts -- no per-record [H, W] mask exists at any point.
// A pixel's raw label is 1 + the largest paint rank among the records that cover it (= the result of overwriting in paint order), so the
// merge is an agent-scope integer atomicMax of rank + 1 and the result does not depend on which block runs when.  A plain (wide) store
// cannot take part in a max-merge between concurrently painted records -- it would erase a larger value -- so every painted pixel is one
// atomic; the lanes of a wave cover consecutive addresses (one 256-byte segment per wave instruction), and the owner of a short run
// walks it alone.  One block paints one record.  Every access is clipped to f < H * W and a record whose rank is outside 0..N-1 paints
// nothing, so malformed input cannot write outside the frame or produce a label above N.
// Stats.  Visible area and inclusive XYXY box of every raw label, over the transposed scratch read as one flat array: one atomicAdd per
// run of equal labels of a 64-pixel segment, one per wave for a run of whole segments; a run inside one column x covers rows y0..y1 of
// it, a run that crosses a column end covers row H - 1 of its first and row 0 of its last column, so its box is (x0, 0, x1, H - 1).  A
// box bound is only sent as an atomicMin / atomicMax when a relaxed load says it would improve (bounds move one way, so a stale load
// costs an atomic, never a result).
// Compaction.  One workgroup: the dropped decision, an exclusive scan of the kept flags over the (at most 65535) ranks, the table
// raw label -> final label, label_of_record, the kept labels' areas / boxes, and K.
// Remap.  labels[y, x] = map[rawT[x, y]] through a 32 x 33 LDS tile: coalesced reads of the scratch, coalesced writes of the image.
#include "label_common.h"   // the relaxed atomics, the memset helper
#include <limits.h>

// ---- paint ------------------------------------------------------------------------------------------------------------------
#define LP_PT 8
#define LP_CH (256 * LP_PT)
#define LP_LONG 32
// grid N, block 256.  The scan of the counts is rle_expand_kernel's (2048 counts at a time, 8 per thread, wave scan, carry).
__global__ __launch_bounds__(256) void rle_paint_kernel(const int* __restrict__ counts, const long* __restrict__ offsets,
                                                        const int* __restrict__ rank, long N, long per, int* __restrict__ rawT,
                                                        int* __restrict__ status) {
    __shared__ long start[LP_CH + 1];
    __shared__ long wsum[4];
    __shared__ int bad_s;
    const long n = blockIdx.x;
    const int rk = rank[n];
    if (rk < 0 || rk >= N) {                             // block-uniform: nothing is painted under a label the tables do not hold
        if (threadIdx.x == 0) status[n] = 1;
        return;
    }
    const int value = rk + 1;
    const long c0 = offsets[n], c1 = offsets[n + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) bad_s = 0;
    long carry = 0;
    bool bad = false;
    for (long cb = c0; cb < c1; cb += LP_CH) {           // (LP_CH is even: a run's parity in the chunk is its parity in the record)
        long loc[LP_PT];
        long tsum = 0;
#pragma unroll
        for (int j = 0; j < LP_PT; ++j) {
            const long i = cb + threadIdx.x * LP_PT + j;
            int c = i < c1 ? counts[i] : 0;
            if (c < 0) { bad = true; c = 0; }
            loc[j] = tsum;
            tsum += c;
        }
        long inc = tsum;                                 // inclusive wave scan of the threads' sums (written out: wave_scan_incl() changes this kernel's code)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        __syncthreads();                                 // the previous chunk's readers of start[] / wsum[] are done
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        long before = carry + inc - tsum;
        for (int k = 0; k < wv; ++k) before += wsum[k];
#pragma unroll
        for (int j = 0; j < LP_PT; ++j) start[threadIdx.x * LP_PT + j] = before + loc[j];
        if (threadIdx.x == 255) start[LP_CH] = before + tsum;
        __syncthreads();
        // short 1-runs: the owning thread
#pragma unroll
        for (int j = 1; j < LP_PT; j += 2) {
            const long f0 = before + loc[j];
            const long len = (j + 1 < LP_PT ? before + loc[j + 1] : before + tsum) - f0;
            if (len > 0 && len <= LP_LONG && f0 < per) {
                const long fe = min(f0 + len, per);
                for (long f = f0; f < fe; ++f) mz_max(rawT + f, value);
            }
        }
        // long 1-runs: a wave each, lanes over consecutive f
        for (int r = 1 + 2 * wv; r < LP_CH; r += 8) {
            const long f0 = start[r];
            const long len = start[r + 1] - f0;
            if (len <= LP_LONG || f0 >= per) continue;   // wave-uniform
            const long fe = min(f0 + len, per);
            for (long f = f0 + lane; f < fe; f += 64) mz_max(rawT + f, value);
        }
        carry = start[LP_CH];
    }
    __syncthreads();
    if (bad || carry != per) bad_s = 1;                  // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) status[n] = bad_s;
}

// ---- stats --------------------------------------------------------------------------------------------------------------------
#define LB_SEG 32   // 64-pixel segments per wave
__global__ __launch_bounds__(256) void label_stats_init_kernel(long N, int* __restrict__ areas, int* __restrict__ boxes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    areas[i] = 0;
    boxes[4 * i + 0] = INT_MAX;
    boxes[4 * i + 1] = INT_MAX;
    boxes[4 * i + 2] = -1;
    boxes[4 * i + 3] = -1;
}

// a run of label v (1..N) over the flat transposed range [f0, f0 + cnt)
__device__ __forceinline__ void lb_run(int v, long f0, int cnt, int H, int* __restrict__ areas, int* __restrict__ boxes) {
    mz_add(areas + v, cnt);
    const unsigned int a = (unsigned int)f0, b = (unsigned int)(f0 + cnt - 1);
    const int x0 = (int)(a / (unsigned int)H), x1 = (int)(b / (unsigned int)H);
    int y0 = 0, y1 = H - 1;
    if (x0 == x1) {
        y0 = (int)(a - (unsigned int)x0 * (unsigned int)H);
        y1 = (int)(b - (unsigned int)x1 * (unsigned int)H);
    }
    int* bx = boxes + 4 * (long)v;
    mz_send_min(bx + 0, x0);
    mz_send_min(bx + 1, y0);
    mz_send_max(bx + 2, x1);
    mz_send_max(bx + 3, y1);
}

__global__ __launch_bounds__(256) void label_stats_kernel(const int* __restrict__ rawT, long per, int N, int H, int* __restrict__ areas,
                                                          int* __restrict__ boxes) {
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (LB_SEG * 64);
    int cur = 0, cnt = 0;                                // wave-uniform: a run of whole segments not yet sent (cur == 0: none)
    long cur0 = 0;
    for (int s = 0; s < LB_SEG; ++s) {
        const long s0 = base + (long)s * 64;
        if (s0 >= per) break;                            // wave-uniform
        const long i = s0 + lane;
        int v = i < per ? rawT[i] : 0;
        if (v < 0 || v > N) v = 0;                       // a label the tables do not hold counts as background
        const int prev = __shfl_up(v, 1, 64);
        const bool head = lane == 0 || v != prev;
        const unsigned long long hm = __ballot(head);
        if (hm == 1ull) {                                // one label over the whole segment
            const int v0 = __builtin_amdgcn_readfirstlane(v);
            if (v0 == cur) cnt += 64;
            else {
                if (cur > 0 && lane == 0) lb_run(cur, cur0, cnt, H, areas, boxes);
                cur = v0;
                cur0 = s0;
                cnt = 64;
            }
        } else {
            if (cur > 0 && lane == 0) lb_run(cur, cur0, cnt, H, areas, boxes);
            cur = 0;
            cnt = 0;
            if (head && v > 0) {
                const unsigned long long rest = (hm >> lane) >> 1;    // heads above this lane
                lb_run(v, i, rest ? __builtin_ctzll(rest) + 1 : 64 - lane, H, areas, boxes);
            }
        }
    }
    if (cur > 0 && lane == 0) lb_run(cur, cur0, cnt, H, areas, boxes);
}

// ---- compaction -----------------------------------------------------------------------------------------------------------------
// grid 1, block 256: thread t owns the ranks [t * ceil(N / 256), ...) -- a contiguous share, so the final labels follow paint order.
__global__ __launch_bounds__(256) void label_compact_kernel(const int* __restrict__ areas_raw, const int* __restrict__ boxes_raw,
                                                            const int* __restrict__ rank, int N, int min_visible_area,
                                                            int* __restrict__ map, int* __restrict__ label_of_record,
                                                            int* __restrict__ areas, int* __restrict__ boxes, int* __restrict__ K) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    const int share = (N + 255) / 256;
    const int r0 = min(t * share, N), r1 = min(r0 + share, N);
    int c = 0;
    for (int r = r0; r < r1; ++r) {
        const int a = areas_raw[r + 1];
        c += (a != 0 && a >= min_visible_area) ? 1 : 0;
    }
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
        map[0] = 0;
    }
    __syncthreads();
    int k = part[t];
    for (int r = r0; r < r1; ++r) {
        const int a = areas_raw[r + 1];
        const bool keep = a != 0 && a >= min_visible_area;
        map[r + 1] = keep ? k + 1 : 0;
        if (keep) {
            areas[k] = a;
#pragma unroll
            for (int j = 0; j < 4; ++j) boxes[4 * (long)k + j] = boxes_raw[4 * (long)(r + 1) + j];
            ++k;
        }
    }
    __syncthreads();                                     // map[] is read below by other threads of this workgroup
    for (int i = t; i < N; i += 256) {
        const int rk = rank[i];
        label_of_record[i] = (rk >= 0 && rk < N) ? mz_load(map + rk + 1) : 0;
    }
}

// ---- remap + transpose ----------------------------------------------------------------------------------------------------------
// grid (ceil(W / 32), ceil(H / 32)), block 256 = 32 x 8
__global__ __launch_bounds__(256) void label_remap_kernel(const int* __restrict__ rawT, const int* __restrict__ map, int N, int H, int W,
                                                          int* __restrict__ labels) {
    __shared__ int tile[32][33];
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + ty + 8 * j, y = y0 + tx;
        int out = 0;
        if (x < W && y < H) {
            const int v = rawT[(long)x * H + y];
            if (v > 0 && v <= N) out = map[v];
        }
        tile[ty + 8 * j][tx] = out;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + ty + 8 * j, x = x0 + tx;
        if (y < H && x < W) labels[(long)y * W + x] = tile[tx][ty + 8 * j];
    }
}

// ---- overlap table ----------------------------------------------------------------------------------------------------------------
// T[a, b] += the length of every run of equal (a, b) pairs of a 64-pixel segment of the flat images (a count does not care where a row
// ends), one add per wave for a run of whole segments: the background / background pair of two 2048^2 images costs 2048 adds, not 4 M.
__global__ __launch_bounds__(256) void label_overlap_kernel(const int* __restrict__ A, const int* __restrict__ B, long per, int na, int nb,
                                                            unsigned long long* __restrict__ T, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (LB_SEG * 64);
    const long ld = (long)nb + 1;
    long cur = -1;                                       // wave-uniform: the cell of a run of whole segments not yet added
    unsigned long long cnt = 0;
    bool bad = false;
    for (int s = 0; s < LB_SEG; ++s) {
        const long s0 = base + (long)s * 64;
        if (s0 >= per) break;                            // wave-uniform
        const long i = s0 + lane;
        long cell = -1;                                  // -1: past the end, or an id outside the table (skipped)
        if (i < per) {
            const int a = A[i], b = B[i];
            if (a < 0 || a > na || b < 0 || b > nb) bad = true;
            else cell = (long)a * ld + b;
        }
        const long prev = __shfl_up(cell, 1, 64);
        const bool head = lane == 0 || cell != prev;
        const unsigned long long hm = __ballot(head);
        if (hm == 1ull) {
            const long c0 = __shfl(cell, 0, 64);
            if (c0 == cur) cnt += 64;
            else {
                if (cur >= 0 && lane == 0) mz_add64(T + cur, cnt);
                cur = c0;
                cnt = 64;
            }
        } else {
            if (cur >= 0 && lane == 0) mz_add64(T + cur, cnt);
            cur = -1;
            cnt = 0;
            if (head && cell >= 0) {
                const unsigned long long rest = (hm >> lane) >> 1;
                mz_add64(T + cell, (unsigned long long)(rest ? __builtin_ctzll(rest) + 1 : 64 - lane));
            }
        }
    }
    if (cur >= 0 && lane == 0) mz_add64(T + cur, cnt);
    if (bad) status[0] = 1;                              // (every writer stores the same value)
}

// ---- nearest resize -----------------------------------------------------------------------------------------------------------
// out[y, x] = in[sy(top + y), sx(left + x)], s(d) = min(((2 d + 1) * n_in) / (2 * n_out), n_in - 1).  grid (ceil(w / 256), rows), block 256.
__global__ __launch_bounds__(256) void resize_nearest_i32_kernel(const int* __restrict__ in, long in_ld, int IH, int IW, int OH, int OW, int top,
                                                                 int left, int h, int w, int* __restrict__ out, long out_ld) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const int sx = (int)min(((2L * (left + x) + 1) * IW) / (2L * OW), (long)IW - 1);
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const int sy = (int)min(((2L * (top + y) + 1) * IH) / (2L * OH), (long)IH - 1);
        out[(long)y * out_ld + x] = in[(long)sy * in_ld + sx];
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define LB_FRAME_CHECK(what)                                                                                                 \
    ULLSAM_CHECK(N >= 0 && N <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31), what ": need 0 <= N <= 65535, H, W > 0, H*W < 2^31")

// counts i32 [offsets[N]], offsets i64 [N + 1], rank i32 [N] (a permutation of 0..N-1: the paint order); raw i32 [W, H] (TRANSPOSED:
// raw[x * H + y]) = 1 + the largest rank covering the pixel, 0 where none does; status i32 [N].
extern "C" int ullsam_rle_paint_labels(const int* counts, const long* offsets, const int* rank, long N, int H, int W, int* raw, int* status,
                                       void* stream) {
    LB_FRAME_CHECK("rle_paint_labels");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long per = (long)H * W;
    if (!mz_zero(raw, (size_t)per * 4, s)) { ullsam_set_error("rle_paint_labels: memset failed"); return -2; }
    if (N == 0) return 0;
    rle_paint_kernel<<<(unsigned)N, 256, 0, s>>>(counts, offsets, rank, N, per, raw, status);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// raw i32 [W, H] (transposed, as painted) -> areas i32 [N + 1], boxes i32 [N + 1, 4] (x0, y0, x1, y1 inclusive) indexed by RAW label;
// entry 0 and the labels that are not visible keep area 0 and the box (INT_MAX, INT_MAX, -1, -1).
extern "C" int ullsam_label_stats(const int* raw, long N, int H, int W, int* areas, int* boxes, void* stream) {
    LB_FRAME_CHECK("label_stats");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    label_stats_init_kernel<<<(unsigned)((N + 1 + 255) / 256), 256, 0, s>>>(N, areas, boxes);
    ULLSAM_LAUNCH_CHECK();
    if (N == 0) return 0;
    const long per = (long)H * W;
    const long waves = (per + LB_SEG * 64 - 1) / (LB_SEG * 64);
    label_stats_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, s>>>(raw, per, (int)N, H, areas, boxes);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// areas_raw / boxes_raw as label_stats leaves them; map i32 [N + 1] (raw label -> final label, 0 = dropped), label_of_record i32 [N],
// areas i32 [N] / boxes i32 [N, 4] (their first K entries are written), K i32 [1].
extern "C" int ullsam_label_compact(const int* areas_raw, const int* boxes_raw, const int* rank, long N, int min_visible_area, int* map,
                                    int* label_of_record, int* areas, int* boxes, int* K, void* stream) {
    ULLSAM_CHECK(N >= 0 && N <= 65535, "label_compact: need 0 <= N <= 65535");
    label_compact_kernel<<<1, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(areas_raw, boxes_raw, rank, (int)N, min_visible_area, map,
                                                                              label_of_record, areas, boxes, K);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// labels i32 [H, W] (row-major) = map[raw[x * H + y]]
extern "C" int ullsam_label_remap(const int* raw, const int* map, long N, int H, int W, int* labels, void* stream) {
    LB_FRAME_CHECK("label_remap");
    ULLSAM_CHECK((H + 31) / 32 <= 65535, "label_remap: H <= 32 * 65535");
    label_remap_kernel<<<dim3((unsigned)((W + 31) / 32), (unsigned)((H + 31) / 32)), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        raw, map, (int)N, H, W, labels);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// a, b i32 [H, W]; T u64 [na + 1, nb + 1] (zeroed here); status i32 [1] (zeroed here) = 1 when some id is outside 0..na / 0..nb.
extern "C" int ullsam_label_overlap(const int* a, const int* b, int H, int W, int na, int nb, unsigned long long* T, int* status,
                                    void* stream) {
    ULLSAM_CHECK(H > 0 && W > 0 && (long)H * W < (1L << 31) && na >= 0 && nb >= 0, "label_overlap: need H, W > 0, H*W < 2^31, na, nb >= 0");
    const long cells = ((long)na + 1) * ((long)nb + 1);
    ULLSAM_CHECK(cells <= (1L << 26), "label_overlap: (na + 1) * (nb + 1) must not exceed 2^26 cells (512 MiB of int64)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!mz_zero(T, (size_t)cells * 8, s) || !mz_zero(status, 4, s)) {
        ullsam_set_error("label_overlap: memset failed");
        return -2;
    }
    const long per = (long)H * W;
    const long waves = (per + LB_SEG * 64 - 1) / (LB_SEG * 64);
    label_overlap_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, s>>>(a, b, per, na, nb, T, status);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// in i32 [IH, IW] with row stride in_ld; the image is resized to a virtual [OH, OW] of which the window (top, left, h, w) is written to
// out [h, w] with row stride out_ld.
extern "C" int ullsam_resize_nearest_i32(const int* in, long in_ld, int IH, int IW, int OH, int OW, int top, int left, int h, int w, int* out,
                                         long out_ld, void* stream) {
    ULLSAM_CHECK(IH > 0 && IW > 0 && OH > 0 && OW > 0 && in_ld >= IW, "resize_nearest_i32: need IH, IW, OH, OW > 0 and in_ld >= IW");
    ULLSAM_CHECK(top >= 0 && left >= 0 && h >= 0 && w >= 0 && (long)top + h <= OH && (long)left + w <= OW && out_ld >= w,
                 "resize_nearest_i32: the window must lie inside [OH, OW] and out_ld >= w");
    if (h == 0 || w == 0) return 0;
    resize_nearest_i32_kernel<<<dim3((unsigned)((w + 255) / 256), (unsigned)min(h, 65535)), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        in, in_ld, IH, IW, OH, OW, top, left, h, w, out, out_ld);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
