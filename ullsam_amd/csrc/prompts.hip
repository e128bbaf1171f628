// Point prompts, boxes and per-instance masks from one instance label image (reference: train_joint_v2.py:313-468, the dataset's per-sample
// loop of scipy calls: a 10-iteration binary_erosion, a 10-iteration binary_dilation, a one-step erosion and a full-frame
// distance_transform_edt per chosen instance).  Integer work only; every output is bit-equal to the definitions of DESIGN.md "7b, continued
// (prompts)" and tests/prompts_ref.py, and identical from run to run.
//
// Interior (one pass pair for ALL instances).  d1[p] = the city-block distance from p to the nearest pixel whose label differs from
// labels[p], the outside of the frame counting as different, truncated to R + 1 (R = inner_radius): a row pass takes the distance to the
// nearest different pixel of the row, a column pass takes min(|dy| + (row y + dy differs at x ? 0 : rowdist[y + dy, x])).
// inner_i = {p in M_i : d1[p] > R} = binary_erosion(M_i, iterations = R) with the default cross.
// Choice.  One workgroup lists the present ids of the area table in increasing order and, when there are more than max_instances, draws
// max_instances of them (Philox counter (0, t, 1, 0)).
// Candidate sets (per chosen instance, windowed).  The window is the instance's box grown by hi and clipped to the frame, cut into tiles of
// 64 columns (aligned to 64) x 16 rows.  A tile loads the "label == id" bytes of its rows +- hi and columns +- hi into the LDS, takes
// g = the distance to the nearest instance pixel of the column within +- hi, then D2 = min over |dx| <= hi of dx^2 + g^2: exact wherever
// D2 <= hi^2, which is all the ring asks (lo^2 <= D2 <= hi^2 outside M_i).  A wave handles a row of 64 pixels, so each candidate set leaves
// ONE 64-bit ballot word per (instance, row, 64-column word) and one atomicAdd per row word into the row's count: the sets are kept as bit
// rows + row counts, never as a distance map.  The same pass sums x and y over M_i (the centroid of an instance without interior).
// Points.  One wave per instance: a rank among the candidates in row-major order is found by a prefix scan over the row counts, then over the
// popcounts of the row's words, then by clearing the lowest set bits of the word.  Ranks come from the draw rule (philox.h).
#include "label_common.h"   // the relaxed load
#include "philox.h"
#include <limits.h>

#define PR_IDS 65535        // ids are 1..65535
#define PR_RMAX 64          // inner_radius and ring[1] at most
#define PR_PTS 16           // num_pos, num_neg at most
#define PR_TR 16            // rows of a tile
#define PR_TILES 64         // blocks per instance in prompt_sets_kernel (each strides over the window's tiles)

// ---- interior: truncated city-block distance to the nearest different label -------------------------------------------------------
// grid (ceil(W / 256), min(H, 65535)), block 256
__global__ __launch_bounds__(256) void label_rowdist_kernel(const int* __restrict__ labels, int H, int W, int R, unsigned char* __restrict__ hd,
                                                            int* __restrict__ status) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int* row = labels + (long)y * W;
        const int L = row[x];
        if (L < 0 || L > PR_IDS) status[0] = 1;             // (every writer stores the same value)
        int h = R + 1;
        for (int dx = 1; dx <= R; ++dx) {
            if (x - dx < 0 || x + dx >= W || row[x - dx] != L || row[x + dx] != L) { h = dx; break; }
        }
        hd[(long)y * W + x] = (unsigned char)h;
    }
}

__global__ __launch_bounds__(256) void label_coldist_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ hd, int H, int W, int R,
                                                            unsigned char* __restrict__ d1) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int L = labels[(long)y * W + x];
        int best = hd[(long)y * W + x];                      // <= R + 1, so dy < best keeps dy <= R
        for (int dy = 1; dy < best; ++dy) {
            int up = dy, dn = dy;
            if (y - dy >= 0 && labels[(long)(y - dy) * W + x] == L) up = dy + hd[(long)(y - dy) * W + x];
            if (y + dy < H && labels[(long)(y + dy) * W + x] == L) dn = dy + hd[(long)(y + dy) * W + x];
            best = min(best, min(up, dn));
        }
        d1[(long)y * W + x] = (unsigned char)best;
    }
}

// ---- instance choice --------------------------------------------------------------------------------------------------------------
// grid 1, block 256: thread t owns the ids 256 t + 1 .. 256 t + 256 (a contiguous share: the list comes out in increasing order).
__global__ __launch_bounds__(256) void prompt_choose_kernel(const int* __restrict__ areas, int max_inst, unsigned long long seed,
                                                            int* __restrict__ present, int* __restrict__ sorted, int* __restrict__ sel,
                                                            int* __restrict__ info) {
    __shared__ int part[256];
    __shared__ int total_s;
    const int t = threadIdx.x;
    const int i0 = t * 256 + 1, i1 = min(i0 + 256, PR_IDS + 1);
    int c = 0;
    for (int i = i0; i < i1; ++i) c += areas[i] > 0 ? 1 : 0;
    part[t] = c;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = s;
            s += v;
        }
        total_s = s;
    }
    __syncthreads();
    int k = part[t];
    for (int i = i0; i < i1; ++i)
        if (areas[i] > 0) present[k++] = i;
    __syncthreads();                                         // present[] is read below by other threads of this workgroup
    const int P = total_s;
    if (P <= max_inst) {
        for (int j = t; j < P; j += 256) sel[j] = mz_load(present + j);
        if (t == 0) info[0] = P;
        return;
    }
    if (t != 0) return;
    for (int tt = 0; tt < max_inst; ++tt) {                  // the draw rule, earlier picks kept sorted
        const unsigned int w = philox4x32_10_word0((unsigned int)seed, (unsigned int)(seed >> 32), 0u, (unsigned int)tt, 1u, 0u);
        int r = (int)(((unsigned long long)w * (unsigned long long)(P - tt)) >> 32);
        int j = 0;
        while (j < tt && sorted[j] <= r) { ++r; ++j; }
        for (int q = tt; q > j; --q) sorted[q] = sorted[q - 1];
        sorted[j] = r;
        sel[tt] = mz_load(present + r);
    }
    info[0] = max_inst;
}

// ---- candidate sets ---------------------------------------------------------------------------------------------------------------
struct PrWindow { int bx0, by0, bx1, by1, wx0, wy0, wx1, wy1; };
// boxes_t is label_stats' box table of the label image read as a transposed map: (x0, y0, x1, y1) there = (y0, x0, y1, x1) here
__device__ __forceinline__ PrWindow pr_window(const int* __restrict__ boxes_t, int id, int hi, int H, int W) {
    PrWindow q;
    q.by0 = max(boxes_t[4 * id + 0], 0);
    q.bx0 = max(boxes_t[4 * id + 1], 0);
    q.by1 = min(boxes_t[4 * id + 2], H - 1);
    q.bx1 = min(boxes_t[4 * id + 3], W - 1);
    q.wx0 = max(q.bx0 - hi, 0);
    q.wy0 = max(q.by0 - hi, 0);
    q.wx1 = min(q.bx1 + hi, W - 1);
    q.wy1 = min(q.by1 + hi, H - 1);
    return q;
}

// grid (PR_TILES, slots), block 256.  bits u64 [2, slots, H, Ww], rowcnt i32 [2, slots, H] (zeroed by the caller), sums u64 [slots, 2] (zeroed).
__global__ __launch_bounds__(256) void prompt_sets_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ d1, int H, int W,
                                                          const int* __restrict__ areas, const int* __restrict__ boxes_t,
                                                          const int* __restrict__ sel, const int* __restrict__ info, int slots, int R, int lo, int hi,
                                                          unsigned long long* __restrict__ bits, int* __restrict__ rowcnt,
                                                          unsigned long long* __restrict__ sums, unsigned char* __restrict__ dbg_inner,
                                                          unsigned char* __restrict__ dbg_ring) {
    __shared__ unsigned char m[(PR_TR + 2 * PR_RMAX) * (64 + 2 * PR_RMAX)];
    __shared__ unsigned char g[PR_TR * (64 + 2 * PR_RMAX)];
    const int s = blockIdx.y;
    if (s >= min(info[0], slots)) return;                    // block-uniform
    const int id = sel[s];
    if (id < 1 || id > PR_IDS || areas[id] <= 0) return;
    const PrWindow q = pr_window(boxes_t, id, hi, H, W);
    const int Ww = (W + 63) >> 6;
    const int tx0 = q.wx0 >> 6, ntx = (q.wx1 >> 6) - tx0 + 1, nty = (q.wy1 - q.wy0) / PR_TR + 1;
    const int pitch = 64 + 2 * hi;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lo2 = lo * lo, hi2 = hi * hi;
    unsigned long long sx = 0, sy = 0;
    for (int tile = blockIdx.x; tile < ntx * nty; tile += gridDim.x) {
        const int xa = (tx0 + tile % ntx) * 64, ya = q.wy0 + (tile / ntx) * PR_TR;
        const int rows = min(PR_TR, q.wy1 - ya + 1);
        __syncthreads();                                     // the previous tile's readers of m[] / g[] are done
        for (int i = threadIdx.x; i < (rows + 2 * hi) * pitch; i += 256) {
            const int y = ya - hi + i / pitch, x = xa - hi + i % pitch;
            m[i] = (y >= 0 && y < H && x >= 0 && x < W && labels[(long)y * W + x] == id) ? 1 : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < rows * pitch; i += 256) {
            const int r = i / pitch + hi, c = i % pitch;
            int gv = 255;                                    // no instance pixel of this column within +- hi
            if (m[r * pitch + c]) gv = 0;
            else
                for (int dy = 1; dy <= hi; ++dy)
                    if (m[(r - dy) * pitch + c] || m[(r + dy) * pitch + c]) { gv = dy; break; }
            g[i] = (unsigned char)gv;
        }
        __syncthreads();
        for (int r = wv; r < rows; r += 4) {                 // wave-uniform trip count
            const int y = ya + r, x = xa + lane;
            const bool in_frame = x < W;
            const bool is_m = m[(r + hi) * pitch + lane + hi] != 0;
            bool ring = false;
            if (in_frame && !is_m) {
                int best = INT_MAX;
                for (int dx = -hi; dx <= hi; ++dx) {
                    const int gv = g[r * pitch + lane + hi + dx];
                    if (gv != 255) best = min(best, dx * dx + gv * gv);
                }
                ring = best >= lo2 && best <= hi2;
            }
            const bool inner = is_m && d1[(long)y * W + x] > R;     // (is_m implies in_frame)
            const unsigned long long bi = __ballot(inner), br = __ballot(ring);
            if (lane == 0) {
                const long row_i = (long)s * H + y, row_r = ((long)slots + s) * H + y;
                bits[row_i * Ww + (xa >> 6)] = bi;
                bits[row_r * Ww + (xa >> 6)] = br;
                if (bi) atomicAdd(rowcnt + row_i, __popcll(bi));
                if (br) atomicAdd(rowcnt + row_r, __popcll(br));
            }
            if (is_m) { sx += (unsigned long long)x; sy += (unsigned long long)y; }
            if (dbg_inner && in_frame) {
                dbg_inner[((long)s * H + y) * W + x] = inner ? 1 : 0;
                dbg_ring[((long)s * H + y) * W + x] = ring ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64);
        sy += __shfl_xor(sy, o, 64);
    }
    if (lane == 0 && (sx | sy)) {
        atomicAdd(sums + 2 * (long)s, sx);
        atomicAdd(sums + 2 * (long)s + 1, sy);
    }
}

// ---- points -----------------------------------------------------------------------------------------------------------------------
// the first index i in [i0, i1] whose running sum of cnt(i) exceeds `rank`; `rank` becomes the rank inside it.  All 64 lanes, uniform arguments.
template <typename F> __device__ __forceinline__ int pr_find(int i0, int i1, long& rank, int lane, F cnt) {
    long base = 0;
    for (int a = i0; a <= i1; a += 64) {
        const int i = a + lane;
        const long c = i <= i1 ? (long)cnt(i) : 0;
        long inc = c;                                    // (written out: wave_scan_incl() changes the callers' code)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        const long tot = __shfl(inc, 63, 64);
        if (rank < base + tot) {
            const unsigned long long bm = __ballot(base + inc > rank);
            const int f = __builtin_ctzll(bm);
            rank -= base + __shfl(inc - c, f, 64);
            return a + f;
        }
        base += tot;
    }
    return -1;
}

// the pixel of rank `rank` (row-major) of candidate set `set` of slot s, rows y0..y1, words w0..w1
__device__ __forceinline__ void pr_locate(const unsigned long long* __restrict__ bits, const int* __restrict__ rowcnt, int set, int slots, int s, int H,
                                          int Ww, int y0, int y1, int w0, int w1, long rank, int lane, int& px, int& py) {
    const long rbase = ((long)set * slots + s) * H;
    px = 0;
    py = 0;
    const int y = pr_find(y0, y1, rank, lane, [&](int i) { return rowcnt[rbase + i]; });
    if (y < 0) return;
    const unsigned long long* rowbits = bits + (rbase + y) * Ww;
    const int w = pr_find(w0, w1, rank, lane, [&](int i) { return __popcll(rowbits[i]); });
    if (w < 0) return;
    unsigned long long v = rowbits[w];
    for (long i = 0; i < rank; ++i) v &= v - 1;
    px = w * 64 + __builtin_ctzll(v);
    py = y;
}

// k distinct ranks out of m by the draw rule (counter (id, t + 16 kind, 0, 0)), in pick order; `sorted` is scratch
__device__ __forceinline__ void pr_draw(unsigned long long seed, int id, int kind, int k, long m, int* picks, int* sorted) {
    for (int t = 0; t < k; ++t) {
        const unsigned int w = philox4x32_10_word0((unsigned int)seed, (unsigned int)(seed >> 32), (unsigned int)id, (unsigned int)(t + 16 * kind), 0u, 0u);
        int r = (int)(((unsigned long long)w * (unsigned long long)(m - t)) >> 32);
        int j = 0;
        while (j < t && sorted[j] <= r) { ++r; ++j; }
        for (int q = t; q > j; --q) sorted[q] = sorted[q - 1];
        sorted[j] = r;
        picks[t] = r;
    }
}

// grid slots, block 64.  coords f32 [slots, num_pos + num_neg, 2], boxes f32 [slots, 4], counts i32 [slots, 2], info i32 [2 + 4 slots].
__global__ __launch_bounds__(64) void prompt_points_kernel(int H, int W, const int* __restrict__ areas, const int* __restrict__ boxes_t,
                                                           const int* __restrict__ sel, int* __restrict__ info, int slots, int hi, int num_pos,
                                                           int num_neg, unsigned long long seed, const unsigned long long* __restrict__ bits,
                                                           const int* __restrict__ rowcnt, const unsigned long long* __restrict__ sums,
                                                           float* __restrict__ coords, float* __restrict__ boxes, int* __restrict__ counts) {
    __shared__ int picks[2 * PR_PTS];
    __shared__ int sorted[PR_PTS];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= min(info[0], slots)) return;
    const int id = sel[s];
    int* out = info + 2 + 4 * (long)s;
    if (id < 1 || id > PR_IDS || areas[id] <= 0) {           // an explicit id that is absent: the caller reads area 0 and raises
        if (lane == 0) { out[0] = id; out[1] = 0; out[2] = 0; out[3] = 0; }
        return;
    }
    const int area = areas[id];
    const PrWindow q = pr_window(boxes_t, id, hi, H, W);
    const int Ww = (W + 63) >> 6;
    long ni = 0, nr = 0;
    for (int y = q.by0 + lane; y <= q.by1; y += 64) ni += rowcnt[(long)s * H + y];
    for (int y = q.wy0 + lane; y <= q.wy1; y += 64) nr += rowcnt[((long)slots + s) * H + y];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ni += __shfl_xor(ni, o, 64);
        nr += __shfl_xor(nr, o, 64);
    }
    if (lane == 0) {
        if (ni >= num_pos) pr_draw(seed, id, 0, num_pos, ni, picks, sorted);
        else
            for (int j = 0; j < num_pos; ++j) picks[j] = ni > 0 ? (int)(j % ni) : 0;
        if (nr >= num_neg) pr_draw(seed, id, 1, num_neg, nr, picks + PR_PTS, sorted);
        out[0] = id; out[1] = area; out[2] = (int)ni; out[3] = (int)nr;
        counts[2 * (long)s] = (int)ni;
        counts[2 * (long)s + 1] = (int)nr;
        boxes[4 * (long)s + 0] = (float)q.bx0;
        boxes[4 * (long)s + 1] = (float)q.by0;
        boxes[4 * (long)s + 2] = (float)q.bx1;
        boxes[4 * (long)s + 3] = (float)q.by1;
    }
    __syncthreads();
    float* pts = coords + (long)s * (num_pos + num_neg) * 2;
    for (int j = 0; j < num_pos; ++j) {
        int px, py;
        if (ni > 0) pr_locate(bits, rowcnt, 0, slots, s, H, Ww, q.by0, q.by1, q.bx0 >> 6, q.bx1 >> 6, picks[j], lane, px, py);
        else {                                               // no interior: the centroid, floor of the means (int(np.mean(...)))
            px = (int)(sums[2 * (long)s] / (unsigned long long)area);
            py = (int)(sums[2 * (long)s + 1] / (unsigned long long)area);
        }
        if (lane == 0) { pts[2 * j] = (float)px; pts[2 * j + 1] = (float)py; }
    }
    if (nr >= num_neg)                                       // otherwise the caller applies the fallbacks (it reads the ring count)
        for (int j = 0; j < num_neg; ++j) {
            int px, py;
            pr_locate(bits, rowcnt, 1, slots, s, H, Ww, q.wy0, q.wy1, q.wx0 >> 6, q.wx1 >> 6, picks[PR_PTS + j], lane, px, py);
            if (lane == 0) { pts[2 * (num_pos + j)] = (float)px; pts[2 * (num_pos + j) + 1] = (float)py; }
        }
}

// ---- per-instance masks -----------------------------------------------------------------------------------------------------------
// grid (ceil(per / 1024), N), block 256
__global__ __launch_bounds__(256) void instance_masks_kernel(const int* __restrict__ labels, const int* __restrict__ ids, long per,
                                                             float* __restrict__ masks) {
    const int id = ids[blockIdx.y];
    const long i0 = (long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + 256 * j;
        if (i < per) masks[(long)blockIdx.y * per + i] = labels[i] == id ? 1.f : 0.f;
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define PR_FRAME_CHECK(what) ULLSAM_CHECK(H > 0 && W > 0 && (long)H * W < (1L << 31), what ": need H, W > 0, H*W < 2^31")

// labels i32 [H, W]; rowdist u8 [H, W] (scratch); d1 u8 [H, W] = min(d1, radius + 1); status i32 [1] is set to 1 when a label is outside 0..65535
extern "C" int ullsam_label_d1(const int* labels, int H, int W, int radius, unsigned char* rowdist, unsigned char* d1, int* status, void* stream) {
    PR_FRAME_CHECK("label_d1");
    ULLSAM_CHECK(radius >= 0 && radius <= PR_RMAX, "label_d1: need 0 <= radius <= 64");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)min(H, 65535));
    label_rowdist_kernel<<<grid, 256, 0, s>>>(labels, H, W, radius, rowdist, status);
    ULLSAM_LAUNCH_CHECK();
    label_coldist_kernel<<<grid, 256, 0, s>>>(labels, rowdist, H, W, radius, d1);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// areas i32 [65536] (label_stats with N = 65535); present i32 [65535], sorted i32 [max_instances] (scratch); sel i32 [max_instances];
// info[0] = the number chosen
extern "C" int ullsam_prompt_choose(const int* areas, int max_instances, unsigned long long seed, int* present, int* sorted, int* sel, int* info,
                                    void* stream) {
    ULLSAM_CHECK(max_instances >= 1 && max_instances <= PR_IDS, "prompt_choose: need 1 <= max_instances <= 65535");
    prompt_choose_kernel<<<1, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(areas, max_instances, seed, present, sorted, sel, info);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_prompt_sets(const int* labels, const unsigned char* d1, int H, int W, const int* areas, const int* boxes_t, const int* sel,
                                  const int* info, int slots, int radius, int lo, int hi, unsigned long long* bits, int* rowcnt,
                                  unsigned long long* sums, unsigned char* dbg_inner, unsigned char* dbg_ring, void* stream) {
    PR_FRAME_CHECK("prompt_sets");
    ULLSAM_CHECK(slots >= 1 && slots <= PR_IDS, "prompt_sets: need 1 <= slots <= 65535");
    ULLSAM_CHECK(radius >= 0 && radius <= PR_RMAX && lo >= 0 && lo <= hi && hi <= PR_RMAX, "prompt_sets: need 0 <= radius <= 64 and 0 <= lo <= hi <= 64");
    ULLSAM_CHECK((dbg_inner == nullptr) == (dbg_ring == nullptr), "prompt_sets: give both debug images or neither");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool ok = hipMemsetAsync(rowcnt, 0, (size_t)2 * slots * H * 4, s) == hipSuccess && hipMemsetAsync(sums, 0, (size_t)slots * 16, s) == hipSuccess;
    if (ok && dbg_inner)
        ok = hipMemsetAsync(dbg_inner, 0, (size_t)slots * H * W, s) == hipSuccess && hipMemsetAsync(dbg_ring, 0, (size_t)slots * H * W, s) == hipSuccess;
    if (!ok) { ullsam_set_error("prompt_sets: memset failed"); return -2; }
    prompt_sets_kernel<<<dim3(PR_TILES, (unsigned)slots), 256, 0, s>>>(labels, d1, H, W, areas, boxes_t, sel, info, slots, radius, lo, hi, bits, rowcnt,
                                                                        sums, dbg_inner, dbg_ring);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_prompt_points(int H, int W, const int* areas, const int* boxes_t, const int* sel, int* info, int slots, int hi, int num_pos,
                                    int num_neg, unsigned long long seed, const unsigned long long* bits, const int* rowcnt,
                                    const unsigned long long* sums, float* coords, float* boxes, int* counts, void* stream) {
    PR_FRAME_CHECK("prompt_points");
    ULLSAM_CHECK(slots >= 1 && slots <= PR_IDS && hi >= 0 && hi <= PR_RMAX, "prompt_points: need 1 <= slots <= 65535, 0 <= hi <= 64");
    ULLSAM_CHECK(num_pos >= 0 && num_pos <= PR_PTS && num_neg >= 0 && num_neg <= PR_PTS, "prompt_points: need 0 <= num_pos, num_neg <= 16");
    prompt_points_kernel<<<(unsigned)slots, 64, 0, reinterpret_cast<hipStream_t>(stream)>>>(H, W, areas, boxes_t, sel, info, slots, hi, num_pos, num_neg,
                                                                                            seed, bits, rowcnt, sums, coords, boxes, counts);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// masks f32 [N, per] = (labels == ids[n])
extern "C" int ullsam_instance_masks(const int* labels, const int* ids, long N, long per, float* masks, void* stream) {
    ULLSAM_CHECK(N >= 0 && N <= PR_IDS && per > 0 && per < (1L << 31), "instance_masks: need 0 <= N <= 65535, 0 < H*W < 2^31");
    if (N == 0) return 0;
    instance_masks_kernel<<<dim3((unsigned)((per + 1023) / 1024), (unsigned)N), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(labels, ids, per, masks);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
