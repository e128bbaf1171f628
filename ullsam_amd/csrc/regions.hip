// Connected regions of binary masks: batched 8-connected labelling, small-region removal, inverse RLE (reference:
// utils/amg.py:267-291 remove_small_regions, :138-150 rle_to_mask).  Integer work only: every result is a function of region
// membership and integer sizes, so the outputs are bit-exact with the host helpers and identical from run to run.
//
// Labelling.  The label of a region is the row-major linear index (within its mask) of its raster-first pixel = the minimum
// index of the region; pixels outside the working set get -1.  The label array doubles as the union-find parent array
// (parent[i] <= i, parents only ever decrease), in three launches whose boundaries are the only cross-workgroup ordering:
//   1. label_tile_kernel    union-find of a 32 x 64 tile in LDS, written out as global indices (every pixel -> its tile root);
//   2. label_merge_kernel   one thread per pixel on a tile border joins it to its neighbours across the border.  The eight XCDs
//                           have private L2s, so inside this launch every write of the parent array is an agent-scope atomicMin
//                           and every read an agent-scope relaxed atomic load; a read may still return an OLDER parent, which
//                           is an ancestor all the same (the atomicMin that links a root returns the true old value, and the
//                           loop goes on from it).  No workgroup waits for another; every loop ends by monotone decrease.
//   3. label_flatten_kernel every pixel -> its root (in place: a racing reader sees the old parent or the root, both ancestors).
// Which edges are joined: in raster order a pixel has to meet one pixel of every component of its earlier neighbours NW, N, NE, W.
// N touches the other three, and NW touches W, so: N alone if present, else NW and NE, and W only without NW.  The closure of the
// joined edges does not depend on the order of the joins, so the parallel result is the sequential one.
// Areas.  Integer atomicAdd into a per-root counter, one add per run of equal labels of a 64-pixel segment, and one add per
// wave for a run that spans whole segments (a 2048^2 background region costs 2048 adds, not 4 M).
#include "label_common.h"   // the relaxed atomics, the global union-find

#define RG_TW 64
#define RG_TH 32
#define RG_PX (RG_TW * RG_TH / 256)

__device__ __forceinline__ int rg_find_lds(const int* p, int i) {
    int q = p[i];
    while (q != i) { i = q; q = p[i]; }
    return i;
}
__device__ __forceinline__ void rg_union_lds(int* p, int a, int b) {
    for (;;) {
        a = rg_find_lds(p, a);
        b = rg_find_lds(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&p[a], b);   // a was a root when read: link it under the smaller root
        if (old == a) return;
        a = old;                               // somebody linked a first: a ~ old still has to meet b
    }
}

// grid (tiles x, tiles y, N); block 256.  bg = 1: the working set is mask == 0, else mask != 0.
__global__ __launch_bounds__(256) void label_tile_kernel(const unsigned char* __restrict__ masks, int H, int W, int bg,
                                                         int* __restrict__ labels) {
    __shared__ int par[RG_TW * RG_TH];
    const long base = (long)blockIdx.z * H * W;
    const int x0 = blockIdx.x * RG_TW, y0 = blockIdx.y * RG_TH;
#pragma unroll
    for (int k = 0; k < RG_PX; ++k) {
        const int p = k * 256 + threadIdx.x;
        const int y = y0 + p / RG_TW, x = x0 + p % RG_TW;
        bool in = false;
        if (y < H && x < W) in = (masks[base + (long)y * W + x] != 0) != (bg != 0);
        par[p] = in ? p : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RG_PX; ++k) {
        const int p = k * 256 + threadIdx.x;
        if (par[p] < 0) continue;                      // (-1 never changes; members only move between non-negative values)
        const int r = p / RG_TW, c = p % RG_TW;
        const bool up = r > 0;
        if (up && par[p - RG_TW] >= 0) {
            rg_union_lds(par, p, p - RG_TW);
        } else {
            const bool nw = up && c > 0 && par[p - RG_TW - 1] >= 0;
            if (nw) rg_union_lds(par, p, p - RG_TW - 1);
            if (up && c < RG_TW - 1 && par[p - RG_TW + 1] >= 0) rg_union_lds(par, p, p - RG_TW + 1);
            if (!nw && c > 0 && par[p - 1] >= 0) rg_union_lds(par, p, p - 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RG_PX; ++k) {
        const int p = k * 256 + threadIdx.x;
        const int y = y0 + p / RG_TW, x = x0 + p % RG_TW;
        if (y >= H || x >= W) continue;
        int out = -1;
        if (par[p] >= 0) {
            const int root = rg_find_lds(par, p);      // minimum local index = minimum global index of the tile's part
            out = (y0 + root / RG_TW) * W + (x0 + root % RG_TW);
        }
        labels[base + (long)y * W + x] = out;
    }
}

// One thread per pixel of a tile's top row (y % TH == 0, y > 0: joins N, else NW and NE) or left column (x % TW == 0, x > 0:
// joins W, else NW and SW -- SW's edge to this pixel is SW's own NE edge, needed when SW has no N, i.e. no W here); a pair of
// pixels that crosses both borders has its lower pixel on a top row.  grid (ceil(border pixels / 256), N).
__global__ __launch_bounds__(256) void label_merge_kernel(int H, int W, int nhb, int nvb, int* __restrict__ labels) {
    int* L = labels + (long)blockIdx.y * H * W;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long nh = (long)nhb * W;
    if (t < nh) {
        const int y = (int)(t / W + 1) * RG_TH, x = (int)(t % W);
        const int p = y * W + x;
        if (mz_load(L + p) < 0) return;
        const int q = p - W;
        if (mz_load(L + q) >= 0) {
            mz_union(L, p, q);
        } else {
            if (x > 0 && mz_load(L + q - 1) >= 0) mz_union(L, p, q - 1);
            if (x < W - 1 && mz_load(L + q + 1) >= 0) mz_union(L, p, q + 1);
        }
    } else if (t < nh + (long)nvb * H) {
        const long u = t - nh;
        const int x = (int)(u / H + 1) * RG_TW, y = (int)(u % H);
        const int p = y * W + x;
        if (mz_load(L + p) < 0) return;
        const int q = p - 1;
        if (mz_load(L + q) >= 0) {
            mz_union(L, p, q);
        } else {
            if (y > 0 && mz_load(L + q - W) >= 0) mz_union(L, p, q - W);
            if (y < H - 1 && mz_load(L + q + W) >= 0) mz_union(L, p, q + W);
        }
    }
}

__global__ __launch_bounds__(256) void label_flatten_kernel(long per, int* __restrict__ labels) {
    int* L = labels + (long)blockIdx.y * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const int q = L[i];
        if (q < 0 || q == (int)i) continue;
        int r = q, n = L[r];
        while (n != r) { r = n; n = L[r]; }
        if (r != q) L[i] = r;
    }
}

// ---- areas: per-root counters ------------------------------------------------------------------------------------------
#define RG_SEG 32   // 64-pixel segments per wave
__global__ __launch_bounds__(256) void region_area_kernel(const int* __restrict__ labels, long per, int* __restrict__ areas) {
    const int* L = labels + (long)blockIdx.y * per;
    int* A = areas + (long)blockIdx.y * per;
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (RG_SEG * 64);
    int cur = -1, cnt = 0;                               // wave-uniform: a run of whole segments not yet added
    for (int s = 0; s < RG_SEG; ++s) {
        if (base + (long)s * 64 >= per) break;           // wave-uniform
        const long i = base + (long)s * 64 + lane;
        const int v = i < per ? L[i] : -1;
        const int prev = __shfl_up(v, 1, 64);
        const bool head = lane == 0 || v != prev;
        const unsigned long long hm = __ballot(head);
        if (hm == 1ull) {                                // one label over the whole segment
            const int v0 = __builtin_amdgcn_readfirstlane(v);
            if (v0 == cur) cnt += 64;
            else {
                if (cur >= 0 && lane == 0) atomicAdd(&A[cur], cnt);
                cur = v0;
                cnt = 64;
            }
        } else {
            if (cur >= 0 && lane == 0) atomicAdd(&A[cur], cnt);
            cur = -1;
            cnt = 0;
            if (head && v >= 0) {
                const unsigned long long rest = (hm >> lane) >> 1;    // heads above this lane
                atomicAdd(&A[v], rest ? __builtin_ctzll(rest) + 1 : 64 - lane);
            }
        }
    }
    if (cur >= 0 && lane == 0) atomicAdd(&A[cur], cnt);
}

// per mask: flags bit 0 = some region is small, bit 1 = some region is not; best = max over regions of area << 32 | ~root
// (largest area, then the smallest root = np.argmax over raster-ordered labels).
struct RegionInfo { unsigned long long best; unsigned int flags; unsigned int pad; };

__global__ __launch_bounds__(256) void region_decide_kernel(const int* __restrict__ labels, const int* __restrict__ areas, long per,
                                                            int thresh, RegionInfo* __restrict__ info) {
    const int* L = labels + (long)blockIdx.y * per;
    const int* A = areas + (long)blockIdx.y * per;
    unsigned long long best = 0;
    unsigned int flags = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        if (L[i] != (int)i) continue;                    // roots only
        const int a = A[i];
        flags |= a < thresh ? 1u : 2u;
        const unsigned long long key = ((unsigned long long)(unsigned int)a << 32) | (unsigned int)~(unsigned int)i;
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        flags |= __shfl_xor(flags, o, 64);
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0 && flags) {
        atomicOr(&info[blockIdx.y].flags, flags);
        atomicMax(&info[blockIdx.y].best, best);
    }
}

// holes (bg = 1): out = mask | (its region of zeros is small).  islands: out = mask & (its region is not small, or every region
// is small and this is the largest).  changed = some region was small.
__global__ __launch_bounds__(256) void region_apply_kernel(const int* __restrict__ labels, const int* __restrict__ areas, long per,
                                                           int thresh, int bg, const RegionInfo* __restrict__ info,
                                                           unsigned char* __restrict__ out, unsigned char* __restrict__ changed) {
    const long n = blockIdx.y;
    const RegionInfo inf = info[n];
    const int keep_root = (inf.flags & 2u) ? -1 : (int)~(unsigned int)(inf.best & 0xffffffffull);   // all small: the largest stays
    if (blockIdx.x == 0 && threadIdx.x == 0) changed[n] = (unsigned char)(inf.flags & 1u);
    const int* L = labels + n * per;
    const int* A = areas + n * per;
    unsigned char* o = out + n * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const int l = L[i];
        unsigned char v;
        if (l < 0) v = bg ? 1 : 0;                       // outside the working set: holes -> the mask is 1 there, islands -> 0
        else {
            const bool small = A[l] < thresh;
            v = bg ? (small ? 1 : 0) : ((!small || l == keep_root) ? 1 : 0);
        }
        o[i] = v;
    }
}

static int label_launch(const unsigned char* masks, long N, int H, int W, int bg, int* labels, hipStream_t s) {
    const long per = (long)H * W;
    const dim3 tiles((unsigned)((W + RG_TW - 1) / RG_TW), (unsigned)((H + RG_TH - 1) / RG_TH), (unsigned)N);
    label_tile_kernel<<<tiles, 256, 0, s>>>(masks, H, W, bg, labels);
    ULLSAM_LAUNCH_CHECK();
    const int nhb = (int)tiles.y - 1, nvb = (int)tiles.x - 1;
    const long border = (long)nhb * W + (long)nvb * H;
    if (border > 0) {                                    // (a single tile is final after the first launch)
        label_merge_kernel<<<dim3((unsigned)((border + 255) / 256), (unsigned)N), 256, 0, s>>>(H, W, nhb, nvb, labels);
        ULLSAM_LAUNCH_CHECK();
        const unsigned bx = (unsigned)max(1L, min((per + 1023) / 1024, 4096L));
        label_flatten_kernel<<<dim3(bx, (unsigned)N), 256, 0, s>>>(per, labels);
        ULLSAM_LAUNCH_CHECK();
    }
    return 0;
}

#define RG_SHAPE_CHECK(what)                                                                                                   \
    ULLSAM_CHECK(N > 0 && N <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31) && (H + RG_TH - 1) / RG_TH <= 65535,        \
                 what ": need 0 < N <= 65535, H, W > 0, H*W < 2^31, H <= 32 * 65535")

// masks u8 [N, H, W] (non-zero = set); background = 0 labels the set pixels, 1 the zero pixels; labels i32 [N, H, W].
extern "C" int ullsam_label_regions(const unsigned char* masks, long N, int H, int W, int background, int* labels, void* stream) {
    if (N == 0) return 0;
    RG_SHAPE_CHECK("label_regions");
    return label_launch(masks, N, H, W, background != 0, labels, reinterpret_cast<hipStream_t>(stream));
}

// mode 0 = "holes", 1 = "islands"; area_thresh = ceil of the host's float threshold (sizes are integers).  workspace: 16-byte
// aligned, >= N * (8 * H * W + 16) bytes = labels i32 [N, H, W] (left there for the caller) | areas i32 [N, H, W] | 16 bytes per
// mask.  masks_out may be masks_in (the masks are read by the labelling only).  changed u8 [N].
extern "C" int ullsam_remove_small_regions(const unsigned char* masks_in, unsigned char* masks_out, long N, int H, int W, int area_thresh,
                                           int mode, void* workspace, long workspace_bytes, unsigned char* changed, void* stream) {
    if (N == 0) return 0;
    RG_SHAPE_CHECK("remove_small_regions");
    ULLSAM_CHECK(mode == 0 || mode == 1, "remove_small_regions: mode must be 0 (holes) or 1 (islands)");
    const long per = (long)H * W;
    ULLSAM_CHECK(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= N * (8 * per + 16),
                 "remove_small_regions: workspace must be 16-byte aligned and hold N * (8 * H * W + 16) bytes");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int* labels = reinterpret_cast<int*>(workspace);
    int* areas = labels + N * per;
    RegionInfo* info = reinterpret_cast<RegionInfo*>(areas + N * per);   // 8 * N * per bytes into an aligned buffer: 8-byte aligned
    const int bg = mode == 0;
    const int rc = label_launch(masks_in, N, H, W, bg, labels, s);
    if (rc != 0) return rc;
    if (hipMemsetAsync(areas, 0, (size_t)N * (4 * per + 16), s) != hipSuccess) { ullsam_set_error("remove_small_regions: memset failed"); return -2; }
    const long waves = (per + RG_SEG * 64 - 1) / (RG_SEG * 64);
    region_area_kernel<<<dim3((unsigned)((waves + 3) / 4), (unsigned)N), 256, 0, s>>>(labels, per, areas);
    ULLSAM_LAUNCH_CHECK();
    const unsigned bx = (unsigned)max(1L, min((per + 4095) / 4096, 1024L));
    region_decide_kernel<<<dim3(bx, (unsigned)N), 256, 0, s>>>(labels, areas, per, area_thresh, info);
    ULLSAM_LAUNCH_CHECK();
    region_apply_kernel<<<dim3(bx, (unsigned)N), 256, 0, s>>>(labels, areas, per, area_thresh, bg, info, masks_out, changed);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ---- inverse RLE (utils/amg.py:138-150 rle_to_mask) ------------------------------------------------------------------------
// One block per record.  Runs alternate 0, 1, 0, ... over the column-major flattening f = x * H + y.  The block scans the counts
// 2048 at a time (8 per thread, wave scan, carry), then writes the 1-runs into the zero-filled mask: a short run by the thread
// that owns it, a long one by a whole wave.  Every store is clipped to f < H * W, so malformed counts cannot write outside the
// record's mask; status[n] = 1 when a count is negative or the counts do not sum to H * W (the binding raises on it).
#define RL_PT 8
#define RL_CH (256 * RL_PT)
#define RL_LONG 32
__global__ __launch_bounds__(256) void rle_expand_kernel(const int* __restrict__ counts, const long* __restrict__ offsets, int H, int W,
                                                         unsigned char* __restrict__ masks, int* __restrict__ status) {
    __shared__ long start[RL_CH + 1];
    __shared__ long wsum[4];
    __shared__ int bad_s;
    const long n = blockIdx.x;
    const long c0 = offsets[n], c1 = offsets[n + 1];
    const long per = (long)H * W;
    unsigned char* m = masks + n * per;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) bad_s = 0;
    long carry = 0;
    bool bad = false;
    for (long cb = c0; cb < c1; cb += RL_CH) {           // (RL_CH is even: a run's parity in the chunk is its parity in the record)
        long loc[RL_PT];
        long tsum = 0;
#pragma unroll
        for (int j = 0; j < RL_PT; ++j) {
            const long i = cb + threadIdx.x * RL_PT + j;
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
        for (int j = 0; j < RL_PT; ++j) start[threadIdx.x * RL_PT + j] = before + loc[j];
        if (threadIdx.x == 255) start[RL_CH] = before + tsum;
        __syncthreads();
        // short 1-runs: the owning thread
#pragma unroll
        for (int j = 1; j < RL_PT; j += 2) {
            const long f0 = before + loc[j];
            const long len = (j + 1 < RL_PT ? before + loc[j + 1] : before + tsum) - f0;
            if (len > 0 && len <= RL_LONG && f0 < per) {
                unsigned int f = (unsigned int)f0;
                const unsigned int fe = (unsigned int)min(f0 + len, per);
                unsigned int x = f / (unsigned int)H, y = f - x * (unsigned int)H;
                for (; f < fe; ++f) {
                    m[(long)y * W + x] = 1;
                    if (++y == (unsigned int)H) { y = 0; ++x; }
                }
            }
        }
        // long 1-runs: a wave each, lanes over consecutive f
        for (int r = 1 + 2 * wv; r < RL_CH; r += 8) {
            const long f0 = start[r];
            const long len = start[r + 1] - f0;
            if (len <= RL_LONG || f0 >= per) continue;   // wave-uniform
            const long fe = min(f0 + len, per);
            for (long f = f0 + lane; f < fe; f += 64) {
                const unsigned int x = (unsigned int)f / (unsigned int)H, y = (unsigned int)f - x * (unsigned int)H;
                m[(long)y * W + x] = 1;
            }
        }
        carry = start[RL_CH];
    }
    __syncthreads();
    if (bad || carry != per) bad_s = 1;                  // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) status[n] = bad_s;
}

// counts i32 [offsets[N]] (all records' uncompressed counts, concatenated); offsets i64 [N + 1]; masks u8 [N, H, W]; status i32 [N].
extern "C" int ullsam_rle_to_mask(const int* counts, const long* offsets, long N, int H, int W, unsigned char* masks, int* status,
                                  void* stream) {
    if (N == 0) return 0;
    ULLSAM_CHECK(N > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31), "rle_to_mask: need N >= 0, H, W > 0, H*W < 2^31");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(masks, 0, (size_t)N * H * W, s) != hipSuccess) { ullsam_set_error("rle_to_mask: memset failed"); return -2; }
    rle_expand_kernel<<<(unsigned)N, 256, 0, s>>>(counts, offsets, H, W, masks, status);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
