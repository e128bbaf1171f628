// Surface meshes and Euler numbers of a label VOLUME (host form and definition: utils/mesh3d.py; DESIGN.md "7b, continued (3-D surfaces)").  Integer
// work only -- integer atomics, no floating point anywhere -- so every output is a function of the inputs alone: bit-exact with the numpy definition
// and identical from run to run.
//
// volume i32 [Z, H, W] with ids 0..K (0 = background), 1 <= Z, H, W <= 32767 and Z * H * W <= 2^31 - 1.  Voxel p = (z H + y) W + x; its face towards
// d (0 = -z, 1 = +z, 2 = -y, 3 = +y, 4 = -x, 5 = +x) exists when the voxel has an id k > 0 and the neighbour there is not k (the volume's outside
// is not k) and has the id 6 p + d < 6 * 2^31 < 2^34; lattice corner (cx, cy, cz) has the id (cz (H + 1) + cy) (W + 1) + cx < 8 * 2^31 = 2^34.  A
// key is id | label << 34 with label <= 2^29 - 1, so it stays below 2^63 and sorts as a signed 64-bit number as well.
// mesh3d_mask_kernel.  One workgroup of 256 threads owns a tile of 64 x MS_TILE_Y x MS_TILE_Z voxels, a thread one (x, y) column of MS_TILE_Z voxels;
// it writes the six-bit face mask of every voxel and the tile's face count.  The six neighbours are read from global memory: a form that staged
// the tile and its one-voxel halo (66 x 6 x 6 ids) in LDS first was measured against this one and did not win (profiles/r26_mesh3d.txt), so it
// was taken out.  An id outside 0..K reads as background and sets flags[0]; as a neighbour it is "not k" for every valid k as it stands.
// mesh3d_scan_kernel.  ONE workgroup of 1024 threads: the exclusive prefix sums of n 32-bit counts in 64 bits, offsets[n] = the total.
// mesh3d_faces_kernel.  The mask kernel's grid: a block scan of the threads' face counts places each face key at the tile's offset (ordered
// compaction: where a key lands depends on the volume alone).  The keys are sorted by the caller.
// mesh3d_corners_kernel: the four corner keys of every face.  mesh3d_heads_kernel / mesh3d_vertices_kernel: over the SORTED corner keys, 2048 a
// workgroup, the first key of every run of equal keys is counted, then (after the scan) written with its (x, y, z).  mesh3d_quads_kernel: one
// thread per quad corner, a binary search of its key among the unique keys.  mesh3d_starts_kernel: one thread per id, a binary search for the end
// of its range of sorted keys.
// mesh3d_topology_kernel.  One wave per (z, y) row, 64 voxels at a time: a lane loads the nine ids at its x of the rows around it and takes x - 1
// and x + 1 by __shfl (one extra load at each end of the segment), giving the 27-bit word "this neighbour has my id".  The 26 lattice cells of a
// voxel (8 corners, 12 edges, 6 faces) are the choices of {0}, {-1, 0} or {0, 1} per axis; the voxel owns a cell when none of the voxels around the
// cell that come before it in raster order has its id, and adds +1 per corner and face, -1 per edge and -1 for itself: summed over the object that
// is V - E + F - C.  A pinch edge (k, not k, k, not k around it) is counted by the first of its two voxels of k.  A voxel whose 26 neighbours all
// have its id sums to 0 and sends nothing.
#include "label_common.h"

#define MS_TILE_X 64
#define MS_TILE_Y 4      // rows of a tile (ops.MESH3D_TILE_Y)
#define MS_TILE_Z 4      // planes of a tile (ops.MESH3D_TILE_Z)
#define MS_MAX_SIDE 32767
#define MS_KEY_SHIFT 34  // face ids and corner ids lie below 2^34
#define MS_MAX_LABEL 536870911   // 2^29 - 1: a key stays below 2^63
#define MS_ITEMS 8       // consecutive sorted keys per thread of the heads / vertices kernels: 2048 a workgroup
#define MS_ID_MASK ((1ull << MS_KEY_SHIFT) - 1)

typedef unsigned long long ms_u64;

// the corners of the quad towards d, counter-clockwise seen from outside: (dx | dy << 1 | dz << 2) of corner j at bit 3 j
#define MS_C(dx, dy, dz) ((dx) | (dy) << 1 | (dz) << 2)
#define MS_Q(a, b, c, d) (unsigned short)((a) | (b) << 3 | (c) << 6 | (d) << 9)
__constant__ unsigned short ms_quad[6] = {
    MS_Q(MS_C(0, 0, 0), MS_C(0, 1, 0), MS_C(1, 1, 0), MS_C(1, 0, 0)), MS_Q(MS_C(0, 0, 1), MS_C(1, 0, 1), MS_C(1, 1, 1), MS_C(0, 1, 1)),
    MS_Q(MS_C(0, 0, 0), MS_C(1, 0, 0), MS_C(1, 0, 1), MS_C(0, 0, 1)), MS_Q(MS_C(0, 1, 0), MS_C(0, 1, 1), MS_C(1, 1, 1), MS_C(1, 1, 0)),
    MS_Q(MS_C(0, 0, 0), MS_C(0, 0, 1), MS_C(0, 1, 1), MS_C(0, 1, 0)), MS_Q(MS_C(1, 0, 0), MS_C(1, 1, 0), MS_C(1, 1, 1), MS_C(1, 0, 1))};

// the key of corner j of the face with key fkey
__device__ __forceinline__ ms_u64 ms_corner_key(ms_u64 fkey, int j, int H, int W) {
    const ms_u64 id = fkey & MS_ID_MASK, p = id / 6;
    const int d = (int)(id - 6 * p);
    const ms_u64 x = p % (ms_u64)W, y = (p / (ms_u64)W) % (ms_u64)H, z = p / ((ms_u64)W * (ms_u64)H);
    const unsigned c = (ms_quad[d] >> (3 * j)) & 7u;
    const ms_u64 cx = x + (c & 1u), cy = y + ((c >> 1) & 1u), cz = z + ((c >> 2) & 1u);
    return (fkey & ~MS_ID_MASK) | ((cz * (ms_u64)(H + 1) + cy) * (ms_u64)(W + 1) + cx);
}

// ---- faces --------------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), ceil(H / MS_TILE_Y), ceil(Z / MS_TILE_Z)), block 256; tile t = (blockIdx.z gridDim.y + blockIdx.y) gridDim.x + blockIdx.x
__global__ __launch_bounds__(256) void mesh3d_mask_kernel(const int* __restrict__ vol, int Z, int H, int W, int K, const unsigned char* __restrict__ sel,
                                                          unsigned char* __restrict__ masks, int* __restrict__ tile_counts, int* __restrict__ flags) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int x0 = blockIdx.x * MS_TILE_X, y0 = blockIdx.y * MS_TILE_Y, z0 = blockIdx.z * MS_TILE_Z;
    const long plane = (long)H * W;
    const int x = x0 + tx, y = y0 + ty;
    int n = 0;
    bool bad = false;
    if (x < W && y < H) {
#pragma unroll
        for (int dz = 0; dz < MS_TILE_Z; ++dz) {
            const int z = z0 + dz;
            if (z >= Z) break;
            const long p = z * plane + (long)y * W + x;
            int l = vol[p], nb[6];
            nb[0] = z > 0 ? vol[p - plane] : -1; nb[1] = z + 1 < Z ? vol[p + plane] : -1;
            nb[2] = y > 0 ? vol[p - W] : -1; nb[3] = y + 1 < H ? vol[p + W] : -1;
            nb[4] = x > 0 ? vol[p - 1] : -1; nb[5] = x + 1 < W ? vol[p + 1] : -1;
            if (l < 0 || l > K) { bad = true; l = 0; }
            int m = 0;
            if (l > 0 && (sel == nullptr || sel[l])) {
#pragma unroll
                for (int d = 0; d < 6; ++d) m |= (nb[d] != l ? 1 : 0) << d;
            }
            masks[p] = (unsigned char)m;
            n += __popc((unsigned)m);
        }
    }
    if (bad) mz_store(flags + 0, 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (tx == 0) wsum[ty] = n;
    __syncthreads();
    if (tid == 0) tile_counts[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// grid 1, block 1024
__global__ __launch_bounds__(1024) void mesh3d_scan_kernel(const int* __restrict__ counts, long n, long* __restrict__ offsets) {
    __shared__ ms_u64 wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ms_u64 carry = 0;
    for (long base = 0; base < n; base += 1024) {
        const long i = base + tid;
        const ms_u64 v = i < n ? (ms_u64)counts[i] : 0;
        ms_u64 inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const ms_u64 t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        ms_u64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const ms_u64 t = wtot[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < n) offsets[i] = (long)(carry + before + inc - v);
        carry += total;
        __syncthreads();
    }
    if (tid == 0) offsets[n] = (long)carry;
}

// the mask kernel's grid; F = the length of fkeys (the total of the scan): nothing is written past it
__global__ __launch_bounds__(256) void mesh3d_faces_kernel(const int* __restrict__ vol, const unsigned char* __restrict__ masks, int Z, int H, int W,
                                                           const long* __restrict__ tile_offsets, ms_u64* __restrict__ fkeys, long F) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int x = blockIdx.x * MS_TILE_X + tx, y = blockIdx.y * MS_TILE_Y + ty, z0 = blockIdx.z * MS_TILE_Z;
    const long plane = (long)H * W;
    int m[MS_TILE_Z], n = 0;
#pragma unroll
    for (int dz = 0; dz < MS_TILE_Z; ++dz) {
        m[dz] = (x < W && y < H && z0 + dz < Z) ? (int)masks[(z0 + dz) * plane + (long)y * W + x] : 0;
        n += __popc((unsigned)m[dz]);
    }
    const int inc = wave_scan_incl(n, tx);
    if (tx == 63) wsum[ty] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < ty; ++w) before += wsum[w];
    long at = tile_offsets[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] + before + inc - n;
#pragma unroll
    for (int dz = 0; dz < MS_TILE_Z; ++dz) {
        if (!m[dz]) continue;
        const long p = (z0 + dz) * plane + (long)y * W + x;
        const ms_u64 key = ((ms_u64)vol[p] << MS_KEY_SHIFT) | (6ull * (ms_u64)p);
#pragma unroll
        for (int d = 0; d < 6; ++d)
            if ((m[dz] >> d) & 1) {
                if (at < F) fkeys[at] = key + d;
                ++at;
            }
    }
}

// ---- vertices -----------------------------------------------------------------------------------------------------------------------------------
// one thread per face: ckeys u64 [4 F]
__global__ __launch_bounds__(256) void mesh3d_corners_kernel(const ms_u64* __restrict__ fkeys, long F, int H, int W, ms_u64* __restrict__ ckeys) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const ms_u64 key = fkeys[f];
#pragma unroll
    for (int j = 0; j < 4; ++j) ckeys[4 * f + j] = ms_corner_key(key, j, H, W);
}

// sorted u64 [n]; workgroup b takes the keys 2048 b .. 2048 b + 2047, a thread MS_ITEMS consecutive ones.  WRITE = false: block_counts[b] = the
// keys that differ from their predecessor; WRITE = true: those keys to ukeys at block_offsets[b] + their rank, with their corner in vertices.
template <bool WRITE>
__global__ __launch_bounds__(256) void mesh3d_heads_kernel(const ms_u64* __restrict__ sorted, long n, int* __restrict__ block_counts,
                                                           const long* __restrict__ block_offsets, int H, int W, ms_u64* __restrict__ ukeys,
                                                           int* __restrict__ vertices, long V) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long first = ((long)blockIdx.x * 256 + tid) * MS_ITEMS;
    ms_u64 key[MS_ITEMS];
    ms_u64 prev = first > 0 && first <= n ? sorted[first - 1] : 0;
    unsigned heads = 0;
#pragma unroll
    for (int j = 0; j < MS_ITEMS; ++j) {
        key[j] = first + j < n ? sorted[first + j] : 0;
        if (first + j < n && (first + j == 0 || key[j] != prev)) heads |= 1u << j;
        prev = key[j];
    }
    const int cnt = __popc(heads);
    if (!WRITE) {
        int s = cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) wsum[wave] = s;
        __syncthreads();
        if (tid == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    } else {
        const int inc = wave_scan_incl(cnt, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        long at = block_offsets[blockIdx.x] + before + inc - cnt;
        const ms_u64 w1 = (ms_u64)(W + 1), h1 = (ms_u64)(H + 1);
#pragma unroll
        for (int j = 0; j < MS_ITEMS; ++j)
            if ((heads >> j) & 1u) {
                if (at < V) {
                    const ms_u64 c = key[j] & MS_ID_MASK;
                    ukeys[at] = key[j];
                    vertices[3 * at + 0] = (int)(c % w1);
                    vertices[3 * at + 1] = (int)((c / w1) % h1);
                    vertices[3 * at + 2] = (int)(c / (w1 * h1));
                }
                ++at;
            }
    }
}

// one thread per quad corner: quads i32 [F, 4] = the index of the corner's key among the V unique keys
__global__ __launch_bounds__(256) void mesh3d_quads_kernel(const ms_u64* __restrict__ fkeys, long F, const ms_u64* __restrict__ ukeys, long V, int H, int W,
                                                           int* __restrict__ quads) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 4 * F) return;
    const ms_u64 key = ms_corner_key(fkeys[t >> 2], (int)(t & 3), H, W);
    long lo = 0, hi = V;                                 // the first index with ukeys[index] >= key
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (ukeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    quads[t] = lo < V ? (int)lo : -1;
}

// one thread per id k = 0..K: start[k] = the number of sorted keys whose label is <= k
__global__ __launch_bounds__(256) void mesh3d_starts_kernel(const ms_u64* __restrict__ sorted, long n, int K, long* __restrict__ start) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if ((long)(sorted[mid] >> MS_KEY_SHIFT) <= k) lo = mid + 1;
        else hi = mid;
    }
    start[k] = lo;
}

// ---- topology -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh3d_init_kernel(long K, long* __restrict__ euler, long* __restrict__ pinch, int* __restrict__ flags) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k < 4) flags[k] = 0;
    if (k >= K) return;
    euler[k] = 0;
    pinch[k] = 0;
}

// neighbour (oz, oy, ox) in -1..1 sits at bit (oz + 1) 9 + (oy + 1) 3 + (ox + 1); the voxel itself at bit 13, the voxels before it in raster order below
constexpr int ms_bit(int oz, int oy, int ox) { return (oz + 1) * 9 + (oy + 1) * 3 + (ox + 1); }
// per axis a = 0: the cell spans {0}, 1: {-1, 0}, 2: {0, 1}.  The voxels around the cell that come before the voxel in raster order.
constexpr unsigned ms_cell_before(int az, int ay, int ax) {
    unsigned m = 0;
    for (int oz = -1; oz <= 1; ++oz)
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const bool in_z = az == 0 ? oz == 0 : az == 1 ? oz <= 0 : oz >= 0;
                const bool in_y = ay == 0 ? oy == 0 : ay == 1 ? oy <= 0 : oy >= 0;
                const bool in_x = ax == 0 ? ox == 0 : ax == 1 ? ox <= 0 : ox >= 0;
                if (in_z && in_y && in_x && ms_bit(oz, oy, ox) < 13) m |= 1u << ms_bit(oz, oy, ox);
            }
    return m;
}
template <int AZ, int AY, int AX> __device__ __forceinline__ int ms_cell(unsigned same) {
    constexpr unsigned before = ms_cell_before(AZ, AY, AX);
    constexpr int sign = (((AZ == 0) + (AY == 0) + (AX == 0)) & 1) ? -1 : 1;     // corners and faces +1, edges and the voxel -1
    return (same & before) == 0 ? sign : 0;
}
template <int AZ, int AY> __device__ __forceinline__ int ms_cells_x(unsigned same) {
    return ms_cell<AZ, AY, 0>(same) + ms_cell<AZ, AY, 1>(same) + ms_cell<AZ, AY, 2>(same);
}
template <int AZ> __device__ __forceinline__ int ms_cells_y(unsigned same) {
    return ms_cells_x<AZ, 0>(same) + ms_cells_x<AZ, 1>(same) + ms_cells_x<AZ, 2>(same);
}
// the pinch edge between the voxel and its diagonal neighbour D, with the two voxels A and B beside the edge
template <int D, int A, int B> __device__ __forceinline__ int ms_pinch(unsigned same) {
    return ((same >> D) & 1u) && !((same >> A) & 1u) && !((same >> B) & 1u) ? 1 : 0;
}

// grid ceil(Z * H / 4), block 256: one wave per (z, y) row
__global__ __launch_bounds__(256) void mesh3d_topology_kernel(const int* __restrict__ vol, int Z, int H, int W, int K, long* __restrict__ euler,
                                                              long* __restrict__ pinch, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long line = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= (long)Z * H) return;                     // wave-uniform
    const int z = (int)(line / H), y = (int)(line % H);
    const long plane = (long)H * W;
    bool bad = false;
    for (int xs = 0; xs < W; xs += 64) {
        const int x = xs + lane;
        int l = x < W ? vol[line * W + x] : 0;
        if (l < 0 || l > K) { bad = true; l = 0; }
        if (__ballot(l > 0) == 0ull) continue;           // wave-uniform: nothing labelled in this segment
        unsigned same = 0;
#pragma unroll
        for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
            for (int oy = -1; oy <= 1; ++oy) {
                const bool row_in = z + oz >= 0 && z + oz < Z && y + oy >= 0 && y + oy < H;   // wave-uniform
                const long row = ((long)(z + oz) * H + (y + oy)) * W;
                const int v = row_in && x < W ? vol[row + x] : -1;
                int lf = __shfl_up(v, 1, 64), rt = __shfl_down(v, 1, 64);
                if (lane == 0) lf = row_in && xs > 0 ? vol[row + xs - 1] : -1;
                if (lane == 63) rt = row_in && xs + 64 < W ? vol[row + xs + 64] : -1;
                same |= (unsigned)(lf == l) << ms_bit(oz, oy, -1) | (unsigned)(v == l) << ms_bit(oz, oy, 0) | (unsigned)(rt == l) << ms_bit(oz, oy, 1);
            }
        if (l <= 0) continue;                            // (after the shuffles: every lane takes part in them)
        const int e = ms_cells_y<0>(same) + ms_cells_y<1>(same) + ms_cells_y<2>(same);
        const int q = ms_pinch<ms_bit(0, 1, 1), ms_bit(0, 1, 0), ms_bit(0, 0, 1)>(same) + ms_pinch<ms_bit(0, 1, -1), ms_bit(0, 1, 0), ms_bit(0, 0, -1)>(same) +
                      ms_pinch<ms_bit(1, 0, 1), ms_bit(1, 0, 0), ms_bit(0, 0, 1)>(same) + ms_pinch<ms_bit(1, 0, -1), ms_bit(1, 0, 0), ms_bit(0, 0, -1)>(same) +
                      ms_pinch<ms_bit(1, 1, 0), ms_bit(1, 0, 0), ms_bit(0, 1, 0)>(same) + ms_pinch<ms_bit(1, -1, 0), ms_bit(1, 0, 0), ms_bit(0, -1, 0)>(same);
        if (e) mz_add64(euler + (l - 1), (ms_u64)(long)e);
        if (q) mz_add64(pinch + (l - 1), (ms_u64)q);
    }
    if (bad) mz_store(flags + 0, 1);
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------------
#define MS_VOLUME_CHECK(what) \
    ULLSAM_CHECK(Z >= 1 && H >= 1 && W >= 1 && Z <= MS_MAX_SIDE && H <= MS_MAX_SIDE && W <= MS_MAX_SIDE && (long)Z * H * W <= 2147483647L, \
                 what ": need 1 <= Z, H, W <= 32767 and Z * H * W <= 2^31 - 1")
#define MS_GRID(Z, H, W) dim3((unsigned)((W + MS_TILE_X - 1) / MS_TILE_X), (unsigned)((H + MS_TILE_Y - 1) / MS_TILE_Y), (unsigned)((Z + MS_TILE_Z - 1) / MS_TILE_Z))

extern "C" int ullsam_mesh3d_masks(const int* volume, int Z, int H, int W, int K, const unsigned char* only, unsigned char* masks,
                                   int* tile_counts, long* tile_offsets, int* flags, void* stream) {
    MS_VOLUME_CHECK("mesh3d_masks");
    ULLSAM_CHECK(K >= 0 && K <= MS_MAX_LABEL, "mesh3d_masks: need 0 <= K <= 2^29 - 1");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    mesh3d_init_kernel<<<1, 256, 0, s>>>(0, nullptr, nullptr, flags);
    ULLSAM_LAUNCH_CHECK();
    const dim3 grid = MS_GRID(Z, H, W);
    mesh3d_mask_kernel<<<grid, 256, 0, s>>>(volume, Z, H, W, K, only, masks, tile_counts, flags);
    ULLSAM_LAUNCH_CHECK();
    mesh3d_scan_kernel<<<1, 1024, 0, s>>>(tile_counts, (long)grid.x * grid.y * grid.z, tile_offsets);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_faces(const int* volume, const unsigned char* masks, int Z, int H, int W, const long* tile_offsets, unsigned long long* fkeys,
                                   long F, void* stream) {
    MS_VOLUME_CHECK("mesh3d_faces");
    ULLSAM_CHECK(F >= 0 && F <= 2147483647L, "mesh3d_faces: need 0 <= F <= 2^31 - 1");
    mesh3d_faces_kernel<<<MS_GRID(Z, H, W), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(volume, masks, Z, H, W, tile_offsets, fkeys, F);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_corners(const unsigned long long* fkeys, long F, int H, int W, unsigned long long* ckeys, void* stream) {
    ULLSAM_CHECK(F >= 0 && F <= 2147483647L && H >= 1 && W >= 1 && H <= MS_MAX_SIDE && W <= MS_MAX_SIDE, "mesh3d_corners: need 0 <= F <= 2^31 - 1 and 1 <= H, W <= 32767");
    if (F == 0) return 0;
    mesh3d_corners_kernel<<<mz_blocks(F), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(fkeys, F, H, W, ckeys);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_heads(const unsigned long long* sorted, long n, int* block_counts, long* block_offsets, void* stream) {
    ULLSAM_CHECK(n >= 0 && n <= 4 * 2147483647L, "mesh3d_heads: need 0 <= n <= 4 (2^31 - 1)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long blocks = (n + 256 * MS_ITEMS - 1) / (256 * MS_ITEMS);
    if (blocks) {
        mesh3d_heads_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(sorted, n, block_counts, nullptr, 1, 1, nullptr, nullptr, 0);
        ULLSAM_LAUNCH_CHECK();
    }
    mesh3d_scan_kernel<<<1, 1024, 0, s>>>(block_counts, blocks, block_offsets);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_vertices(const unsigned long long* sorted, long n, const long* block_offsets, int H, int W, unsigned long long* ukeys,
                                      int* vertices, long V, void* stream) {
    ULLSAM_CHECK(n >= 0 && n <= 4 * 2147483647L && V >= 0 && V <= n && V <= 2147483647L && H >= 1 && W >= 1 && H <= MS_MAX_SIDE && W <= MS_MAX_SIDE,
                 "mesh3d_vertices: need 0 <= V <= n <= 4 (2^31 - 1), V <= 2^31 - 1 and 1 <= H, W <= 32767");
    const long blocks = (n + 256 * MS_ITEMS - 1) / (256 * MS_ITEMS);
    if (blocks == 0) return 0;
    mesh3d_heads_kernel<true><<<(unsigned)blocks, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(sorted, n, nullptr, block_offsets, H, W, ukeys, vertices, V);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_quads(const unsigned long long* fkeys, long F, const unsigned long long* ukeys, long V, int H, int W, int* quads, void* stream) {
    ULLSAM_CHECK(F >= 0 && F <= 2147483647L && V >= 0 && V <= 2147483647L && H >= 1 && W >= 1 && H <= MS_MAX_SIDE && W <= MS_MAX_SIDE,
                 "mesh3d_quads: need 0 <= F, V <= 2^31 - 1 and 1 <= H, W <= 32767");
    if (F == 0) return 0;
    mesh3d_quads_kernel<<<mz_blocks(4 * F), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(fkeys, F, ukeys, V, H, W, quads);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_starts(const unsigned long long* sorted, long n, int K, long* start, void* stream) {
    ULLSAM_CHECK(n >= 0 && K >= 0 && K <= MS_MAX_LABEL, "mesh3d_starts: need n >= 0 and 0 <= K <= 2^29 - 1");
    mesh3d_starts_kernel<<<(unsigned)(((long)K + 256) / 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(sorted, n, K, start);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_mesh3d_topology(const int* volume, int Z, int H, int W, int K, long* euler, long* pinch_edges, int* flags, void* stream) {
    MS_VOLUME_CHECK("mesh3d_topology");
    ULLSAM_CHECK(K >= 0 && K <= 2147483646, "mesh3d_topology: need 0 <= K <= 2^31 - 2");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    mesh3d_init_kernel<<<(unsigned)(((long)K + 255) / 256 + 1), 256, 0, s>>>(K, euler, pinch_edges, flags);
    ULLSAM_LAUNCH_CHECK();
    mesh3d_topology_kernel<<<(unsigned)(((long)Z * H + 3) / 4), 256, 0, s>>>(volume, Z, H, W, K, euler, pinch_edges, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
