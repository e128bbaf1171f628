// Splitting the touching objects of an instance label VOLUME: split.hip's flood-free watershed with a third axis (host form and definition:
// utils/split3d.py; DESIGN.md "7b, continued (3-D splitting)").  Only the stages that know the volume's shape live here -- the ascent over the 26
// neighbours, the pass table over the 13 forward neighbours, the tables and the relabel with (x, y, z) peaks; flatten, the round (best + decide)
// and collect are split.hip's flat entry points, called on the flattened volume.  Integer work only, ordinary vector stores, integer atomics,
// and every choice is a maximum under a strict total order: every output is a function of the volume alone.
//
// D2 = inner_distance3d(volume, spacing, edge) (distance3d.hip), p = (z * H + y) * W + x, key(p) = (D2[p], -p).  n = Z * H * W <= 32767^2 < 2^30
// (the bound of the flat entry points), so p and every neighbour index p +- (H W + W + 1) stay inside int32.
//   ascent   up[p] = the voxel of greatest key among p and its 26 neighbours with p's label (p itself on the background).  A workgroup of
//            S3_BLOCK threads covers S3_TX x S3_TY x S3_TZ voxels, one (x, y) column of S3_TZ voxels per thread; it either stages the tile with a
//            one-voxel halo in LDS (voxels outside the volume enter as label 0, which is never live) or reads global memory.
//   passes   every voxel looks at its 13 forward neighbours -- (dz, dy, dx) > (0, 0, 0) in that order of significance --, so every 26-adjacent
//            pair is met once; where the neighbour has its label and another root, min(D2, D2) goes into the pair table under
//            (smaller root << 32 | larger root) with a maximum per key (pair_table.h mz_pair_max): split_passes' table, slot for slot.  The
//            ascent's tile, staged in LDS with the forward halo; a thread sends the running maximum of its last key, not every voxel pair.
//   relabel  part i of the sorted list gets id i + 1: parent, peak_r2, peak_xyz = (p % W, (p / W) % H, p / (W H)), parts_of; every voxel takes
//            the id of its root.
// flags i32 [8] as in split.hip: [0] = a label below 0 or above K, or a list entry outside the volume (skipped; nothing is indexed with it),
// [1] = a pair was refused, [2] = the pairs claimed; [3], [4], [5] belong to flatten and collect.
#include "pair_table.h"
#include <stdint.h>

#define S3_TX 64
#define S3_TY 4
#define S3_TZ 4
#define S3_BLOCK (S3_TX * S3_TY)

// ---- ascent ---------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(W / S3_TX), ceil(H / S3_TY), ceil(Z / S3_TZ)), block S3_BLOCK
template <bool LDS>
__global__ __launch_bounds__(S3_BLOCK) void split3_ascent_kernel(const int* __restrict__ labels, const int* __restrict__ d2, int Z, int H, int W, long K,
                                                                 int* __restrict__ up, int* __restrict__ flags) {
    constexpr int LW = S3_TX + 2, LH = S3_TY + 2, LZ = S3_TZ + 2;
    __shared__ int s_lab[LDS ? LZ * LH * LW : 1];
    __shared__ int s_d2[LDS ? LZ * LH * LW : 1];
    const int x0 = blockIdx.x * S3_TX, y0 = blockIdx.y * S3_TY, z0 = blockIdx.z * S3_TZ;
    const int HW = H * W;                                 // H W <= n < 2^30
    if (LDS) {
        for (int i = threadIdx.x; i < LZ * LH * LW; i += S3_BLOCK) {
            const int gz = z0 - 1 + i / (LH * LW), gy = y0 - 1 + (i / LW) % LH, gx = x0 - 1 + i % LW;
            const bool in = gz >= 0 && gz < Z && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int q = in ? gz * HW + gy * W + gx : 0;
            s_lab[i] = in ? labels[q] : 0;                // (0 is no live label: the volume's outside never matches)
            s_d2[i] = in ? d2[q] : 0;
        }
        __syncthreads();
    }
    const int lx = threadIdx.x % S3_TX, ly = threadIdx.x / S3_TX;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
#pragma unroll
    for (int lz = 0; lz < S3_TZ; ++lz) {
        const int z = z0 + lz;
        if (z >= Z) break;
        const int p = z * HW + y * W + x;
        const int c = ((lz + 1) * LH + (ly + 1)) * LW + (lx + 1);
        const int l = LDS ? s_lab[c] : labels[p];
        if (!mz_live(l, K)) {
            if (l != 0) mz_store(flags + 0, 1);
            up[p] = p;
            continue;
        }
        int bd = LDS ? s_d2[c] : d2[p], bq = p;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx == 0 && dy == 0 && dz == 0) continue;
                    const int q = p + dz * HW + dy * W + dx;
                    int nl, nd;
                    if (LDS) {
                        const int i = ((lz + 1 + dz) * LH + (ly + 1 + dy)) * LW + (lx + 1 + dx);
                        nl = s_lab[i];
                        nd = s_d2[i];
                    } else {
                        const int zz = z + dz, yy = y + dy, xx = x + dx;
                        if (zz < 0 || zz >= Z || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                        nl = labels[q];
                        nd = d2[q];
                    }
                    if (nl == l && (nd > bd || (nd == bd && q < bq))) {
                        bd = nd;
                        bq = q;
                    }
                }
            }
        }
        up[p] = bq;
    }
}

// ---- passes ---------------------------------------------------------------------------------------------------------------------------------
// grid and block of the ascent; up is flattened.  The tile's labels, roots and D2 are staged in LDS with the halo the forward offsets reach: one plane
// above, one row and one column on either side (outside the volume: label 0).  26 global reads a voxel become 3 x 1.9.
__global__ __launch_bounds__(S3_BLOCK) void split3_passes_kernel(const int* __restrict__ labels, const int* __restrict__ d2, const int* __restrict__ up,
                                                                 int Z, int H, int W, long K, mz_u64* __restrict__ keys, int* __restrict__ vals, mz_u64 mask,
                                                                 int max_pairs, int* __restrict__ flags) {
    constexpr int LW = S3_TX + 2, LH = S3_TY + 2, LZ = S3_TZ + 1;
    __shared__ int s_lab[LZ * LH * LW];
    __shared__ int s_up[LZ * LH * LW];
    __shared__ int s_d2[LZ * LH * LW];
    const int x0 = blockIdx.x * S3_TX, y0 = blockIdx.y * S3_TY, z0 = blockIdx.z * S3_TZ;
    const int HW = H * W;
    for (int i = threadIdx.x; i < LZ * LH * LW; i += S3_BLOCK) {
        const int gz = z0 + i / (LH * LW), gy = y0 - 1 + (i / LW) % LH, gx = x0 - 1 + i % LW;
        const bool in = gz < Z && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int q = in ? gz * HW + gy * W + gx : 0;
        s_lab[i] = in ? labels[q] : 0;
        s_up[i] = in ? up[q] : 0;
        s_d2[i] = in ? d2[q] : 0;
    }
    __syncthreads();
    const int lx = threadIdx.x % S3_TX, ly = threadIdx.x / S3_TX;
    if (x0 + lx >= W || y0 + ly >= H) return;
    // A thread's 4 x 13 voxel pairs mostly cross one border between the same two basins: the running maximum of the last key stays in registers and
    // goes to the table when the key changes (a maximum per key: the table does not depend on how the sends are grouped).
    mz_u64 held = 0;
    int held_v = 0;
#pragma unroll
    for (int lz = 0; lz < S3_TZ; ++lz) {
        if (z0 + lz >= Z) break;
        const int c = (lz * LH + (ly + 1)) * LW + (lx + 1);
        const int l = s_lab[c];
        if (!mz_live(l, K)) continue;
        const int dp = s_d2[c];
        const unsigned rp = (unsigned)s_up[c];
#pragma unroll
        for (int j = 0; j < 13; ++j) {
            // (0, 0, 1); (0, 1, -1..1); (1, -1..1, -1..1)
            const int dz = j >= 4 ? 1 : 0, dy = j >= 4 ? (j - 4) / 3 - 1 : (j >= 1 ? 1 : 0), dx = j >= 4 ? (j - 4) % 3 - 1 : (j >= 1 ? j - 2 : 1);
            const int i = c + (dz * LH + dy) * LW + dx;
            if (s_lab[i] != l) continue;                  // (the volume's outside is label 0, never l)
            const unsigned rq = (unsigned)s_up[i];
            if (rq == rp) continue;
            const mz_u64 key = ((mz_u64)min(rp, rq) << 32) | (mz_u64)max(rp, rq);
            const int v = min(dp, s_d2[i]);
            if (key == held) held_v = max(held_v, v);
            else {
                if (held) mz_pair_max(held, held_v, keys, vals, mask, max_pairs, flags);
                held = key;
                held_v = v;
            }
        }
    }
    if (held) mz_pair_max(held, held_v, keys, vals, mask, max_pairs, flags);
}

// ---- numbering ------------------------------------------------------------------------------------------------------------------------------
// one thread per part of the sorted list
__global__ __launch_bounds__(256) void split3_tables_kernel(const mz_u64* __restrict__ list, long parts, const int* __restrict__ d2, long n, int H, int W,
                                                            long K, int* __restrict__ newid, int* __restrict__ parent, int* __restrict__ peak_r2,
                                                            int* __restrict__ peak_xyz, int* __restrict__ parts_of, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= parts) return;
    const mz_u64 k = list[i];
    const long l = (long)(k >> 32), p = (long)(k & 0xffffffffull);
    parent[i] = 0;
    peak_r2[i] = 0;
    peak_xyz[3 * i + 0] = -1;
    peak_xyz[3 * i + 1] = -1;
    peak_xyz[3 * i + 2] = -1;
    if (l < 1 || l > K || p >= n) {                       // (a hand-made list)
        mz_store(flags + 0, 1);
        return;
    }
    parent[i] = (int)l;
    peak_r2[i] = d2[p];
    peak_xyz[3 * i + 0] = (int)(p % W);
    peak_xyz[3 * i + 1] = (int)((p / W) % H);
    peak_xyz[3 * i + 2] = (int)(p / ((long)W * H));
    newid[p] = (int)(i + 1);
    mz_add(parts_of + (l - 1), 1);
}
// one thread per voxel: the id of its root (newid is written at the representatives only, and read there only)
__global__ __launch_bounds__(256) void split3_relabel_kernel(const int* __restrict__ labels, const int* __restrict__ up, const int* __restrict__ newid, long n,
                                                             long K, int* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int v = 0;
    if (mz_live(labels[p], K)) {
        const int r = up[p];
        if (r >= 0 && r < n) v = newid[r];
    }
    out[p] = v;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
#define S3_VOLUME_CHECK(what)                                                                                                                    \
    ULLSAM_CHECK(Z >= 1 && Z <= 32767 && H >= 1 && H <= 32767 && W >= 1 && W <= 32767 && (long)Z * H * W <= 32767L * 32767L && K >= 0 && K <= 2147483647L, \
                 what ": need 1 <= Z, H, W <= 32767, Z * H * W <= 32767^2 and 0 <= K <= 2^31 - 1")

extern "C" int ullsam_split3d_ascent(const int* labels, const int* d2, int Z, int H, int W, long K, int route, int* up, int* flags, void* stream) {
    S3_VOLUME_CHECK("split3d_ascent");
    ULLSAM_CHECK(route >= 0 && route <= 2, "split3d_ascent: route in 0..2");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((W + S3_TX - 1) / S3_TX), (unsigned)((H + S3_TY - 1) / S3_TY), (unsigned)((Z + S3_TZ - 1) / S3_TZ));
    if (route != 2) split3_ascent_kernel<true><<<grid, S3_BLOCK, 0, s>>>(labels, d2, Z, H, W, K, up, flags);
    else split3_ascent_kernel<false><<<grid, S3_BLOCK, 0, s>>>(labels, d2, Z, H, W, K, up, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split3d_passes(const int* labels, const int* d2, const int* up, int Z, int H, int W, long K, unsigned long long* keys, int* vals,
                                     long cap, int max_pairs, int* flags, void* stream) {
    S3_VOLUME_CHECK("split3d_passes");
    ULLSAM_CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && max_pairs >= 1 && 2L * max_pairs <= cap, "split3d_passes: cap must be a power of two >= 2 * max_pairs");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!mz_zero(keys, (size_t)cap * 8, s) || !mz_zero(vals, (size_t)cap * 4, s)) {
        ullsam_set_error("split3d_passes: memset failed");
        return -2;
    }
    const dim3 grid((unsigned)((W + S3_TX - 1) / S3_TX), (unsigned)((H + S3_TY - 1) / S3_TY), (unsigned)((Z + S3_TZ - 1) / S3_TZ));
    split3_passes_kernel<<<grid, S3_BLOCK, 0, s>>>(labels, d2, up, Z, H, W, K, reinterpret_cast<mz_u64*>(keys), vals, (mz_u64)(cap - 1), max_pairs, flags);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_split3d_relabel(const unsigned long long* list, long parts, const int* labels, const int* d2, const int* up, int Z, int H, int W,
                                      long K, int* newid, int* out, int* parent, int* peak_r2, int* peak_xyz, int* parts_of, int* flags, void* stream) {
    S3_VOLUME_CHECK("split3d_relabel");
    const long n = (long)Z * H * W;
    ULLSAM_CHECK(parts >= 0 && parts <= n && K <= 2147483646L, "split3d_relabel: need 0 <= parts <= Z * H * W and K <= 2^31 - 2");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!mz_zero(parts_of, (size_t)K * 4, s)) {
        ullsam_set_error("split3d_relabel: memset failed");
        return -2;
    }
    const unsigned blocks = mz_blocks(n);
    if (parts > 0) {
        split3_tables_kernel<<<mz_blocks(parts), 256, 0, s>>>(reinterpret_cast<const mz_u64*>(list), parts, d2, n, H, W, K, newid, parent, peak_r2,
                                                                             peak_xyz, parts_of, flags);
        ULLSAM_LAUNCH_CHECK();
    }
    split3_relabel_kernel<<<blocks, 256, 0, s>>>(labels, up, newid, n, K, out);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
