// The common layer of the label-image kernels (labels, regions, prompts, mosaic, stack, distance*, split*, measure*, outline, simplify, raster,
// mesh3d, skeleton): relaxed agent-scope atomics, the lock-free union-find over a global parent array, the wave and workgroup scans, the per-label LDS slot
// claim of the measurement kernels, and the host one-liners of the C ABI.  Integer work only.  pair_table.h builds the row runs and the pair table
// on top of this; a new label kernel takes its helpers from these two headers and defines none of them again.
#pragma once
#include "common.h"

typedef unsigned long long mz_u64;

// ---- relaxed agent-scope atomics ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mz_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ mz_u64 mz_load(const mz_u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_add(int* p, int v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_add(long* p, int v) { (void)__hip_atomic_fetch_add(p, (long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a 64-bit add into a table of any 64-bit integer type (two's complement: the sign of the element type does not matter)
template <class P> __device__ __forceinline__ void mz_add64(P* p, mz_u64 v) {
    static_assert(sizeof(P) == 8, "mz_add64 adds into 64-bit words");
    (void)__hip_atomic_fetch_add(reinterpret_cast<mz_u64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int mz_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_max(int* p, int v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_min(mz_u64* p, mz_u64 v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_max(mz_u64* p, mz_u64 v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_or(int* p, int bits) { (void)__hip_atomic_fetch_or(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The atomic is sent only when a relaxed load says it improves: a bound moves one way, so a stale load costs an atomic, never a result, and most
// arrivals at a busy address leave without one.
template <class T> __device__ __forceinline__ void mz_send_min(T* p, T v) { if (mz_load(p) > v) (void)mz_min(p, v); }
template <class T> __device__ __forceinline__ void mz_send_max(T* p, T v) { if (mz_load(p) < v) mz_max(p, v); }

// ---- union-find over a global parent array ------------------------------------------------------------------------------------------------
// L[i] <= i and a parent only ever decreases, so a component's root is its smallest member whatever the order of the unions.  Inside one launch
// every write is an agent-scope atomicMin and every read a relaxed load: a read may return an OLDER parent, which is an ancestor all the same.
__device__ __forceinline__ int mz_find(const int* L, int i) {
    int q = mz_load(L + i);
    while (q != i) { i = q; q = mz_load(L + i); }
    return i;
}
__device__ __forceinline__ void mz_union(int* L, int a, int b) {
    const int a0 = a, b0 = b;
    for (;;) {
        a = mz_find(L, a);
        b = mz_find(L, b);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = mz_min(L + a, b);                // a was a root when read: link it under the smaller root
        if (old == a) { a = b; break; }
        a = old;                                         // somebody linked a first: a ~ old still has to meet b
    }
    if (a < a0) mz_min(L + a0, a);                       // shorten the two chains: `a` is an ancestor of both, and a parent only moves down
    if (a < b0) mz_min(L + b0, a);
}

// ---- scans ------------------------------------------------------------------------------------------------------------------------------------
// the inclusive scan of v over the 64 lanes of a wave
template <class T> __device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
// the exclusive scan of v over the workgroup's BLOCK threads; total = the sum over all of them
template <int BLOCK, class T> __device__ __forceinline__ T block_exscan(T v, T& total) {
    __shared__ T s_wave[BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_scan_incl(v, lane);
    __syncthreads();                                      // (the table may still be read from an earlier call)
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; ++i) {
        const T t = s_wave[i];
        if (i < wave) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

// ---- ids and samples ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mz_in(long i, long n) { return i >= 0 && i < n; }                 // an index inside its table
__device__ __forceinline__ bool mz_live(int l, long K) { return l > 0 && l <= K; }                // an id of an instance (not background, not malformed)
__device__ __forceinline__ int mz_clean(int v, int K) { return (v < 0 || v > K) ? 0 : v; }        // an id outside 0..K reads as background
// the final label of local id l of a tile or plane with k ids whose global ids start after b0
__device__ __forceinline__ int mz_look(int l, int b0, int k, const int* __restrict__ log) { return (l > 0 && l <= k) ? log[b0 + l] : 0; }
// sample i of an image of 1- or 2-byte unsigned samples
__device__ __forceinline__ int mz_sample(const void* __restrict__ img, int bytes, long i) {
    return bytes == 1 ? (int)reinterpret_cast<const unsigned char*>(img)[i] : (int)reinterpret_cast<const unsigned short*>(img)[i];
}

// ---- the per-label table in LDS (measure.hip, measure3d.hip) ----------------------------------------------------------------------------------
// Open addressing keyed by label over skey [slots] (0 = free, slots a power of two or 0): the slot of `label`, claimed if need be, or -1 when
// PROBES probes find neither it nor a free slot (or slots == 0).  (The label by reference: by value measure_kernel allocates its registers
// differently around the compare-and-swap.)
template <int PROBES> __device__ __forceinline__ int mz_lds_slot(const int& label, int slots, int* skey) {
    int slot = -1;
    if (slots) {
        unsigned h = ((unsigned)label * 0x9E3779B1u) >> 16;
        for (int p = 0; p < PROBES && slot < 0; ++p, ++h) {
            int* kp = skey + (h & (unsigned)(slots - 1));
            int k = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (k == 0) {
                k = atomicCAS(kp, 0, label);
                if (k == 0) k = label;
            }
            if (k == label) slot = (int)(h & (unsigned)(slots - 1));
        }
    }
    return slot;
}

// ---- host one-liners ----------------------------------------------------------------------------------------------------------------------------
inline unsigned mz_blocks(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }
inline bool mz_zero(void* p, size_t bytes, hipStream_t s) { return bytes == 0 || hipMemsetAsync(p, 0, bytes, s) == hipSuccess; }
inline int isqrt_floor(long v) {                         // floor(sqrt(v)), 0 <= v < 2^31
    int r = 0;
    for (int bit = 1 << 15; bit; bit >>= 1)
        if ((long)(r + bit) * (r + bit) <= v) r += bit;
    return r;
}
