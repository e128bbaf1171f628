// Shared by mosaic.hip (label pairs across tile seams) and measure.hip (label pairs across pixel sides): runs of equal keys along a row and the
// open-addressing pair table in global memory.  Integer work only; what the table holds at the end does not depend on the order of arrival.
#pragma once
#include "common.h"

typedef unsigned long long mz_u64;

__device__ __forceinline__ int mz_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_add(int* p, int v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_add(long* p, int v) { (void)__hip_atomic_fetch_add(p, (long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int mz_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mz_max(int* p, int v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- runs of equal keys along a row ---------------------------------------------------------------------------------------------
// Wave-uniform: a run of whole 64-pixel segments that has not been sent yet (key 0: none).
struct MzRun {
    mz_u64 key;
    int x0, cnt;
};
// One 64-pixel segment starting at column xs; k = the lane's key (0: nothing to count).  emit(key, first column, length) is called by one lane per run.
template <class F> __device__ __forceinline__ void mz_segment(MzRun& c, mz_u64 k, int xs, int lane, F emit) {
    const mz_u64 prev = __shfl_up(k, 1, 64);
    const bool head = lane == 0 || k != prev;
    const mz_u64 hm = __ballot(head);
    if (hm == 1ull) {                                    // one key over the whole segment
        const mz_u64 k0 = __shfl(k, 0, 64);
        if (k0 == c.key) c.cnt += 64;
        else {
            if (c.key && lane == 0) emit(c.key, c.x0, c.cnt);
            c.key = k0;
            c.x0 = xs;
            c.cnt = 64;
        }
    } else {
        if (c.key && lane == 0) emit(c.key, c.x0, c.cnt);
        c.key = 0;
        c.cnt = 0;
        if (head && k) {
            const mz_u64 rest = (hm >> lane) >> 1;       // heads above this lane
            emit(k, xs + lane, rest ? __builtin_ctzll(rest) + 1 : 64 - lane);
        }
    }
}
template <class F> __device__ __forceinline__ void mz_flush(MzRun& c, int lane, F emit) {
    if (c.key && lane == 0) emit(c.key, c.x0, c.cnt);
    c.key = 0;
    c.cnt = 0;
}

// ---- the pair table -------------------------------------------------------------------------------------------------------------
// keys u64 [mask + 1] (0 = empty slot), counts i32 or i64 [mask + 1]; flags[1] = 1 when a key was refused, flags[2] = the number of claimed slots.
__device__ __forceinline__ mz_u64 mz_hash(mz_u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return k;
}
template <class CT>
__device__ __forceinline__ void mz_pair_add(mz_u64 key, int n, mz_u64* __restrict__ keys, CT* __restrict__ counts, mz_u64 mask, int max_pairs,
                                            int* __restrict__ flags) {
    mz_u64 slot = mz_hash(key) & mask;
    for (mz_u64 probes = 0; probes <= mask; ++probes, slot = (slot + 1) & mask) {
        mz_u64 old = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) {
            if (mz_load(flags + 2) > max_pairs) break;   // the table takes no new keys once it holds more than max_pairs (flags[1] is set below)
            old = atomicCAS(keys + slot, 0ull, key);
            if (old == 0) {
                mz_add(flags + 2, 1);
                old = key;
            }
        }
        if (old == key) {
            mz_add(counts + slot, n);
            return;
        }
    }
    mz_store(flags + 1, 1);
}
// The same table with three 64-bit counts per key, counts i64 [mask + 1, 3] (measure3d.hip: the faces two objects share, per axis): adds n at
// 3 * slot + axis.
__device__ __forceinline__ void mz_pair_add_axis(mz_u64 key, int axis, int n, mz_u64* __restrict__ keys, long* __restrict__ counts, mz_u64 mask,
                                                 int max_pairs, int* __restrict__ flags) {
    mz_u64 slot = mz_hash(key) & mask;
    for (mz_u64 probes = 0; probes <= mask; ++probes, slot = (slot + 1) & mask) {
        mz_u64 old = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) {
            if (mz_load(flags + 2) > max_pairs) break;
            old = atomicCAS(keys + slot, 0ull, key);
            if (old == 0) {
                mz_add(flags + 2, 1);
                old = key;
            }
        }
        if (old == key) {
            mz_add(counts + 3 * slot + axis, n);
            return;
        }
    }
    mz_store(flags + 1, 1);
}
// The same table with a maximum per key instead of a sum (split.hip: the pass between two basins); vals are zeroed by the caller and v > 0.  The
// atomic is sent only when a relaxed load says it improves.
__device__ __forceinline__ void mz_pair_max(mz_u64 key, int v, mz_u64* __restrict__ keys, int* __restrict__ vals, mz_u64 mask, int max_pairs,
                                            int* __restrict__ flags) {
    mz_u64 slot = mz_hash(key) & mask;
    for (mz_u64 probes = 0; probes <= mask; ++probes, slot = (slot + 1) & mask) {
        mz_u64 old = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) {
            if (mz_load(flags + 2) > max_pairs) break;
            old = atomicCAS(keys + slot, 0ull, key);
            if (old == 0) {
                mz_add(flags + 2, 1);
                old = key;
            }
        }
        if (old == key) {
            if (mz_load(vals + slot) < v) mz_max(vals + slot, v);
            return;
        }
    }
    mz_store(flags + 1, 1);
}
