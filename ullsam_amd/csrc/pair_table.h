// The row runs and the pair table of the label-image kernels, on top of label_common.h: runs of equal keys along a row (one atomic per run), and the
// open-addressing table of id pairs in global memory (mosaic, stack, split*, measure*: seams, links, passes, contacts).  Integer work only; what
// the table holds at the end does not depend on the order of arrival.
#pragma once
#include "label_common.h"

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
// The probe loop: use(slot) is called with the slot of `key`, claimed if need be; flags[1] is set instead when the table refuses the key.  (A
// form that returns the slot, or -1, changes the code of every kernel that counts pairs; this one compiles to what the three copies did.)
template <class F>
__device__ __forceinline__ void mz_pair_slot(mz_u64 key, mz_u64* __restrict__ keys, mz_u64 mask, int max_pairs, int* __restrict__ flags, F use) {
    mz_u64 slot = mz_hash(key) & mask;
    for (mz_u64 probes = 0; probes <= mask; ++probes, slot = (slot + 1) & mask) {
        mz_u64 old = mz_load(keys + slot);
        if (old == 0) {
            if (mz_load(flags + 2) > max_pairs) break;   // the table takes no new keys once it holds more than max_pairs (flags[1] is set below)
            old = atomicCAS(keys + slot, 0ull, key);
            if (old == 0) {
                mz_add(flags + 2, 1);
                old = key;
            }
        }
        if (old == key) {
            use(slot);
            return;
        }
    }
    mz_store(flags + 1, 1);
}
// the pair key of two neighbouring ids: smaller << 32 | larger, 0 (nothing to count) unless both are positive and differ
__device__ __forceinline__ mz_u64 mz_pair_key(int a, int b) {
    if (a <= 0 || b <= 0 || a == b) return 0;
    return a < b ? ((mz_u64)a << 32) | (mz_u64)b : ((mz_u64)b << 32) | (mz_u64)a;
}
template <class CT>
__device__ __forceinline__ void mz_pair_add(mz_u64 key, int n, mz_u64* __restrict__ keys, CT* __restrict__ counts, mz_u64 mask, int max_pairs,
                                            int* __restrict__ flags) {
    mz_pair_slot(key, keys, mask, max_pairs, flags, [&](mz_u64 slot) { mz_add(counts + slot, n); });
}
// The same table with three 64-bit counts per key, counts i64 [mask + 1, 3] (measure3d.hip: the faces two objects share, per axis): adds n at
// 3 * slot + axis.
__device__ __forceinline__ void mz_pair_add_axis(mz_u64 key, int axis, int n, mz_u64* __restrict__ keys, long* __restrict__ counts, mz_u64 mask,
                                                 int max_pairs, int* __restrict__ flags) {
    mz_pair_slot(key, keys, mask, max_pairs, flags, [&](mz_u64 slot) { mz_add(counts + 3 * slot + axis, n); });
}
// The same table with a maximum per key instead of a sum (split.hip: the pass between two basins); vals are zeroed by the caller and v > 0.
__device__ __forceinline__ void mz_pair_max(mz_u64 key, int v, mz_u64* __restrict__ keys, int* __restrict__ vals, mz_u64 mask, int max_pairs,
                                            int* __restrict__ flags) {
    mz_pair_slot(key, keys, mask, max_pairs, flags, [&](mz_u64 slot) { mz_send_max(vals + slot, v); });
}
