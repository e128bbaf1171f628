// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32 with its default 10
// rounds): word 0 of the block with key (k0, k1) and counter (c0, c1, c2, c3).  Shared by the fused sampler (llm_misc.hip) and the prompt draws
// (prompts.hip); the host mirror is ullsam_amd/sampling.py philox4x32_10.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned int philox4x32_10_word0(unsigned int k0, unsigned int k1, unsigned int c0, unsigned int c1, unsigned int c2,
                                                            unsigned int c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned int h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned int h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
