"""Host mirror of the random numbers of the fused sampler (ullsam_sample_topk_topp, csrc/llm_misc.hip): Philox4x32-10 (Salmon, Moraes, Dror, Shaw:
"Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library's philox4x32 with its default 10 rounds) in numpy integers.

A sequence's uniform at a decode step is a function of (its seed, the step) alone:
    key = (seed & 0xffffffff, seed >> 32), counter = (step & 0xffffffff, step >> 32, 0, 0), u = (word 0 >> 8) * 2^-24 in [0, 1)."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # key increments (golden ratio, sqrt(3) - 1)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """counter [..., 4], key [..., 2] (broadcast against each other; 32-bit words as any integer type) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _M32
    k = np.asarray(key, dtype=np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(W0)) & _M32, (k1 + np.uint64(W1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def row_seeds(seed, B: int) -> np.ndarray:
    """uint64 [B]: an int s -> (s + b) mod 2^64 for sequence b; a sequence of B ints -> those (mod 2^64)."""
    if isinstance(seed, (int, np.integer)):
        return np.array([(int(seed) + b) % (1 << 64) for b in range(B)], dtype=np.uint64)
    vals = [int(s) % (1 << 64) for s in (seed.tolist() if hasattr(seed, "tolist") else seed)]
    if len(vals) != B:
        raise ValueError(f"seed: {len(vals)} values for a batch of {B}")
    return np.array(vals, dtype=np.uint64)


def uniforms(seeds, step: int) -> np.ndarray:
    """float32 [B]: the uniform each sequence draws at `step` (bit-equal to the kernel's)."""
    s = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))
    step = int(step) % (1 << 64)
    key = np.stack([s & _M32, s >> np.uint64(32)], -1)
    ctr = np.array([step & 0xFFFFFFFF, step >> 32, 0, 0], dtype=np.uint64)
    w0 = philox4x32_10(ctr, key)[..., 0]
    return ((w0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
